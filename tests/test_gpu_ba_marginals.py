"""Marginal covariances of the dense BA on the device (`slam_ext.dense_ba_marginals`: vipe_dense_ba_linearize, the float64
inverse of the reduced system, ba_disp_variance_kernel) against the float64 numpy reference of
tests/ba_marginals_reference.py, which tests/test_ba_marginals_reference.py ties to the pinned solver.

Cases (oracle/ba_cases.py, the smallest problems that reach each path): ragged_plan (13 x 17, one partial tile; fixed
sources, a target-only free pose, a pose without edges, duplicated edges), the same with the shared intrinsics (E_f, mono
tail), behind_mei (zero validity weights, MEI) and behind_pinhole (both 17 x 19: a second, partial tile), deg9_17 (walk +
Schur accumulate, more than 6 members; also under BA_OPT_GENERAL_ACCUMULATE), m4160 (64 terms per frame: 390 rows of E per
pixel, 153 chunk pairs of the variance kernel, n = 384), rig8_n129 (8 views, E_t tail, 818 unknowns).

Tolerance per output, relative per element (`ba_marginals_reference.rel_err_var` / `rel_err_cov`): 4 x delta32, delta32 =
the distance between the reference in float32 and in float64 on that case, never looser than 1e-4 - the convention of
`oracle.ba_cases.step_bounds`.  Every call works in buffers with two frames beyond the graph.
"""

import numpy as np
import pytest
import torch

import ba_marginals_reference as mr
from oracle import ba_cases as bc
from oracle import se3 as ose3
from vipe_amd.synth import expand_edges

pytestmark = pytest.mark.gpu

GUARD = 2


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _padded(a, rows, fill):
    a = np.asarray(a, np.float32)
    return np.concatenate([a, np.resize(np.asarray(fill, np.float32), (rows,) + a.shape[1:])])


def case_tensors(name):
    """device arguments of `dense_ba` / `dense_ba_marginals` for a case, in buffers of n + GUARD poses"""
    c = bc.case(name)
    g = c.g
    V = g.V if c.rig else 1
    n, ht, wd = g.n, g.ht, g.wd
    pi, qi, di, pj, qj = expand_edges(g.ii, g.jj, V)
    M = len(pi)
    flat = lambda a: np.asarray(a).reshape(n * V, ht, wd)
    sentinel_pose = np.array([[0.3, -0.2, 0.1, 0.5, -0.5, 0.5, 0.5], [7.0, 8.0, 9.0, 0.0, 0.6, 0.0, 0.8]], np.float32)
    state = [T(_padded(g.poses, GUARD, sentinel_pose)), T(_padded(flat(g.disps), GUARD * V, [0.5, 1e-5])),
             T(_padded(flat(g.disps_sens), GUARD * V, [0.0])), T(c.intr).clone(),
             T(g.rig if c.rig else ose3.se3_identity(1)).clone()]
    data = [T(g.target.reshape(M, -1, 2)), T(g.weight.reshape(M, -1, 2)), T(_padded(flat(g.eta), GUARD * V, [0.01]))]
    idx = [T(pi), T(qi), T(pj), T(qj), T(di)]
    kw = {k: v for k, v in c.bk.items() if k != "n_iters"}
    return c, state + data + idx, dict(kw, camera=c.cam)


def run_marginals(tag, opts=0, **over):
    """-> (disp_var [nF + guard, P], pose_cov [n + guard, 6, 6], info, again) as numpy.  Checks on the way: `linearize`
    leaves the state arrays bitwise alone; the marginals stage (no atomics, plain stores) gives the same bits when it runs
    again on the same linearisation and inverse.  Two WHOLE calls cannot be bitwise equal: the accumulate kernels sum the
    reduced system with atomics (f32 in LDS, fp64 in memory) in an order that changes from launch to launch.  `again` =
    the relative distance in disp_var between two whole calls; each lies within the case's bound of the reference, so
    `check_against` holds it to twice that bound."""
    from vipe_amd.ext import slam_ext
    name, case_over = mr.CASES[tag]
    c, args, kw = case_tensors(name)
    kw = dict(kw, **case_over, **over)
    before = [a.clone() for a in args[:5]]
    S, info, ctx = slam_ext.dense_ba_linearize(*args, solver_options=opts, **kw)
    torch.cuda.synchronize()
    for a, b, what in zip(args[:5], before, ("poses", "disps", "disps_sens", "intrinsics", "rig")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what} was written"
    Sinv = slam_ext.invert_reduced_system(S) if S.shape[0] else None
    dv, pc = slam_ext.dense_ba_marginals_apply(ctx, Sinv)
    dv2, pc2 = slam_ext.dense_ba_marginals_apply(ctx, Sinv)
    torch.cuda.synchronize()
    assert torch.equal(dv.view(torch.int32), dv2.view(torch.int32)), "disp_var differs between two calls"
    assert torch.equal(pc.view(torch.int64), pc2.view(torch.int64)), "pose_cov differs between two calls"
    dv3, pc3, _ = slam_ext.dense_ba_marginals(*args, solver_options=opts, **kw)
    m = torch.isfinite(dv)
    again = float(((dv3[m] - dv[m]).abs() / dv[m]).max()) if m.any() else 0.0
    print(f"{tag}: a second whole call differs by {again:.3g} relative in disp_var")
    assert torch.equal(torch.isnan(dv3), torch.isnan(dv)) and torch.equal(torch.isnan(pc3), torch.isnan(pc))
    return dv.cpu().numpy().reshape(dv.shape[0], -1), pc.cpu().numpy(), info.cpu().numpy(), again


def check_against(tag, what, got, ref, bounds):
    """`got` with GUARD frames beyond the graph against a reference namespace; -> error / bound ratios"""
    dv, pc, info, again = got
    nF, n = ref.disp_var.shape[0], ref.pose_cov.shape[0]
    # rows that are not free keep the NaN prefill - in the graph and beyond it - and free rows are written everywhere
    assert np.array_equal(np.isnan(dv[:nF]), np.isnan(ref.disp_var)), "disp_var: written rows differ from the free frames"
    assert np.array_equal(np.isnan(pc[:n]), np.isnan(ref.pose_cov)), "pose_cov: written rows differ from the free poses"
    assert np.isnan(dv[nF:]).all() and np.isnan(pc[n:]).all(), "a row beyond the graph was written"
    assert (info[0], info[1], info[3]) == (len(ref.lin.free_pose), len(ref.lin.free_disp), ref.lin.n), info
    (d_v, b_v), (d_c, b_c) = bounds
    e_v, e_c = mr.rel_err_var(dv[:nF], ref.disp_var), mr.rel_err_cov(pc[:n], ref.pose_cov)
    print(f"{tag} [{what}] disp_var: error {e_v:.3g}, delta32 {d_v:.3g}, bound {b_v:.3g}, error/bound {e_v / b_v:.3g}")
    print(f"{tag} [{what}] pose_cov: error {e_c:.3g}, delta32 {d_c:.3g}, bound {b_c:.3g}, error/bound {e_c / b_c:.3g}")
    if len(ref.lin.free_disp):
        m = np.isfinite(ref.disp_var)
        assert (dv[:nF][m] > 0).all()
    assert e_v <= b_v, (tag, what, "disp_var", e_v, d_v, b_v)
    assert again <= 2 * b_v, (tag, what, "two whole calls", again, b_v)
    assert e_c <= b_c, (tag, what, "pose_cov", e_c, d_c, b_c)


@pytest.mark.parametrize("tag", sorted(mr.CASES))
def test_marginals_match_the_float64_reference(tag):
    check_against(tag, "default", run_marginals(tag), mr.case_marginals(tag), mr.bounds(tag))


def test_marginals_under_the_general_accumulate_agree():
    """deg9_17 takes the walk + Schur pair by its degree; ragged_plan only when asked to: both forms leave the same blocks"""
    from vipe_amd.ext import slam_ext
    for tag in ("deg9_17", "ragged_plan"):
        got = run_marginals(tag, opts=slam_ext.BA_OPT_GENERAL_ACCUMULATE)
        check_against(tag, "general", got, mr.case_marginals(tag), mr.bounds(tag))


def test_motion_only_and_no_terms_write_pose_rows_only():
    from vipe_amd.ext import slam_ext
    args, kw = mr.case_kwargs("ragged_plan")
    kw = dict(kw, motion_only=True)
    ref64, ref32 = (mr.marginals(*args, dtype=dt, **kw) for dt in (np.float64, np.float32))
    assert not ref64.lin.free_disp and len(ref64.lin.free_pose) > 0
    d_c = mr.rel_err_cov(ref32.pose_cov, ref64.pose_cov)
    got = run_marginals("ragged_plan", motion_only=True)
    assert np.isnan(got[0]).all()
    check_against("ragged_plan", "motion_only", got, ref64, ((0.0, 1e-4), (d_c, min(4 * d_c, 1e-4))))
    # M = 0: nothing is free, nothing is written, VIPE_OK
    c, targs, tkw = case_tensors("ragged_plan")
    P = c.g.ht * c.g.wd
    empty = [torch.zeros((0, P, 2), device=dev()), torch.zeros((0, P, 2), device=dev()), targs[7]]
    noidx = [torch.zeros(0, dtype=torch.int64, device=dev()) for _ in range(5)]
    dv, pc, info = slam_ext.dense_ba_marginals(*targs[:5], *empty, *noidx, **tkw)
    torch.cuda.synchronize()
    assert torch.isnan(dv).all() and torch.isnan(pc).all() and int(info[0]) == 0 and int(info[3]) == 0


def test_more_than_eight_views_is_unsupported():
    from vipe_amd.ext import slam_ext
    d = dev()
    V, n, ht, wd = 9, 2, 4, 6
    f = lambda *s: torch.ones(s, device=d)
    rig = torch.tensor(ose3.se3_identity(V), dtype=torch.float32, device=d)
    poses = torch.tensor(ose3.se3_identity(n), dtype=torch.float32, device=d)
    idx = [torch.zeros(V, dtype=torch.int64, device=d) for _ in range(5)]
    with pytest.raises(NotImplementedError):
        slam_ext.dense_ba_marginals(poses, f(n * V, ht, wd), f(n * V, ht, wd), f(V, 4), rig, f(V, ht * wd, 2), f(V, ht * wd, 2),
                                    f(n * V, ht, wd), *idx, t0=1, t1=2, pose_damping=1e-3, pose_ep=0.1)


def test_a_reused_plan_survives_a_marginals_call_in_its_workspace():
    """dense_ba, dense_ba (plan reused) against dense_ba, marginals, dense_ba (plan reused) in one private workspace: the
    marginals leave S / Hd zero and the plan intact, so the last call computes the same step"""
    from vipe_amd.ext import slam_ext
    name = "ragged_plan"
    outs = []
    for with_marginals in (False, True):
        c, args, kw = case_tensors(name)
        state = {}
        slam_ext.dense_ba(*args, n_iters=1, state=state, plan_key=7, **kw)
        if with_marginals:
            key = state["key"]
            slam_ext.dense_ba_marginals(*args, state=state, plan_key=7, **kw)
            assert state["key"] == key and key is not None, "the marginals call must keep the plan of this workspace valid"
        slam_ext.dense_ba(*args, n_iters=1, state=state, plan_key=7, **kw)
        torch.cuda.synchronize()
        outs.append([a.cpu().numpy().astype(np.float64) for a in args[:2]])
    bounds = bc.step_bounds(name)
    n, nF = c.g.n, c.g.n
    e_p = np.abs(outs[0][0][:n] - outs[1][0][:n]).max()
    e_d = np.abs(outs[0][1][:nF] - outs[1][1][:nF]).max()
    print(f"reuse after marginals: poses {e_p:.3g} (bound {bounds['poses'][1]:.3g}), disps {e_d:.3g} (bound {bounds['disps'][1]:.3g})")
    assert e_p <= bounds["poses"][1] and e_d <= bounds["disps"][1]
    assert np.array_equal(outs[0][0][n:], outs[1][0][n:])
