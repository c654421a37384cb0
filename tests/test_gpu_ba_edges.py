"""The dense BA on the device off the smooth trajectory: pixels behind the camera, pixels / edges / frames without weight,
rejected and clamped disparity steps, ragged plans, source frames of 7 / 9 / 17 terms, M > 4096 terms, more than 1024
disparity frames - and a factorisation that fails.

Cases: oracle/ba_cases.py (tests/test_oracle_ba_cases.py proves on the CPU what each one reaches, that none sits on a
branch, and that an oracle with one branch wrong leaves the tolerance used here).  Tolerance, relative to the STEP: per
output 4 x delta32, delta32 = the distance between the oracle in float32 and in float64 on that case (the margin is for
the other summation order of atomics and matrix cores; the kernels keep the reduced system in fp64), never looser than
the suite's 1e-4 form (`ba_cases.step_bounds`).  Every call works in buffers with two frames beyond the graph.
"""

import os

import numpy as np
import pytest
import torch

from oracle import ba_cases as bc
from oracle import se3 as ose3
from vipe_amd.synth import expand_edges, make_graph

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GUARD = 2  # frames beyond the graph in the pose and disparity buffers


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def _padded(a, rows, fill):
    """[rows + extra, ...] float32: `a` and then sentinel rows cycling through `fill`"""
    a = np.asarray(a, np.float32)
    tail = np.resize(np.asarray(fill, np.float32), (rows,) + a.shape[1:])
    return np.concatenate([a, tail])


def run_case(c, opts=0):
    """`slam_ext.dense_ba` on a case, in buffers of n + GUARD poses / (n + GUARD) V frames.  The sentinel poses must keep
    their bits; the sentinel disparities (0.5 and 1e-5 in turn) change only by the clamp at 1e-3 of the whole buffer
    (buffer.py:525).  -> poses [n,7], disps like g.disps, intrinsics, rig, info"""
    from vipe_amd.ext import slam_ext
    g = c.g
    V = g.V if c.rig else 1
    n, ht, wd = g.n, g.ht, g.wd
    pi, qi, di, pj, qj = expand_edges(g.ii, g.jj, V)
    M = len(pi)
    flat = lambda a: np.asarray(a).reshape(n * V, ht, wd)
    sentinel_pose = np.array([[0.3, -0.2, 0.1, 0.5, -0.5, 0.5, 0.5], [7.0, 8.0, 9.0, 0.0, 0.6, 0.0, 0.8]], np.float32)
    poses = T(_padded(g.poses, GUARD, sentinel_pose))
    disps = T(_padded(flat(g.disps), GUARD * V, [0.5, 1e-5]))
    sens = T(_padded(flat(g.disps_sens), GUARD * V, [0.0]))
    eta = T(_padded(flat(g.eta), GUARD * V, [0.01]))
    intr = T(c.intr).clone()
    rig = T(g.rig if c.rig else ose3.se3_identity(1)).clone()
    tail_p, tail_d = poses[n:].clone(), disps[n * V:].clone()
    info = slam_ext.dense_ba(poses, disps, sens, intr, rig, T(g.target.reshape(M, -1, 2)), T(g.weight.reshape(M, -1, 2)), eta,
                             T(pi), T(qi), T(pj), T(qj), T(di), camera=c.cam, want_info=True, solver_options=opts, **c.bk)
    torch.cuda.synchronize()
    assert torch.equal(poses[n:].view(torch.int32), tail_p.view(torch.int32)), "a pose beyond the graph was written"
    assert torch.equal(disps[n * V:], tail_d.clamp(min=1e-3)), "disparities beyond the graph: only the 1e-3 clamp may act"
    return (poses[:n].cpu().numpy(), disps[:n * V].cpu().numpy().reshape(g.disps.shape), intr.cpu().numpy(),
            rig.cpu().numpy(), info.cpu().numpy())


def _option_sets():
    from vipe_amd.ext import slam_ext
    return {"default": 0, "general": slam_ext.BA_OPT_ONE_CHAIN | slam_ext.BA_OPT_GENERAL_ACCUMULATE}


def _check(name, tag, got):
    """against the float64 oracle at the step tolerance, against the reference Solver's outputs at the 1e-4 form, and the
    plan's counts against the oracle's sets"""
    c = bc.case(name)
    p, d, k, r, info = got
    o64 = bc.oracle_run(name)
    bounds = bc.step_bounds(name)
    n_free, n_fd, n_unknown = bc.counts(name)
    assert info[2] == 0, "Cholesky must not fail"
    assert (info[0], info[1], info[3]) == (n_free, n_fd, n_unknown), info
    outs = {"poses": p, "disps": d.reshape(o64[1].shape), "intr": k, "rig": r}
    errs = {}
    for (key, (d32, bound)), ref in zip(bounds.items(), o64):
        errs[key] = float(np.nan_to_num(np.abs(outs[key].astype(np.float64) - ref), nan=np.inf).max())
        ratio = errs[key] / d32 if d32 > 0 else (0.0 if errs[key] == 0 else np.inf)
        print(f"{name} [{tag}] {key}: kernel error {errs[key]:.3g}, delta32 {d32:.3g}, ratio {ratio:.3g}, bound {bound:.3g}")
    for key, (d32, bound) in bounds.items():
        assert errs[key] <= bound, (name, tag, key, errs[key], d32, bound)
    G = np.load(os.path.join(GOLD, "ba_edges_reference.npz"))
    rp, rd, rk, rr = (G[f"{name}/{x}"] for x in ("poses", "disps", "intrinsics", "rig"))
    assert np.abs(p - rp).max() <= 1e-4 * max(1.0, np.abs(rp).max())
    assert np.abs(d - rd).max() <= 1e-4 * np.abs(rd).max()
    assert np.abs(k - rk).max() <= 1e-4 * np.abs(rk).max()
    assert np.abs(r - rr).max() <= 1e-4
    if not c.bk.get("optimize_intrinsics"):
        assert np.array_equal(k, c.intr)


@pytest.mark.parametrize("tag", ["default", "general"])
@pytest.mark.parametrize("name", bc.MONO)
def test_dense_ba_edge_case_within_the_step_tolerance(name, tag):
    """mono cases under the default kernel selection (fused matrix-core accumulate where the degree allows, two-chain band
    solve) and under BA_OPT_ONE_CHAIN | BA_OPT_GENERAL_ACCUMULATE (the walk kernel): both must see every branch"""
    _check(name, tag, run_case(bc.case(name), _option_sets()[tag]))


def test_dense_ba_rig_of_more_than_1024_disparity_frames():
    """8 views x (129 + 2) keyframes: the second trip of the plan's 1024-lane loops and two entries per lane in its scans;
    rig rotation and per-view intrinsics on (818 unknowns)"""
    _check("rig8_n129", "default", run_case(bc.case("rig8_n129")))


@pytest.mark.parametrize("kind", ["band", "dense", "global"])
def test_dense_ba_failed_factorisation_takes_a_zero_step(kind):
    """One NaN in a target, at a pixel with weight, on the three graphs of
    test_dense_ba_path_hints_across_calls_with_one_plan (band solver, LDS dense solver, tiled Cholesky), two iterations in
    one call.  "Zero step on a failed factorisation": the failure is counted, the solver that owns the system is the one
    that reports, no pose moves, and every disparity comes back finite and >= 1e-3 (the pixels the NaN reached are set to
    the clamp value)."""
    from vipe_amd.ext import slam_ext
    g = {"band": lambda: make_graph(n=14, height=96, width=128, radius=2, seed=71),
         "dense": lambda: make_graph(n=20, height=96, width=128, radius=19, seed=91),
         "global": lambda: make_graph(n=70, height=96, width=128, radius=3, extra_edges=260, seed=101)}[kind]()
    n, E, P = len(g.poses), len(g.ii), g.ht * g.wd
    e, px = E // 2, P // 2
    tgt, w = g.target.reshape(E, P, 2).copy(), g.weight.reshape(E, P, 2)
    assert w[e, px, 0] > 0.01 and w[e, px, 1] > 0.01 and 1 <= g.ii[e] < n and 1 <= g.jj[e] < n
    tgt[e, px, 0] = np.nan
    z = np.zeros_like(g.ii)
    poses, disps = T(g.poses).clone(), T(g.disps).clone()
    info = slam_ext.dense_ba(poses, disps, T(g.disps_sens), T(g.intrinsics), T(ose3.se3_identity(1)), T(tgt), T(w), T(g.eta),
                             T(g.ii), T(z), T(g.jj), T(z), T(g.ii), want_info=True, t0=1, t1=n, n_iters=2, pose_damping=1e-3,
                             pose_ep=0.1)
    torch.cuda.synchronize()
    info, p, d = info.cpu().numpy(), poses.cpu().numpy(), disps.cpu().numpy()
    print(kind, "info", info, "max pose change", np.abs(p - g.poses).max(), "non-finite disparities", (~np.isfinite(d)).sum())
    assert info[2] >= 1, info
    assert info[5] == {"band": 1, "dense": 2, "global": 0}[kind], info
    assert np.isfinite(p).all() and np.abs(p - g.poses).max() <= 1e-6
    assert np.isfinite(d).all() and d.min() >= 1e-3
