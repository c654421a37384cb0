"""The dense BA on the device off the smooth trajectory: pixels behind the camera, pixels / edges / frames without weight,
rejected and clamped disparity steps, ragged plans, source frames of 7 / 9 / 17 terms, M > 4096 terms, more than 1024
disparity frames - and a factorisation that fails, in each of the four solvers.

Cases: oracle/ba_cases.py (tests/test_oracle_ba_cases.py proves on the CPU what each one reaches, that none sits on a
branch, and that an oracle with one branch wrong leaves the tolerance used here).  Tolerance, relative to the STEP: per
output 4 x delta32, delta32 = the distance between the oracle in float32 and in float64 on that case (the margin is for
the other summation order of atomics and matrix cores; the kernels keep the reduced system in fp64), never looser than
the suite's 1e-4 form (`ba_cases.step_bounds`).  Every call works in buffers with two frames beyond the graph.
"""

import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from ba_device import T, check_outputs, run_case
from ba_device import option_sets as _option_sets
from oracle import ba_cases as bc
from oracle import ba_route as br
from oracle import se3 as ose3
from oracle import solver_cases as sc
from vipe_amd.synth import expand_edges, make_graph

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    check_outputs(name, tag, got, o64, bounds)
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


def _failing_case(kind):
    """the graphs of test_dense_ba_path_hints_across_calls_with_one_plan, pose-only, and the two single-workgroup systems
    of oracle/solver_cases.py (n = 175 with the focal length; the rig with intrinsics and rig rotations, n = 254)"""
    if kind.startswith("one_workgroup"):
        return sc.case({"one_workgroup": "wg175", "one_workgroup_rig": "wg254_rig"}[kind])
    g = {"band": lambda: make_graph(n=14, height=96, width=128, radius=2, seed=71),
         "dense": lambda: make_graph(n=20, height=96, width=128, radius=19, seed=91),
         "global": lambda: make_graph(n=70, height=96, width=128, radius=3, extra_edges=260, seed=101)}[kind]()
    return SimpleNamespace(g=g, cam="pinhole", intr=g.intrinsics, rig=False,
                           bk=dict(t0=1, t1=g.n, n_iters=2, pose_damping=1e-3, pose_ep=0.1))


@pytest.mark.parametrize("kind", ["band", "dense", "global", "one_workgroup", "one_workgroup_rig"])
def test_dense_ba_failed_factorisation_takes_a_zero_step(kind):
    """One NaN in a target, at a pixel with weight, on the three graphs of
    test_dense_ba_path_hints_across_calls_with_one_plan (band solver, LDS dense solver, tiled Cholesky) and on two systems
    of the single-workgroup global-memory Cholesky (its `sh.fail` path; mono with the focal length, and a rig with eight
    tail rows), two iterations in one call.  "Zero step on a failed factorisation": the failure is counted, the solver that
    owns the system is the one that reports, no pose (intrinsic, rig transform) moves, and every disparity comes back
    finite and >= 1e-3 (the pixels the NaN reached are set to the clamp value)."""
    from vipe_amd.ext import slam_ext
    c = _failing_case(kind)
    g, V = c.g, (c.g.V if c.rig else 1)
    pi, qi, di, pj, qj = expand_edges(g.ii, g.jj, V)
    n, M, P = len(g.poses), len(pi), g.ht * g.wd
    e, px = M // 2, P // 2
    tgt, w = g.target.reshape(M, P, 2).copy(), g.weight.reshape(M, P, 2)
    assert w[e, px, 0] > 0.01 and w[e, px, 1] > 0.01 and 1 <= pi[e] < n and 1 <= pj[e] < n
    tgt[e, px, 0] = np.nan
    if kind.startswith("one_workgroup"):
        assert br.global_form(*sc.route_args(c.name)) == "one_workgroup"
    rig0 = g.rig if c.rig else ose3.se3_identity(1)
    poses, disps, intr, rig = T(g.poses).clone(), T(g.disps.reshape(n * V, g.ht, g.wd)).clone(), T(c.intr).clone(), T(rig0).clone()
    info = slam_ext.dense_ba(poses, disps, T(g.disps_sens.reshape(n * V, g.ht, g.wd)), intr, rig, T(tgt), T(w),
                             T(g.eta.reshape(n * V, g.ht, g.wd)), T(pi), T(qi), T(pj), T(qj), T(di), camera=c.cam, want_info=True,
                             **c.bk)
    torch.cuda.synchronize()
    info, p, d = info.cpu().numpy(), poses.cpu().numpy(), disps.cpu().numpy()
    print(kind, "info", info, "max pose change", np.abs(p - g.poses).max(), "non-finite disparities", (~np.isfinite(d)).sum())
    assert info[2] >= 1, info
    assert info[5] == {"band": 1, "dense": 2, "global": 0, "one_workgroup": 0, "one_workgroup_rig": 0}[kind], info
    assert np.isfinite(p).all() and np.abs(p - g.poses).max() <= 1e-6
    assert np.isfinite(d).all() and d.min() >= 1e-3
    k, r = intr.cpu().numpy(), rig.cpu().numpy()
    assert np.array_equal(k, c.intr) and np.isfinite(r).all() and np.abs(r - rig0).max() <= 1e-6
