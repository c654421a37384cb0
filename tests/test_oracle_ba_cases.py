"""The dense-BA cases of oracle/ba_cases.py, proved on the CPU: each reaches the branch it was built for (counted from the
oracle's debug output), none sits on a knife edge of a branch, the float64 oracle agrees with the reference Solver's
recorded outputs on all of them (tests/golden/ba_edges_reference.npz, make_golden.gen_ba_edges), and an oracle with one
of those branches wrong leaves the tolerance the GPU test (tests/test_gpu_ba_edges.py) holds the kernels to.
"""

import os

import numpy as np
import pytest

from oracle import ba, geom, se3
from oracle import ba_cases as bc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ID7 = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _debug(name):
    return bc.oracle_run(name, "float64", True)[4]


def _dz(d):
    """[frames, P] of one iteration's disparity steps before the rejection, in the order of d["free_disp"]"""
    return np.stack([d["dz"][k] for k in d["free_disp"]])


# ------------------------------------------------------------------------------------------------ by hand


def _one_pixel(pose_j, disp, target, weight=1000.0, t0=0, t1=0):
    """one term 0 -> 1 on a 1 x 1 grid, fx = fy = 1 and cx = cy = 0 at grid scale, eta = 0 -> (poses, disparity of frame 0)"""
    one = lambda v: np.full((2, 1, 1, 1), v, dtype=np.float64)
    p, d, _, _ = ba.bundle_adjustment(np.stack([ID7, pose_j]), one(disp), one(0.0), np.array([[8.0, 8.0, 0.0, 0.0]]), ID7[None],
                                      np.array(target, dtype=np.float64).reshape(1, 1, 2), np.full((1, 1, 2), weight), one(0.0),
                                      [0], [1], t0=t0, t1=t1, n_iters=1, pose_damping=1e-3, pose_ep=0.1)
    return p, d[0, 0, 0, 0]


def test_by_hand_a_pixel_behind_min_depth_carries_nothing():
    """X1 = (0.5 d, 0, 1 - 0.5 d): at d = 1.9 the depth is 0.05 < MIN_DEPTH, the term's weight is zero whatever the
    residual (here 1000 weight x a 3 px residual), so neither pose 1 nor the disparity moves; at d = 1 (Z = 0.5) both do."""
    pose_j = np.array([0.5, 0, -0.5, 0, 0, 0, 1.0])
    p, d = _one_pixel(pose_j, 1.9, [3.0, 0.0], t0=1, t1=2)
    assert np.array_equal(p[1], pose_j) and d == 1.9
    p, d = _one_pixel(pose_j, 1.0, [3.0, 0.0], t0=1, t1=2)
    assert not np.array_equal(p[1], pose_j) and abs(d - 1.0) > 1e-3  # (the disparity takes nearly all of it)


def test_by_hand_a_step_of_twelve_is_rejected_and_minus_twelve_is_not():
    """Poses fixed, X1 = (0.5 d, 0, 1): coords = (0.5 d, 0), Jz = (0.5, 0), w = 1, C = 0.25 + 2e-7.  A target 6 px to the
    right asks for dz = 3 / C = 12 (1 - 8e-7): rejected, the disparity stays.  6 px to the left: dz = -12 is applied,
    d = 1 - 12 < 0 and the final clamp makes it 1e-3.  4 px to the right: dz = 8, applied."""
    pose_j = np.array([0.5, 0, 0, 0, 0, 0, 1.0])
    assert _one_pixel(pose_j, 1.0, [6.5, 0.0])[1] == 1.0
    assert _one_pixel(pose_j, 1.0, [-5.5, 0.0])[1] == 1e-3
    assert _one_pixel(pose_j, 1.0, [4.5, 0.0])[1] == pytest.approx(1.0 + 2.0 / (0.25 + 2e-7), rel=1e-12)


# ------------------------------------------------------------------------------------------------ branch reach


@pytest.mark.parametrize("cam", ["pinhole", "mei"])
def test_behind_reaches_the_validity_branches(cam):
    c = bc.case("behind_" + cam)
    assert c.g.ht * c.g.wd == 323 and len(c.g.ii) == 14 and (c.g.poses[:, 6] < 0).sum() == 2
    assert c.g.disps[0].max() > 11.5
    rel = se3.se3_mul(c.g.poses[c.g.jj].astype(np.float64), se3.se3_inv(c.g.poses[c.g.ii].astype(np.float64)))
    ang = 2 * np.arctan2(np.linalg.norm(rel[:, 3:6], axis=-1), np.abs(rel[:, 6]))
    assert 1.9 < ang.max() < 2.1
    for d in _debug(c.name):
        Z = d["Z"]
        share, neg = (Z < geom.MIN_DEPTH).mean(), (Z < 0).mean()
        print(c.name, "Z < 0.1:", share, "Z < 0:", neg)
        assert 0.05 <= share <= 0.30 and neg >= 0.02
        assert np.array_equal(d["valid"], Z > geom.MIN_DEPTH)
        per_term = (Z < geom.MIN_DEPTH).mean(1)
        assert (per_term > 0.75).sum() >= 2 and ((per_term > 0.02) & (per_term < 0.98)).sum() >= 6  # (nearly) whole terms, partial ones
        assert (per_term == 0).sum() >= 2


def test_zero_support_reaches_what_it_claims():
    c = bc.case("zero_support")
    g = c.g
    E, P = len(g.ii), g.ht * g.wd
    w = g.weight.reshape(E, P, 2)
    assert P == 221 and g.n == 6
    ordinary = (np.arange(E) != bc.ZS_EDGE) & (g.ii != bc.ZS_FRAME)
    both, one = (w == 0).all(-1)[ordinary], ((w == 0).sum(-1) == 1)[ordinary]
    print("both zero", both.mean(), "one zero", one.mean())
    assert 0.27 < both.mean() < 0.33 and 0.17 < one.mean() < 0.23
    assert g.ii[bc.ZS_EDGE] != bc.ZS_FRAME and not w[bc.ZS_EDGE].any()
    assert (g.ii == bc.ZS_FRAME).sum() == 4 and not w[g.ii == bc.ZS_FRAME].any() and not g.eta[bc.ZS_FRAME].any()
    for d in _debug(c.name):
        assert bc.ZS_FRAME in d["free_pose"] and bc.ZS_FRAME in d["free_disp"]
        assert np.array_equal(d["C"][bc.ZS_FRAME], np.full(P, 1e-7 + (0.2 * 0.0 + 1e-7)))  # damping only
        assert not d["dz"][bc.ZS_FRAME].any()
        # pixels of other frames without weight in any of their terms: C is their damping alone, and they stay
        for k in set(d["free_disp"]) - {bc.ZS_FRAME}:
            dead = ~w[g.ii == k].any(axis=(0, 2))
            assert not d["dz"][k][dead].any()


def test_reject_and_clamp_reaches_what_it_claims():
    c = bc.case("reject_and_clamp")
    g = c.g
    sgn = bc.reject_pixels().reshape(g.n, -1)
    pos, neg = sgn > 0, sgn < 0
    n_hit = int((sgn != 0).sum())
    assert 0.03 < n_hit / sgn.size < 0.07 and pos.sum() >= 20 and neg.sum() >= 20
    dbg = _debug(c.name)
    dz0, dz1 = _dz(dbg[0]), _dz(dbg[1])
    assert dbg[0]["free_disp"] == list(range(g.n))
    print("rejected:", np.sort(dz0[pos])[[0, -1]], "applied:", np.sort(dz0[neg])[[0, -1]], "others:", np.abs(dz0[sgn == 0]).max())
    assert (dz0[pos] > 11).all() and (dz0[pos] < 100).all() and (dz0[neg] < -11).all()
    assert np.abs(dz0[sgn == 0]).max() < 5 and np.abs(dz1[sgn == 0]).max() < 5
    assert (dz1[pos] > 11).all()  # rejected again
    d0 = g.disps.reshape(g.n, -1).astype(np.float64)
    d_end = bc.oracle_run(c.name)[1].reshape(g.n, -1)
    assert ((d0 + dz0)[neg] < -10).all()  # negative going into iteration 2
    assert (d_end[neg] == 1e-3).all(), "the applied ones end at the clamp"
    assert np.array_equal(d_end[pos], d0[pos]), "the rejected ones never move"


def test_ragged_plan_reaches_what_it_claims():
    c = bc.case("ragged_plan")
    g, t0, t1 = c.g, c.bk["t0"], c.bk["t1"]
    ii, jj = g.ii, g.jj
    pairs = list(zip(ii.tolist(), jj.tolist()))
    assert g.n == 9 and (t0, t1) == (2, 6)
    assert len(pairs) - len(set(pairs)) == bc.RAGGED_DUPLICATES == 3
    assert (np.diff(ii) < 0).any() and (np.diff(ii) > 0).any(), "not sorted"
    assert ((ii < t0) & (jj >= t0) & (jj < t1)).sum() >= 3, "fixed sources with free targets"
    assert ((ii < t0) & (jj < t0)).sum() >= 2, "both ends fixed"
    u = bc.RAGGED_UNUSED
    assert t0 <= u < t1 and u not in ii and u not in jj
    t = bc.RAGGED_TARGET_ONLY
    assert t >= t1 and t not in ii and (jj == t).sum() >= 2
    assert ((ii >= t1)).sum() >= 2 and {6, 8} <= set(ii.tolist())
    d = _debug(c.name)[0]
    assert d["free_pose"] == [2, 3, 5, 7] and d["fixed_pose"] == [0, 1, 6, 8]
    assert d["free_disp"] == [0, 1, 2, 3, 5, 6, 8] and d["fixed_disp"] == []
    # the target-only pose does move
    assert np.abs(bc.oracle_run(c.name)[0][t] - g.poses[t]).max() > 1e-3


def test_degrees_and_large_plans_reach_what_they_claim():
    deg = np.bincount(bc.case("deg9_17").g.ii, minlength=19)
    assert {7, 9, 17} <= set(deg.tolist()) and all(deg[k] == v for k, v in bc.DEG_WANT.items())
    c = bc.case("m4160")
    assert len(c.g.ii) == 4160 > 4096 and c.g.ht * c.g.wd == 24
    assert (np.bincount(c.g.ii) == 64).all() and len(set(zip(c.g.ii.tolist(), c.g.jj.tolist()))) == 4160
    assert len(np.unique(c.g.ii[4096:])) >= 32, "the second staging chunk holds terms of many source frames"
    assert (np.diff(c.g.ii) < 0).sum() > 1000
    c = bc.case("rig8_n129")
    pi, qi, di, pj, qj = bc.terms(c)
    assert c.g.V == 8 and c.g.n * c.g.V == 1032 > 1024 and len(np.unique(di)) == 1032 and (pi == pj).sum() == 8 * 129
    assert c.bk["optimize_intrinsics"] and c.bk["optimize_rig_rotation"] and c.g.ht * c.g.wd == 24


@pytest.mark.parametrize("name", bc.ALL)
def test_counts_follow_the_oracle_sets(name):
    """what the GPU test asserts info[0], info[1], info[3] against"""
    d = _debug(name)[0]
    n_free, n_fd, n_unknown = bc.counts(name)
    assert n_free == len(d["free_pose"]) and n_fd == len(d["free_disp"]) and n_unknown == len(d["dx"])
    expect = {"behind_pinhole": (4, 5, 24), "zero_support": (5, 6, 30), "ragged_plan": (4, 7, 24), "deg9_17": (18, 19, 108),
              "m4160": (64, 65, 384), "rig8_n129": (128, 1032, 6 * 128 + 8 + 42)}
    if name in expect:
        assert (n_free, n_fd, n_unknown) == expect[name]


# ------------------------------------------------------------------------------------------------ no knife edges


@pytest.mark.parametrize("name", bc.ALL)
def test_no_pixel_sits_on_a_branch(name):
    """In float64, at every iteration: no (term, pixel) within 1e-3 of MIN_DEPTH, no free pixel with dz within 0.1 of the
    rejection threshold - float32 rounding (1e-6 of Z, 1e-5 of dz) cannot move anything across, so the float32 oracle
    and a float32 kernel take the float64 oracle's branch everywhere.  Nothing is excluded."""
    for it, d in enumerate(_debug(name)):
        assert (np.abs(d["Z"] - geom.MIN_DEPTH) < 1e-3).sum() == 0, (name, it)
        assert (np.abs(_dz(d) - 10.0) < 0.1).sum() == 0, (name, it)


def test_float32_oracle_takes_the_same_branches():
    for name in ("behind_pinhole", "behind_mei", "reject_and_clamp"):
        args, kw = bc.oracle_inputs(bc.case(name))
        d32 = ba.bundle_adjustment(*args, dtype=np.float32, return_debug=True, **kw)[4]
        for a, b in zip(d32, _debug(name)):
            assert np.array_equal(a["valid"], b["valid"])
            assert np.array_equal(_dz(a) > 10, _dz(b) > 10)


# ------------------------------------------------------------------------------------------------ the reference


@pytest.mark.parametrize("name", bc.ALL)
def test_oracle_matches_reference_solver(name):
    """float64 oracle vs the reference Solver's outputs, at the tolerance of tests/test_oracle_golden.py (2e-5 relative on
    poses, inverse depth and the rig, 1e-4 on the intrinsics)"""
    G = np.load(os.path.join(GOLD, "ba_edges_reference.npz"))
    c = bc.case(name)
    p, d, k, r = bc.oracle_run(name)
    rp, rd, rk, rr = (G[f"{name}/{x}"] for x in ("poses", "disps", "intrinsics", "rig"))
    assert np.isfinite(rp).all() and np.isfinite(rd).all()
    assert np.abs(p - rp).max() <= 2e-5 * max(1.0, np.abs(rp).max())
    assert np.abs(d.reshape(rd.shape) - rd).max() <= 2e-5 * np.abs(rd).max()
    assert np.abs(k - rk).max() <= 1e-4 * np.abs(rk).max()
    assert np.abs(r - rr).max() <= 2e-5
    assert np.abs(rp - c.g.poses).max() + np.abs(rd - c.g.disps).max() > 1e-3


# ------------------------------------------------------------------------------------------------ sensitivity


def _off_by(name, out):
    """largest distance of a mutated oracle from the float64 oracle, in bounds of the GPU test (outputs with a bound)"""
    ref = bc.oracle_run(name)
    worst = 0.0
    for (key, (_, bound)), a, b in zip(bc.step_bounds(name).items(), out, ref):
        if bound > 0:
            worst = max(worst, float(np.nan_to_num(np.abs(a - b), nan=np.inf).max()) / bound)
    return worst


def _mutants():
    def with_code(name, *mut):
        args, kw = bc.oracle_inputs(bc.case(name))
        return ba.bundle_adjustment(*args, mutate=mut, **kw)

    def with_inputs(name, edit):
        args, kw = bc.oracle_inputs(bc.case(name))
        args = edit(list(args))
        return ba.bundle_adjustment(*args, **kw)

    def drop_last(a):
        a[5], a[6], a[8], a[9] = a[5][:-1], a[6][:-1], a[8][:-1], a[9][:-1]
        return a

    def first_weight_only(a):
        a[6] = np.repeat(a[6][..., :1], 2, axis=-1)
        return a

    yield "no validity mask", "behind_pinhole", lambda n: with_code(n, "no_valid")
    yield "no validity mask", "behind_mei", lambda n: with_code(n, "no_valid")
    yield "|dz| > 10 rejected", "reject_and_clamp", lambda n: with_code(n, "abs_reject")
    yield "no final clamp", "reject_and_clamp", lambda n: with_code(n, "no_clamp")
    for name in ("ragged_plan", "deg9_17", "m4160"):
        yield "last term dropped", name, lambda n: with_inputs(n, drop_last)
    yield "target-only pose >= t1 fixed", "ragged_plan", lambda n: with_code(n, "fix_target_only")
    yield "second weight component ignored", "zero_support", lambda n: with_inputs(n, first_weight_only)


@pytest.mark.parametrize("what,name,run", list(_mutants()), ids=lambda v: v.replace(" ", "_") if isinstance(v, str) else "")
def test_wrong_branches_leave_the_step_tolerance(what, name, run):
    """each mutant, on a case that reaches it, is off by at least 2 bounds of the GPU test on some output"""
    off = _off_by(name, run(name))
    print(what, "on", name, "off by", off, "bounds")
    assert off >= 2.0, (what, name, off)


def test_bounds_are_never_looser_than_the_suite_form():
    for name in bc.ALL:
        o = bc.oracle_run(name)
        b = bc.step_bounds(name)
        assert b["poses"][1] <= 1e-4 * max(1.0, np.abs(o[0]).max()) and b["disps"][1] <= 1e-4 * np.abs(o[1]).max()
        assert b["poses"][1] > 0 and b["disps"][1] > 0
        print(name, {k: "%.3g" % v[0] for k, v in b.items()})
