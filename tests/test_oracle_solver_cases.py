"""The solver cases of oracle/solver_cases.py, proved on the CPU: each lands on the route and the boundary it names
according to oracle/ba_route.py (the restatement of vipe_amd/csrc/ba_route.cuh), the plan's facts agree with the oracle's
own sets and with the block band of its float64 reduced system, the step is what the tolerance measures, and a solver
with one tile, one panel or one band block wrong leaves the tolerance that tests/test_gpu_ba_solvers.py holds the
kernels to.  Run with -s for the route table, the per-case delta32 / step / bounds and the defect ratios.
"""

import numpy as np
import pytest

from oracle import ba_cases as bc
from oracle import ba_route as br
from oracle import solver_cases as sc

# ------------------------------------------------------------------------------------------------ the route by hand


def test_route_constants_and_known_systems():
    """figures that can be checked against ba_route.cuh with a pencil"""
    assert br.SOLVER_LDS_DOUBLES == 20224 and br.band_pair_cap(2) == 917 and br.band_pair_cap(br.BAND_UPT) == 2709
    assert br.band_npair(24, 1) == 300 + 24 and br.band_npair(66, 3) == 2211 + 198 + 5
    # PB = 42 with the focal length: 903 + 84 + 2 = 989 > 917 pairs, one band column: wide by the pair count alone
    assert br.band_form(49, 8, 7, 1, 0) == "wide" and br.band_form(48, 8, 7, 0, 0) == "wide"
    # 26 free poses, every pair coupled: PB = 150, the band solver declines (WBP > 128), n + 1 = 157 rows fit the dense one
    assert br.band_form(156, 26, 25, 0, 0) == "declines" and br.dense_takes(156, 26, 25, 0, 0) and br.dense_tile_rows(156) == 10
    assert not br.dense_takes(162, 27, 26, 0, 0) and br.global_form(162, 27, 26, 0, 0) == "one_workgroup"  # 11 tile rows: 66 tiles
    # a rig goes to the global-memory solvers whatever its band
    assert br.band_form(32, 4, 2, 8, 1) == "declines" and br.solver(32, 4, 2, 8, 1) == br.SOLVER_GLOBAL
    assert br.global_form(256, 42, 41, 4, 1) == "one_workgroup" and br.global_form(257, 42, 41, 5, 1) == "tiled"
    assert br.solver(0, 0, 0, 0, 0) is None and br.global_form(0, 0, 0, 0, 0) == "declines"
    # three tail unknowns: neither LDS solver
    assert br.solver(6 * 8 + 3, 8, 2, 3, 0) == br.SOLVER_GLOBAL


def test_band_boundaries_are_where_the_lds_carves_put_them():
    """radius 3 (bandblk 6, WBP 43): two images of 6 (nb - (nb - 6) // 2) rows fit up to 68 free poses, one image up to 74"""
    b = sc.band_boundaries(3)
    assert b == dict(two_min=28, two_max=68, one_max=74), b
    rows = br.band2_rows_max(68, 6)
    assert rows == 6 * 37 and 2 * br.band2_image(rows, 43) + 8 <= br.SOLVER_LDS_DOUBLES < 2 * br.band2_image(br.band2_rows_max(69, 6), 43) + 8
    assert br.band_need(444, 444, 1, 43) <= br.SOLVER_LDS_DOUBLES < br.band_need(450, 450, 1, 43)
    b = sc.band_boundaries(1)
    assert b["two_min"] == 12 and b["two_max"] < b["one_max"]


# ------------------------------------------------------------------------------------------------ every case on its route

EXPECT = {  # name -> (n_free, n, bandblk), written down by hand, not computed (None: whatever the random long-range edges give)
    "wg168": (28, 168, 27), "wg252": (42, 252, 41), "wg253": (42, 253, 41), "wg234_band": (39, 234, 16), "wg254_rig": (41, 254, 4),
    "wg256_rig4": (42, 256, 2),
    "wg240_in_big_ws": (40, 240, None), "ct258": (43, 258, 42), "ct319": (53, 319, 52), "ct320_rig": (53, 320, 2),
    "ct385": (64, 385, 63), "ct360_in_big_ws": (60, 360, None), "ct_band": (75, 450, 6), "band_r3_two_min": (28, 168, 6),
    "band_r3_below_two": (27, 162, 6), "band_r3_two_max": (68, 408, 6), "band_r3_above_two": (69, 414, 6),
    "band_r3_one_max": (74, 444, 6), "band_r1_two_min": (12, 72, 2), "band_r1_below_two": (11, 66, 2), "wg175": (29, 175, None),
    "ct414": (69, 414, None), "ct414_f": (69, 415, None), "dense114": (19, 114, 18), "window28": (27, 162, 26),
}


def test_route_table():
    print()
    for name in sc.ALL:
        c = sc.case(name)
        n_free, n, bandblk, ntail, degree = sc.facts(name)
        print(f"{name:24s} n_free {n_free:3d} n {n:3d} band {bandblk:3d} tail {ntail} degree {degree:3d}  "
              f"{sc.route(name):13s} one-chain option: {sc.route(name, False):13s} {c.boundary}")


@pytest.mark.parametrize("name", sc.ALL)
def test_case_lands_on_its_route(name):
    c = sc.case(name)
    n_free, n, bandblk, ntail, _ = sc.facts(name)
    assert sc.route(name) == c.route, (name, sc.route(name), c.route)
    assert sc.TILE[c.route] == c.tile
    if name in EXPECT:
        e = EXPECT[name]
        assert (n_free, n) == e[:2] and (e[2] is None or bandblk == e[2]), (name, n_free, n, bandblk)
    args = sc.route_args(name)
    want = {"tiled": br.SOLVER_GLOBAL, "one_workgroup": br.SOLVER_GLOBAL, "dense": br.SOLVER_DENSE}.get(c.route, br.SOLVER_BAND)
    assert br.solver(*args) == want
    assert br.global_form(*args) == (c.route if want == br.SOLVER_GLOBAL else "declines")
    # under BA_OPT_ONE_CHAIN a two-chain system is a narrow one; everything else stays
    assert sc.route(name, band2=False) == ("narrow" if c.route == "two_chain" else c.route)


def test_single_workgroup_and_tiled_cases_sit_on_their_block_boundaries():
    n = {name: sc.facts(name)[1] for name in sc.ALL}
    assert n["wg168"] % br.NB == 0 and n["wg252"] % br.NB == 0 and n["wg253"] % br.NB == 1
    assert n["wg252"] == 6 * ((br.CT_MIN_N) // 6) and n["wg253"] == n["wg252"] + 1  # the largest sizes without / with one tail
    assert n["wg254_rig"] <= br.CT_MIN_N < n["wg254_rig"] + 6  # one more keyframe leaves the kernel
    assert n["wg256_rig4"] == br.CT_MIN_N and n["wg256_rig4"] % br.NB == 4  # the last size of the kernel: one unknown more is tiled
    assert n["ct258"] == 6 * (br.CT_MIN_N // 6 + 1) > br.CT_MIN_N  # the first pose-only size beyond it
    assert n["ct319"] % br.CT == br.CT - 1 and n["ct385"] % br.CT == 1 and n["ct320_rig"] % br.CT == 0
    assert sc.facts("ct320_rig")[3] == 2 and sc.facts("wg254_rig")[3] == 8 and sc.facts("wg256_rig4")[3] == 4
    # the band is narrow against the matrix where the case says so: panels of band rows (+ tail rows), not all rows
    for name in ("wg234_band", "wg254_rig", "wg256_rig4", "ct320_rig", "ct_band"):
        n_free, _, bandblk, _, _ = sc.facts(name)
        assert 2 * bandblk < n_free, name
    # why wg234_band is nobody else's: the band solver declines by pair count and LDS, the dense solver by size
    n_, nf, b, _, _, _ = sc.route_args("wg234_band")
    assert br.band_npair(6 * b, 1) > br.band_pair_cap(br.BAND_UPT) and br.band_need(n_, 6 * nf, 1, 6 * b + 7) > br.SOLVER_LDS_DOUBLES
    assert br.dense_need(n_) > br.SOLVER_LDS_DOUBLES
    # workspaces sized for more than the system: the library sizes S for 6 poses-in-the-buffer + 2 unknowns
    for name, tiles in (("wg240_in_big_ws", None), ("ct360_in_big_ws", 7)):
        c = sc.case(name)
        nmax = 6 * c.g.n + 2
        assert nmax > br.CT_MIN_N and nmax > n[name] + 6 * 9
        if tiles:
            assert -(-nmax // br.CT) >= tiles > -(-n[name] // br.CT)


@pytest.mark.parametrize("a,b", sc.BAND_PAIRS)
def test_band_boundary_neighbours_take_the_other_form(a, b):
    fa, fb = sc.facts(a), sc.facts(b)
    assert fb[0] == fa[0] + 1 and fa[2] == fb[2] and fa[3] == fb[3] == 0, "one free pose apart, same band"
    assert sc.route(a) != sc.route(b) and sc.route(a) == sc.case(a).route and sc.route(b) == sc.case(b).route


# ------------------------------------------------------------------------------------------------ the plan's facts


@pytest.mark.parametrize("name", sc.ALL)
def test_plan_facts_agree_with_the_oracle(name):
    """free poses and unknowns against the oracle's sets (`ba_cases.case_counts`), the band against the nonzero 6 x 6 blocks
    of the float64 reduced system of the first iteration"""
    c = sc.case(name)
    n_free, n, bandblk, ntail, degree = sc.facts(name)
    assert (n_free, n) == (bc.case_counts(c)[0], bc.case_counts(c)[2])
    w = sc.oracle_system(name)
    assert len(w.dx) == c.bk["n_iters"] and all(len(dx) == n for dx in w.dx)
    assert w.symmetric and w.band == bandblk, (name, w.band, bandblk)
    V = c.g.V if c.rig else 1
    assert degree == np.bincount(np.repeat(c.g.ii, V) * V + np.tile(np.arange(V), len(c.g.ii))).max()


@pytest.mark.parametrize("name", bc.ALL)
def test_plan_facts_on_the_ragged_cases(name):
    """the same rule on plans with fixed sources, target-only poses, unused poses and a rig (oracle/ba_cases.py)"""
    c = bc.case(name)
    f = br.plan_facts(c.g.ii, c.g.jj, c.bk["t0"], c.bk["t1"], c.g.V if c.rig else 1, c.bk.get("optimize_intrinsics", False),
                      c.intr.shape[1] - 4, c.bk.get("optimize_rig_rotation", False))
    assert (f[0], f[1]) == (bc.counts(name)[0], bc.counts(name)[2])
    if name == "ragged_plan":  # free poses 2, 3, 5, 7 in slots 0..3; frame 5 reaches 3 and 7, frame 1 (fixed) reaches 2 and 3
        assert f[2] == 2


# ------------------------------------------------------------------------------------------------ the tolerance


def test_bounds_table():
    print()
    for name in sc.ALL:
        b = sc.step_bounds(name)
        print(f"{name:24s} step {sc.pose_step(name):.2e}  " + "  ".join(f"{k} {d32:.2e} / {bound:.2e}" for k, (d32, bound) in b.items())
              + f"  1e-4 form / bound (poses) {sc.old_pose_bound(name) / b['poses'][1]:.1f}")


@pytest.mark.parametrize("name", sc.ALL)
def test_bound_is_about_the_step(name):
    """8 delta32 on the poses is below the 1e-4 form (the known exception: wg175, where the old form binds), no bound is
    looser than that form, and the step is at least 100 pose bounds"""
    o = sc.oracle_run(name)
    b = sc.step_bounds(name)
    old = (sc.old_pose_bound(name), 1e-4 * np.abs(o[1]).max(), 1e-4 * np.abs(o[2]).max(), 1e-4)
    for (key, (d32, bound)), lim in zip(b.items(), old):
        assert 0 < bound <= lim, (name, key)
    if name in sc.OLD_FORM_BINDS:
        assert 8 * b["poses"][0] >= old[0]
    else:
        assert 8 * b["poses"][0] < old[0], (name, b["poses"][0], old[0])
    assert sc.pose_step(name) >= 100 * b["poses"][1], (name, sc.pose_step(name), b["poses"][1])


def test_float64_cholesky_emulation_is_a_solver():
    """`_chol_solve` without a defect solves: it is the tiled factorisation with the rhs riding along, nothing else"""
    rng = np.random.default_rng(7)
    for n, tile in ((130, 64), (128, 64), (65, 64), (37, 16), (30, 6)):
        A = rng.normal(size=(n, n))
        S, g = A @ A.T + n * np.eye(n), rng.normal(size=n)
        x, left = sc._chol_solve(S, g, tile)
        assert left == 0 and np.abs(x - np.linalg.solve(S, g)).max() < 1e-12


# (case, defect) pairs that touch the system and still stay within 10 bounds, with the ratio seen: listed, not dropped
# update_entry damages ONE entry of the last row: where that row is an ordinary pose row far from the gauge, its step and
# the disparities behind it move by a few bounds only.  tail_as_pose on the rig: the last unknown is a rig rotation, whose
# diagonal (every term of the second view) dwarfs the poses' ep = 0.1.  backsub_tile on ct385: the last tile row is the
# focal length alone.  Every one of these cases is told apart by its other defects (>= 43 bounds).
BELOW_TEN = {("wg234_band", "update_entry"): 8.06, ("wg254_rig", "update_entry"): 6.31, ("wg254_rig", "tail_as_pose"): 0.446,
             ("wg240_in_big_ws", "update_entry"): 2.65, ("ct385", "backsub_tile"): 4.74, ("ct360_in_big_ws", "update_entry"): 0.517,
             ("window17", "update_entry"): 0.502, ("window24", "update_entry"): 1.04}


@pytest.mark.parametrize("name", sc.ALL)
def test_wrong_solvers_leave_the_bound(name):
    """every defect that touches the case's system is off by >= 10 bounds on some output"""
    offs = {}
    for what, solve in sc.case_defects(name).items():
        out = sc.run_with(name, solve)
        if solve.left == 0:
            print(f"{name:24s} {what:13s} touches nothing here (a zero tile of the factor)")
            n_free, _, bandblk, ntail, _ = sc.facts(name)  # a banded system without tail rows: that tile lies outside the band
            assert what == "backsub_tile" and bandblk < n_free - 1 and ntail == 0, (name, what)
            continue
        offs[what] = sc.off_by(name, out)
        print(f"{name:24s} {what:13s} off by {offs[what]:9.3g} bounds; the 1e-4 asserts would "
              f"{'' if sc.old_asserts_catch(name, out) else 'NOT '}have caught it")
    assert {"update_entry", "rhs_panel"} <= set(offs)
    low = {what for what, off in offs.items() if off < 10}
    assert low == {what for (case, what) in BELOW_TEN if case == name}, (name, {what: offs[what] for what in low})
