"""The reduced-system solvers of the dense BA at their route and tile boundaries: the LDS band solver (narrow, wide,
two-chain), the LDS dense solver, the single-workgroup global-memory Cholesky and the 64 x 64 tiled one.

Cases: oracle/solver_cases.py (tests/test_oracle_solver_cases.py proves on the CPU that each one sits on the boundary it
names and that a solver with one tile, panel or band block wrong leaves the tolerance used here).  Which solver should
take a case is decided on the CPU by oracle/ba_route.py; the device must report the same plan facts and the same solver.
Tolerance, relative to the STEP: per output min(8 x delta32, the suite's 1e-4 form), not below 8 float32 units in the
last place; delta32 = the distance between the oracle in float32 and in float64 on the case (`solver_cases.step_bounds`).
Every call works in buffers with two frames beyond the graph, so a workspace is always sized for 12 unknowns more than
the system has.
"""

import pytest

from ba_device import case_tensors, check_outputs, option_sets, run_case
from oracle import ba_route as br
from oracle import solver_cases as sc
from test_gpu_parity import band_solver_form

pytestmark = pytest.mark.gpu


def _check(name, tag, got):
    """the plan's facts and the solver against the CPU route, the outputs against the float64 oracle"""
    c = sc.case(name)
    info = got[4]
    band2 = tag == "default"  # the general selection carries BA_OPT_ONE_CHAIN
    n_free, n, bandblk, ntail, degree = sc.facts(name)
    print(f"{name} [{tag}] info {info.tolist()}, route {sc.route(name, band2)}")
    assert info[2] == 0, "Cholesky must not fail"
    assert (info[0], info[3], info[4], info[6]) == (n_free, n, bandblk, degree), info
    assert info[5] == br.solver(*sc.route_args(name, band2)), info
    want = sc.route(name, band2)
    assert want == (c.route if band2 or c.route != "two_chain" else "narrow")
    if info[5] == br.SOLVER_BAND:
        assert band_solver_form(info, two_chain=band2) == want
    check_outputs(name, tag, got, sc.oracle_run(name), sc.step_bounds(name))
    if not c.bk.get("optimize_intrinsics"):
        assert (got[2] == c.intr).all()


@pytest.mark.parametrize("tag", ["default", "general"])
@pytest.mark.parametrize("name", sc.ALL)
def test_solver_case_within_the_step_tolerance(name, tag):
    """every case under the default kernel selection (two-chain band solve, fused matrix-core accumulate where the degree
    allows) and under BA_OPT_ONE_CHAIN | BA_OPT_GENERAL_ACCUMULATE: a two-chain system is then a narrow one, every other
    system keeps its solver"""
    _check(name, tag, run_case(sc.case(name), option_sets()[tag]))


@pytest.mark.parametrize("name", sc.REUSE)
def test_solver_case_with_a_reused_plan(name):
    """One case per route, twice from the same start with the caller's plan state: the first call builds the plan and
    launches every solver, the second reuses the plan and launches what the first one learnt (`path_hint`).  Same solver,
    same bound."""
    from vipe_amd.ext import slam_ext
    c = sc.case(name)
    tensors, state = case_tensors(c), {}
    first = run_case(c, 0, tensors, state=state, plan_key=("solver case", name))
    _check(name, "first call", first)
    second = run_case(c, 0, tensors, state=state, plan_key=("solver case", name))
    hint = slam_ext._path_hint(state, state.get("key"))
    print(name, "hint", hint)
    solved = {br.SOLVER_BAND: 4 | 16, br.SOLVER_DENSE: 4 | 8, br.SOLVER_GLOBAL: 8 | 16}[int(first[4][5])]
    assert hint != 0 and hint & solved == solved, (hint, solved)
    assert second[4][5] == first[4][5]
    _check(name, "reused plan", second)
