"""The numpy reference of the BA marginals (tests/ba_marginals_reference.py) against the pinned solver, on the CPU.

The reference rebuilds the linearisation on its own; here its reduced system S and every damped C[k] are tied to the
`debug` output of `oracle.ba.bundle_adjustment` (itself pinned to the reference project's Solver by the golden fixtures),
the Schur-identity variance is tied to the diagonal of a dense inverse of the full Hessian, and every case is shown to
have a pose part that a kernel returning 1/C alone would miss.
"""

import numpy as np
import pytest

import ba_marginals_reference as mr
from oracle import ba as oba


@pytest.mark.parametrize("tag", sorted(mr.CASES))
def test_reference_system_is_the_pinned_solvers(tag):
    args, kw = mr.case_kwargs(tag)
    kw = dict(kw, n_iters=1)
    dbg = oba.bundle_adjustment(*args, dtype=np.float64, return_debug=True, **kw)[-1][0]
    ref = mr.case_marginals(tag)
    assert ref.S.shape == dbg["S"].shape and ref.lin.off == dbg["off"]
    eS = np.abs(ref.S - dbg["S"]).max() if ref.S.size else 0.0
    eC = max(np.abs(ref.lin.C[k] - dbg["C"][k]).max() for k in dbg["C"])
    print(f"{tag}: |S - oracle S| = {eS:.3g}, |C - oracle C| = {eC:.3g}, cond(S) = {np.linalg.cond(ref.S):.4g}")
    assert sorted(ref.lin.C) == sorted(dbg["C"]) == sorted(dbg["free_disp"])
    assert ref.lin.free_pose == dbg["free_pose"]
    assert eS <= 1e-10 and eC <= 1e-10
    assert np.abs(ref.S - ref.S.T).max() <= 1e-10


def test_schur_identity_equals_the_full_inverse_on_ragged_plan():
    ref = mr.case_marginals("ragged_plan")
    lin = ref.lin
    k = 3  # a free source frame of the window with free targets (2, 5) and a fixed one (1); the edge 2 -> 3 is duplicated
    assert k in lin.free_disp
    full = mr.full_inverse_variance(lin, k)
    err = (np.abs(full - ref.disp_var[k]) / full).max()
    print(f"identity vs full inverse: {err:.3g} relative (variances {ref.disp_var[k].min():.3g} .. {ref.disp_var[k].max():.3g})")
    assert err <= 1e-12


@pytest.mark.parametrize("tag", sorted(mr.CASES))
def test_pose_part_is_not_negligible(tag):
    """(var - 1/C) C = e^T S^-1 e / C exceeds 0.05 somewhere: a kernel that returns 1/C alone fails the GPU tolerance"""
    ref = mr.case_marginals(tag)
    pp = np.nanmax(ref.pose_part)
    print(f"{tag}: largest pose part {pp:.3g}")
    assert pp > 0.05
    assert np.nanmin(ref.pose_part) >= 0.0 and np.nanmin(ref.disp_var) > 0.0


@pytest.mark.parametrize("tag", sorted(mr.CASES))
def test_unfree_rows_stay_nan_and_bounds_come_from_delta32(tag):
    ref = mr.case_marginals(tag)
    Nbuf, V, P = ref.lin.shape
    free_d = np.zeros(Nbuf * V, bool)
    free_d[ref.lin.free_disp] = True
    assert np.isfinite(ref.disp_var[free_d]).all() and np.isnan(ref.disp_var[~free_d]).all()
    free_p = np.zeros(Nbuf, bool)
    free_p[ref.lin.free_pose] = True
    assert np.isfinite(ref.pose_cov[free_p]).all() and np.isnan(ref.pose_cov[~free_p]).all()
    (dv, bv), (dc, bc_) = mr.bounds(tag)
    print(f"{tag}: delta32 disp_var {dv:.3g} (bound {bv:.3g}), pose_cov {dc:.3g} (bound {bc_:.3g})")
    assert 0 < bv <= 1e-4 and 0 < bc_ <= 1e-4
