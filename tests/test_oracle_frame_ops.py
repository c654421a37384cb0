"""The inputs that tests/test_gpu_geom_scatter.py feeds the slam_ext geometry kernels, checked with the oracle alone:
every decision the kernels take on them (the 0.75 valid share, the depth-filter threshold, the 0.01 / 0.25 depth
branches) is either far from its boundary or covered by an exception whose share of the pixels is capped - so that a
failure on the GPU means a wrong kernel, not an unlucky input.  Also pins the `dtype` argument of oracle/frame_ops.py:
float32 by default with the values it has always had, float64 on request.
"""

import os

import numpy as np
import pytest

from oracle import frame_cases as fc
from oracle import frame_ops

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAP = 0.005  # the share of pixels a comparison may leave out


def _fd(c, **kw):
    return frame_ops.frame_distance(c.fd_poses, c.disps, c.intr2, fc.FD_PI, fc.FD_PJ, fc.FD_QI, fc.FD_QJ, fc.FD_DI, fc.BETA, **kw)


def test_default_dtype_keeps_its_values():
    """the float32 default returns, bit for bit, what the functions returned before they took a `dtype`
    (tests/golden/frame_ops_default.npz was written by that version on the (9, 29) case)"""
    c = fc.geom_case(9, 29)
    want = np.load(os.path.join(GOLD, "frame_ops_default.npz"))
    coords, valid = frame_ops.projmap(c.pm_poses, c.disps, c.intr, fc.PM_II, fc.PM_JJ)
    got = {"frame_distance": _fd(c), "depth_filter": frame_ops.depth_filter(c.g.poses, c.disps, c.intr, fc.DF_INDS, c.df_thresh),
           "coords": coords, "valid": valid, "iproj": frame_ops.iproj(c.g.poses, c.disps, c.intr)}
    for k, v in got.items():
        assert v.dtype == np.float32 and np.array_equal(v, want[k]), k
    assert np.array_equal(_fd(c, dtype=np.float32), got["frame_distance"])


def test_float64_runs_in_float64_and_agrees_with_float32():
    c = fc.geom_case(9, 29)
    d32, d64 = _fd(c), _fd(c, dtype=np.float64)
    assert d64.dtype == np.float64 and np.abs(d32 - d64).max() <= 1e-5 * np.abs(d64).min()
    p32, p64 = (frame_ops.iproj(c.g.poses, c.disps, c.intr, dtype=t) for t in (np.float32, np.float64))
    assert p64.dtype == np.float64 and 0 < np.abs(p32 - p64).max() < 1e-5
    c64, v64 = frame_ops.projmap(c.pm_poses, c.disps, c.intr, fc.PM_II, fc.PM_JJ, dtype=np.float64)
    assert c64.dtype == np.float64 and v64.dtype == np.float32
    assert frame_ops.depth_filter(c.g.poses, c.disps, c.intr, fc.DF_INDS, c.df_thresh, dtype=np.float64).dtype == np.float32


def test_index_arrays_do_not_alias():
    arrays = [fc.FD_PI, fc.FD_PJ, fc.FD_DI]
    assert all(not np.array_equal(a, b) for i, a in enumerate(arrays) for b in arrays[i + 1:])
    assert all(set(q.tolist()) == {0, 1} for q in (fc.FD_QI, fc.FD_QJ, fc.RIG_QI, fc.RIG_QJ))
    assert not np.array_equal(fc.FD_QI, fc.FD_QJ) and not np.array_equal(fc.RIG_QI, fc.RIG_QJ)
    assert len(fc.DF_INDS) != fc.N and {0, fc.N - 1} <= set(fc.DF_INDS.tolist())
    assert not np.array_equal(fc.DF_INDS, np.sort(fc.DF_INDS)) and len(set(fc.DF_SCALE.tolist())) == len(fc.DF_INDS)
    c = fc.geom_case(5, 7)
    assert np.allclose(c.intr2[1], 1.03 * c.intr2[0], rtol=1e-6) and c.g.ht == 5 and c.g.wd == 7 and c.disps.shape[0] == fc.N


@pytest.mark.parametrize("grid", fc.GRIDS)
def test_frame_distance_valid_shares_stay_clear_of_the_threshold(grid):
    c = fc.geom_case(*grid)
    d, share = _fd(c, dtype=np.float64, with_share=True)
    assert np.all(np.abs(share - 0.75) > 0.01), share
    assert d[fc.FD_FAR] == 1000.0 and share[fc.FD_FAR] < 0.75
    assert 0.75 < share[fc.FD_PARTIAL] < 1.0  # some pixels masked, the pair still scored
    ok = np.arange(len(d)) != fc.FD_FAR
    assert np.all(d[ok] < 1000.0) and np.all(d[ok] > 0.1)  # no reference value near 0 for the relative tolerance
    _, share32 = _fd(c, with_share=True)
    assert np.array_equal(share32 < 0.75, share < 0.75)


@pytest.mark.parametrize("bidirectional", [False, True])
def test_rig_valid_shares_stay_clear_of_the_threshold(bidirectional):
    d, share = fc.rig_reference(fc.rig_case(41, 73), bidirectional)
    assert share.shape == (1 + bidirectional, len(fc.RIG_PI))
    assert np.all(np.abs(share - 0.75) > 0.01) and np.all(d < 1000.0) and np.all(d > 0.1)


@pytest.mark.parametrize("grid", fc.GRIDS)
def test_depth_filter_inputs(grid):
    c = fc.geom_case(*grid)
    args = (c.g.poses, c.disps, c.intr, fc.DF_INDS, c.df_thresh)
    cnt32 = frame_ops.depth_filter(*args)
    cnt64, margin = frame_ops.depth_filter(*args, dtype=np.float64, with_margin=True)
    left_out = margin < 1e-4 * c.df_thresh[:, None, None]
    assert left_out.mean() <= CAP
    assert (cnt32 != cnt64).mean() <= CAP  # float32 and float64 already agree within the cap
    assert cnt32.max() >= 3 and cnt32.min() == 0
    assert len(set(c.df_thresh.tolist())) == len(fc.DF_INDS)


@pytest.mark.parametrize("grid", fc.GRIDS)
def test_projmap_inputs_reach_both_depth_branches(grid):
    c = fc.geom_case(*grid)
    _, valid, depth = frame_ops.projmap(c.pm_poses, c.disps, c.intr, fc.PM_II, fc.PM_JJ, dtype=np.float64, with_depth=True)
    assert (depth < 0.01).any() and ((depth > 0.01) & (depth < 0.25)).any() and (depth > 0.25).any()
    assert (np.abs(depth - 0.25) < 1e-5).mean() <= CAP and (np.abs(depth - 0.01) < 1e-5).mean() <= CAP
    assert 0 < valid.mean() < 1
