"""The float64 oracle of `vipe_convex_upsample` (tests/cvx_reference.py, written from the formula with explicit tap and
sub-pixel indexing) against DROID-SLAM's torch composition - softmax over `mask.view(N,1,9,8,8,h,w)`, `F.unfold`, sum,
permute - in float64, on the seeded inputs the GPU test uses.  No GPU."""
import numpy as np
import pytest
import torch

import cvx_reference as cr


def _composition(data, mask):
    return cr.torch_composition(torch.from_numpy(data).double(), torch.from_numpy(mask.astype(np.float64))).numpy()


@pytest.mark.parametrize("shape", cr.RAGGED_SHAPES + [cr.MULTI_WORKGROUP_SHAPE])
@pytest.mark.parametrize("mask_dtype", [np.float16, np.float32])
def test_reference_equals_unfold_composition(shape, mask_dtype):
    data, mask = cr.make_inputs(*shape, mask_dtype=mask_dtype)
    ref = cr.cvx_upsample_ref(data, mask)
    assert ref.shape == (shape[0], 8 * shape[1], 8 * shape[2], shape[3])
    assert np.abs(ref - _composition(data, mask)).max() <= 1e-12


@pytest.mark.parametrize("lo,hi", [(80.0, 100.0), (-100.0, -80.0)])
def test_reference_large_logits(lo, hi):
    data, mask = cr.make_large_logits(2, 3, 9, 2, lo, hi)
    ref = cr.cvx_upsample_ref(data, mask)
    assert np.isfinite(ref).all() and np.abs(ref - _composition(data, mask)).max() <= 1e-12


def test_reference_one_hot_selects_the_neighbour():
    """the one-hot generator and its expectation agree with the reference: pins k = ky*3 + kx, dy*8 + dx and the padding"""
    data, mask, taps = cr.make_one_hot(*cr.ONE_HOT_SHAPE)
    want = cr.one_hot_expected(data, taps)
    assert (want == 0.0).any()  # some taps fall outside the grid
    assert np.array_equal(cr.cvx_upsample_ref(data, mask), want.astype(np.float64))
    assert np.abs(_composition(data, mask) - want).max() <= 1e-12


def test_reference_rows_and_envelope():
    c = cr.ROWS_CASE
    data, mask = cr.make_inputs(c["N"], c["h"], c["w"], c["C"], R=c["R"])
    ref = cr.cvx_upsample_ref(data, mask, rows=c["rows"])
    assert np.array_equal(ref, cr.cvx_upsample_ref(data[c["rows"]], mask))
    lo, hi = cr.neighbourhood_minmax(data, rows=c["rows"])
    assert (ref >= lo - 1e-12).all() and (ref <= hi + 1e-12).all()  # a convex combination
    assert cr.cvx_bound(data, rows=c["rows"]).shape == ref.shape
