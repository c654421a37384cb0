"""`vipe_convex_upsample` (convex_upsample.hip) through the ctypes ABI and through `droid_net_ext.cvx_upsample`, against
the float64 reference of tests/cvx_reference.py with the bound derived there (C_BOUND * 2^-23 * max |data| over the 3 x 3
neighbourhood - from the kernel's operation count, never from what it returns).  Every output buffer is prefilled with
a sentinel; each test prints its largest error as a fraction of the bound."""
import numpy as np
import pytest
import torch

import cvx_reference as cr

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, -1, -3
F16, F32 = 0, 1


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def abi_call(data, mask, rows=None, out=None, shape=None):
    """the raw entry point -> (return code, out tensor); `shape` = (N, R, h, w, C) overrides what the tensors say"""
    from vipe_amd._lib import lib, ptr, stream_ptr
    R, h, w, C = data.shape
    N = mask.shape[0]
    if out is None:
        out = torch.full((R, 8 * h, 8 * w, C), cr.SENTINEL, dtype=torch.float32, device=dev())
    N, R, h, w, C = shape or (N, R, h, w, C)
    code = lib().vipe_convex_upsample(ptr(mask), F16 if mask.dtype == torch.float16 else F32, ptr(data), ptr(out),
                                      ptr(rows), N, R, h, w, C, stream_ptr(data))
    torch.cuda.synchronize()
    return code, out


def within_bound(got, data, mask, rows=None, what=""):
    ref = cr.cvx_upsample_ref(data, mask, rows)
    bound = cr.cvx_bound(data, rows)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print(f"{what}: max |err| / bound = {ratio:.3f} (max |err| = {err.max():.3e})")
    assert np.isfinite(got).all()
    assert (err <= bound).all(), f"{what}: {ratio:.3f} x the bound"
    return ratio


def both_routes(data, mask, what):
    """ABI and wrapper on the same inputs: each within the bound, and bit-equal to one another"""
    from vipe_amd.ext import droid_net_ext
    d, m = T(data), T(mask)
    code, out = abi_call(d, m)
    assert code == OK
    got = out.cpu().numpy()
    within_bound(got, data, mask, what=what)
    got2 = droid_net_ext.cvx_upsample(d, m).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), got2.view(np.uint32)), f"{what}: wrapper differs from the ABI call"


@pytest.mark.parametrize("shape", cr.RAGGED_SHAPES)
@pytest.mark.parametrize("mask_dtype", [np.float16, np.float32])
def test_ragged_shapes(shape, mask_dtype):
    data, mask = cr.make_inputs(*shape, mask_dtype=mask_dtype)
    both_routes(data, mask, f"{shape} {np.dtype(mask_dtype).name}")


def test_more_than_one_workgroup_in_each_dimension():
    data, mask = cr.make_inputs(*cr.MULTI_WORKGROUP_SHAPE)
    both_routes(data, mask, f"{cr.MULTI_WORKGROUP_SHAPE}")


@pytest.mark.parametrize("mask_dtype", [np.float16, np.float32])
def test_one_hot_masks_select_the_neighbour_bit_for_bit(mask_dtype):
    data, mask, taps = cr.make_one_hot(*cr.ONE_HOT_SHAPE, mask_dtype=mask_dtype)
    want = cr.one_hot_expected(data, taps)
    code, out = abi_call(T(data), T(mask))
    assert code == OK
    got = out.cpu().numpy()
    assert (want == 0.0).any()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("lo,hi", [(80.0, 100.0), (-100.0, -80.0)])
def test_large_logits(lo, hi):
    data, mask = cr.make_large_logits(2, 3, 9, 2, lo, hi)
    code, out = abi_call(T(data), T(mask))
    assert code == OK
    within_bound(out.cpu().numpy(), data, mask, what=f"logits in [{lo}, {hi}]")


def test_rows_write_only_the_named_rows():
    from vipe_amd.ext import droid_net_ext
    c = cr.ROWS_CASE
    data, mask = cr.make_inputs(c["N"], c["h"], c["w"], c["C"], R=c["R"])
    rows = T(np.asarray(c["rows"], dtype=np.int64))
    for route in ("abi", "wrapper"):
        out = torch.full((c["R"], 8 * c["h"], 8 * c["w"], c["C"]), cr.SENTINEL, dtype=torch.float32, device=dev())
        if route == "abi":
            code, _ = abi_call(T(data), T(mask), rows=rows, out=out)
            assert code == OK
        else:
            assert droid_net_ext.cvx_upsample(T(data), T(mask), rows=rows, out=out) is out
        got = out.cpu().numpy()
        within_bound(got[c["rows"]], data, mask, rows=c["rows"], what=f"rows {c['rows']} ({route})")
        others = [r for r in range(c["R"]) if r not in c["rows"]]
        assert len(others) == 4
        sentinel = np.full_like(got[others], cr.SENTINEL)
        assert np.array_equal(got[others].view(np.uint32), sentinel.view(np.uint32))


def test_return_codes():
    data, mask = cr.make_inputs(2, 3, 9, 1)
    d, m = T(data), T(mask)
    untouched = np.full((2, 24, 72, 1), cr.SENTINEL, dtype=np.float32)
    # C = 5: unsupported, nothing launched
    d5 = torch.zeros((2, 3, 9, 5), dtype=torch.float32, device=dev())
    code, out = abi_call(d5, m)
    assert code == EUNSUPPORTED and (out == cr.SENTINEL).all()
    # N = 0: fine, nothing launched
    code, out = abi_call(d, m, shape=(0, 2, 3, 9, 1))
    assert code == OK and np.array_equal(out.cpu().numpy().view(np.uint32), untouched.view(np.uint32))
    # null pointers / bad shapes
    from vipe_amd._lib import lib, ptr, stream_ptr
    L, s = lib(), stream_ptr(d)
    out = T(untouched)
    assert L.vipe_convex_upsample(None, F16, ptr(d), ptr(out), None, 2, 2, 3, 9, 1, s) == EINVAL
    assert L.vipe_convex_upsample(ptr(m), F16, None, ptr(out), None, 2, 2, 3, 9, 1, s) == EINVAL
    assert L.vipe_convex_upsample(ptr(m), F16, ptr(d), None, None, 2, 2, 3, 9, 1, s) == EINVAL
    assert L.vipe_convex_upsample(ptr(m), F16, ptr(d), ptr(out), None, 2, 2, 0, 9, 1, s) == EINVAL
    assert L.vipe_convex_upsample(ptr(m), F16, ptr(d), ptr(out), None, 2, 1, 3, 9, 1, s) == EINVAL  # N > R without rows
    assert L.vipe_convex_upsample(ptr(m), 2, ptr(d), ptr(out), None, 2, 2, 3, 9, 1, s) == EINVAL    # f64 masks
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), untouched.view(np.uint32))
    from vipe_amd.ext import droid_net_ext
    with pytest.raises(NotImplementedError):
        droid_net_ext.cvx_upsample(d5, m)


def test_nchw_mask_layout_is_bit_equal():
    from vipe_amd.ext import droid_net_ext
    data, mask = cr.make_inputs(2, 3, 9, 2)
    d, m = T(data), T(mask)
    a = droid_net_ext.cvx_upsample(d, m)
    nchw = m.permute(0, 3, 1, 2).contiguous()
    b = droid_net_ext.cvx_upsample(d, nchw, mask_layout="nchw")
    c = droid_net_ext.cvx_upsample(d, nchw[None], mask_layout="nchw")  # [1,N,576,h,w], as UpdateEngine.forward returns it
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    within_bound(a.cpu().numpy(), data, mask, what="nchw")


def test_cpu_tensors_raise():
    from vipe_amd.ext import droid_net_ext
    data, mask = cr.make_inputs(1, 2, 3, 1)
    with pytest.raises(NotImplementedError):
        droid_net_ext.cvx_upsample(torch.from_numpy(data), torch.from_numpy(mask))
