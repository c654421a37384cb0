"""`vipe_depth_export` (depth_export.hip) through `vipe_amd.slam.ingest.depth_export`, the single route to the kernel,
against the float64 reference and the derived per-pixel bound of tests/depth_export_reference.py.  Disparities are
1 / U(1, 5) with fixed seeds on (24, 40) maps - the smallest that still span more than one 64 x 4 tile in both directions
after export."""
import numpy as np
import pytest
import torch

import depth_export_reference as dr

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def export(disp, params, rows=None, out=None, dtype=torch.float32, depth_scale=1.0):
    from vipe_amd.slam.ingest import depth_export
    r = None if rows is None else torch.tensor(rows, dtype=torch.int64, device=dev())
    got = depth_export(torch.from_numpy(disp).to(dev()), params, rows=r, out=out, dtype=dtype, depth_scale=depth_scale)
    torch.cuda.synchronize()
    return got


def check(got, disp, params, what, **kw):
    ref, bound = dr.depth_export_ref(disp, params, **kw), dr.depth_bound(disp, params, **kw)
    assert tuple(got.shape) == ref.shape and np.isfinite(bound).all()
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    print(f"{what}: max err / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), what


def test_upsampling_with_a_crop():
    disp = dr.make_disps(3, seed=11)
    got = export(disp, dr.UP_CROP)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 61, 97)
    check(got, disp, dr.UP_CROP, "upsampling with a crop")
    # the band the crop removed takes the edge row / column of the cropped map
    h1, w1, top, left, H0, W0 = dr.UP_CROP
    y0, _, _, ly1 = dr.axis_taps(h1, H0, top, dr.HW[0])
    x0, _, _, lx1 = dr.axis_taps(w1, W0, left, dr.HW[1])
    g = got.cpu().numpy()
    rows_band, cols_band = np.flatnonzero((y0 == 0) & (ly1 == 0)), np.flatnonzero((x0 == 0) & (lx1 == 0))
    assert len(rows_band) >= 2 and len(cols_band) >= 2
    assert (g[:, rows_band] == g[:, rows_band[-1]][:, None]).all()
    assert (g[:, :, cols_band] == g[:, :, cols_band[-1]][:, :, None]).all()
    y_last, x_last = np.flatnonzero(y0 == dr.HW[0] - 1), np.flatnonzero(x0 == dr.HW[1] - 1)  # the bottom / right bands
    assert len(y_last) >= 2 and len(x_last) >= 2
    assert (g[:, y_last] == g[:, y_last[-1]][:, None]).all() and (g[:, :, x_last] == g[:, :, x_last[-1]][:, :, None]).all()
    assert np.array_equal(g[:, 0, 0], np.float32(1.0) / disp[:, 0, 0])
    assert np.array_equal(g[:, -1, -1], np.float32(1.0) / disp[:, -1, -1])


def test_downsampling():
    disp = dr.make_disps(3, seed=11)
    got = export(disp, dr.DOWN)
    assert tuple(got.shape) == (3, 13, 19)
    check(got, disp, dr.DOWN, "downsampling")


def test_standard_resize_object_and_scale():
    from vipe_amd.slam.ingest import StandardResize, export_params
    r = StandardResize(160, 600)
    H, W = r.out_size
    disp = dr.make_disps(2, H, W, seed=12)
    got = export(disp, r, depth_scale=2.5)
    assert tuple(got.shape) == (2, 160, 600)
    check(got, disp, export_params(r, H, W), "StandardResize(160, 600)", depth_scale=2.5)


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_identity_is_bitwise_scale_over_disp(scale):
    disp = dr.make_disps(2, seed=13)
    want = np.float32(scale) / disp
    assert np.array_equal(export(disp, None, depth_scale=scale).cpu().numpy(), want)
    assert np.array_equal(export(disp, dr.identity_params(*dr.HW), depth_scale=scale).cpu().numpy(), want)


@pytest.mark.parametrize("params", [dr.UP_CROP, dr.DOWN, None], ids=["up_crop", "down", "identity"])
def test_f16_output_is_the_f32_output_rounded(params):
    disp = dr.make_disps(2, seed=14)
    f32 = export(disp, params)
    f16 = export(disp, params, dtype=torch.float16)
    assert f16.dtype == torch.float16 and torch.equal(f16, f32.half())
    assert torch.equal(export(disp, params, dtype=torch.float16, depth_scale=1000.0), export(disp, params, depth_scale=1000.0).half())


def test_rows_permutation_repeats_and_skipped_entries():
    R = 5
    disp = dr.make_disps(R, seed=15)
    rows = [3, -1, 0, 3, R, 4, 1, -7]
    out = torch.full((len(rows), 61, 97), dr.SENTINEL, dtype=torch.float32, device=dev())
    got = export(disp, dr.UP_CROP, rows=rows, out=out)
    assert got.data_ptr() == out.data_ptr()
    named = [n for n, r in enumerate(rows) if 0 <= r < R]
    skipped = [n for n, r in enumerate(rows) if not 0 <= r < R]
    assert bool(torch.isnan(got[skipped]).all()), "a row outside [0, R) must leave its output as it is"
    check(got[named], disp, dr.UP_CROP, "rows", rows=[rows[n] for n in named])
    assert torch.equal(got[0], got[3])
    # N = 3 with R = 5, and the empty batch
    got3 = export(disp, dr.DOWN, rows=[4, 4, 2])
    check(got3, disp, dr.DOWN, "rows N=3 R=5", rows=[4, 4, 2])
    empty = export(disp, dr.DOWN, rows=[])
    assert tuple(empty.shape) == (0, 13, 19)
    # a fresh output is zero-filled: skipped rows read 0
    fresh = export(disp, dr.DOWN, rows=[R, 1])
    assert not bool(fresh[0].any()) and bool(fresh[1].all())


def test_zero_and_negative_disparities_give_zero():
    disp = dr.make_disps(3, seed=16)
    disp[0, 5:9, 7:21] = 0.0
    disp[0, 15:, :4] = -disp[0, 15:, :4]
    disp[1] = -disp[1]
    disp[2, :3] = 0.0
    ident = export(disp, None).cpu().numpy()
    assert np.array_equal(ident, np.where(disp > 0, np.float32(1.0) / np.where(disp > 0, disp, 1), np.float32(0.0)))
    up = export(disp, dr.UP_CROP)
    assert not bool(up[1].any())                      # an all-negative map
    check(up[2:], disp[2:], dr.UP_CROP, "zero rows")  # bound 0 where all four taps are <= 0, derived elsewhere
    assert not bool(up[2, 0].any()) and bool(up[2, -1].all())
    assert bool((up >= 0).all()) and bool(torch.isfinite(up).all())
    assert torch.equal(export(disp, dr.UP_CROP, dtype=torch.float16), up.half())


def test_return_codes():
    from vipe_amd._lib import F16, F32, F64, lib, ptr
    L = lib()
    disp = torch.from_numpy(dr.make_disps(5, seed=17)).to(dev())
    out = torch.zeros(3, 61, 97, device=dev())
    rows = torch.tensor([0, 1, 2], device=dev())
    s = torch.cuda.current_stream().cuda_stream

    def call(d=disp, r=rows, o=out, dtype=F32, N=3, R=5, H=24, W=40, h1=27, w1=45, top=1, left=2, H0=61, W0=97):
        return L.vipe_depth_export(ptr(d), ptr(r), ptr(o), dtype, N, R, H, W, h1, w1, top, left, H0, W0, 1.0, s)

    EINVAL = -1
    assert call() == 0 and call(r=None) == 0 and call(N=0, d=None, o=None, r=None) == 0
    for bad in (dict(H=0), dict(W=0), dict(h1=0), dict(w1=0), dict(H0=0), dict(W0=0), dict(N=-1), dict(R=-1),
                dict(top=4), dict(left=6), dict(top=-1), dict(left=-1), dict(dtype=F64), dict(dtype=3), dict(d=None),
                dict(o=None), dict(N=6, r=None), dict(N=65536)):
        assert call(**bad) == EINVAL, bad
    # the grid.y limit, asked with an empty batch: a library that did not reject it would return VIPE_OK without a
    # launch - a case with N > 0 would instead write a 262141-row map into this 61-row buffer
    assert call(N=0, H0=4 * 65535 + 1) == EINVAL and call(N=0, H0=4 * 65535) == 0
    assert call(dtype=F16) == 0  # writes 3 * 61 * 97 halves into the f32 buffer: in bounds
    torch.cuda.synchronize()


def test_host_tensors_raise():
    from vipe_amd.slam.ingest import depth_export
    with pytest.raises(NotImplementedError):
        depth_export(torch.from_numpy(dr.make_disps(1)), None)
    with pytest.raises(RuntimeError):
        depth_export(torch.from_numpy(dr.make_disps(1)).to(dev()), None, rows=torch.tensor([0]))  # rows on the host
    with pytest.raises(RuntimeError):
        depth_export(torch.from_numpy(dr.make_disps(1)).to(dev()), (27, 45, 1, 2, 61))
