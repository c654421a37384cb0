"""The float64 oracle of `vipe_depth_export` (tests/depth_export_reference.py, written from the formula with explicit
indexing) against an independent composition - torch's float32 replicate pad + bilinear interpolate + reciprocal - so
that the oracle's taps, crop offsets and clamps are checked without the kernel; the identity case; `StandardResize`
parameters against the kernel's argument conditions; the entry point's argument checks (a rejected call launches
nothing, so they need no GPU); the defaults of the new configuration and output fields."""
import numpy as np
import pytest
import torch

import depth_export_reference as dr


@pytest.mark.parametrize("params", [dr.UP_CROP, dr.DOWN], ids=["up_crop", "down"])
def test_reference_matches_torch_float32_composition(params):
    disp = dr.make_disps(3, seed=1)
    ref = dr.depth_export_ref(disp, params)
    bound = dr.depth_bound(disp, params)
    got = dr.torch_composition(torch.from_numpy(disp), params).numpy()
    assert got.dtype == np.float32 and got.shape == ref.shape == (3, params[4], params[5])
    err = np.abs(got.astype(np.float64) - ref)
    print(f"torch f32 vs reference: max err / bound = {(err / bound).max():.3f}, max rel = {(err / ref).max():.3e}")
    assert np.isfinite(bound).all() and (err <= bound).all()


def test_crop_band_takes_the_edge_values():
    """native pixels whose source lies in the band the crop removed equal their neighbours inside: the first output rows /
    columns map to src <= off and are constant along the axis"""
    disp = dr.make_disps(1, seed=2)
    h1, w1, top, left, H0, W0 = dr.UP_CROP
    ref = dr.depth_export_ref(disp, dr.UP_CROP)[0]
    y0, _, _, ly1 = dr.axis_taps(h1, H0, top, dr.HW[0])
    x0, _, _, lx1 = dr.axis_taps(w1, W0, left, dr.HW[1])
    rows_in_band = np.flatnonzero((y0 == 0) & (ly1 == 0))
    cols_in_band = np.flatnonzero((x0 == 0) & (lx1 == 0))
    assert len(rows_in_band) >= 2 and len(cols_in_band) >= 2  # more than the one pixel that lands on the edge itself
    assert (ref[rows_in_band] == ref[rows_in_band[-1]]).all()
    assert (ref[:, cols_in_band] == ref[:, cols_in_band[-1]][:, None]).all()
    assert ref[0, 0] == 1.0 / np.float64(disp[0, 0, 0])
    assert ref[-1, -1] == 1.0 / np.float64(disp[0, -1, -1])   # the bottom / right bands: src clamped to n_in - 1


@pytest.mark.parametrize("scale", [1.0, 2.5])
def test_identity_is_scale_over_disp_bitwise(scale):
    disp = dr.make_disps(2, seed=3)
    ref = dr.depth_export_ref(disp, dr.identity_params(*dr.HW), depth_scale=scale)
    want = np.float32(scale) / disp  # float32 division, correctly rounded
    assert np.array_equal(ref.astype(np.float32), want)
    assert (np.abs(ref - want.astype(np.float64)) <= dr.depth_bound(disp, dr.identity_params(*dr.HW), depth_scale=scale)).all()


def test_rows_and_nonpositive_disparities():
    disp = dr.make_disps(5, seed=4)
    disp[1] = -disp[1]
    disp[2, :3] = 0.0
    rows = [4, 1, 1, 2]
    ref = dr.depth_export_ref(disp, dr.UP_CROP, rows=rows)
    bound = dr.depth_bound(disp, dr.UP_CROP, rows=rows)
    assert np.array_equal(ref[0], dr.depth_export_ref(disp[4:5], dr.UP_CROP)[0])
    assert not ref[1].any() and not ref[2].any() and not bound[1].any()  # an all-negative map: exact zeros
    assert not ref[3, 0].any() and bound[3, 0].max() == 0 and ref[3, -1].all()


@pytest.mark.parametrize("size", [(1080, 1920), (720, 1280), (2160, 3840), (480, 640), (160, 600), (1920, 1080), (777, 333)])
def test_standard_resize_parameters_satisfy_the_kernel(size):
    from vipe_amd.slam.ingest import StandardResize, export_params
    r = StandardResize(*size)
    h1, w1, top, left, H0, W0 = export_params(r, *r.out_size)
    H, W = r.out_size
    assert (H0, W0) == size and (h1, w1) == r.size
    assert min(H, W, h1, w1, H0, W0) > 0 and 0 <= top <= 7 and 0 <= left <= 7
    assert top + H <= h1 and left + W <= w1 and h1 - H <= 7 and w1 - W <= 7
    assert (H0 + 3) // 4 <= 65535
    assert np.float32(h1) / np.float32(H0) >= 2.0 ** -5 and np.float32(w1) / np.float32(W0) >= 2.0 ** -5
    assert export_params(None, H, W) == (H, W, 0, 0, H, W)
    with pytest.raises(RuntimeError):
        export_params(r, H + 8, W)


def test_abi_exposes_depth_export_and_rejects_bad_arguments():
    from vipe_amd import _lib
    protos = _lib.parse_header()
    assert "vipe_depth_export" in protos and len(protos["vipe_depth_export"][1]) == 16
    L = _lib.lib()
    assert L.vipe_amd_abi_version() == 4
    p = 0x1000  # never dereferenced: every call below is rejected before a launch

    def call(disp=p, rows=None, out=p, dtype=_lib.F16, N=3, R=5, H=24, W=40, h1=27, w1=45, top=1, left=2, H0=61, W0=97):
        return L.vipe_depth_export(disp, rows, out, dtype, N, R, H, W, h1, w1, top, left, H0, W0, 1.0, None)

    assert call(N=0, disp=None, out=None) == 0                     # the empty batch: no launch, no pointers needed
    for bad in (dict(H=0), dict(W=0), dict(h1=0), dict(w1=0), dict(H0=0), dict(W0=0), dict(N=-1), dict(R=-1)):
        assert call(**bad) == -1, bad
    assert call(top=4) == -1 and call(left=6) == -1                # the crop leaves (h1, w1)
    assert call(top=-1) == -1 and call(left=-1) == -1
    assert call(dtype=_lib.F64) == -1 and call(dtype=3) == -1
    assert call(disp=None) == -1 and call(out=None) == -1
    assert call(N=6) == -1 and call(N=6, rows=p, disp=None) == -1   # N > R needs rows (then rejected for the null map)
    assert call(N=65536, rows=p) == -1                             # grid.z
    assert call(N=0, H0=4 * 65535 + 1) == -1 and call(N=0, H0=4 * 65535) == 0   # grid.y (empty batch: never a launch)


def test_defaults_leave_frame_depth_off():
    import inspect
    from vipe_amd.slam.interface import SLAMOutput
    from vipe_amd.slam.system import SLAMConfig
    cfg = SLAMConfig()
    assert cfg.frame_depth is False and cfg.frame_depth_sink is None and cfg.frame_depth_dtype == torch.float16
    assert cfg.infill.infill_dense_disp is False and cfg.upsample_disps is False
    sig = inspect.signature(SLAMOutput.__init__).parameters
    assert sig["frame_depths"].default is None and sig["frame_disps_lowres"].default is None
    out = SLAMOutput(trajectory=None, intrinsics=None)
    assert out.frame_depths is None and out.frame_disps_lowres is None
