"""Native-resolution frame ingest on the GPU: `vipe_frame_ingest` against the reference's `VideoFrame.resize(...).crop(...)`
+ `_precompute_features` + sensor-disparity lines (tests/golden/frame_ingest_reference.npz, cases (b) of
make_golden_ingest.py), against torch's own composition at 1080 x 1920, and `SLAMSystem.run(..., native_resolution=True)`.

Bounds.  images: 2e-5 absolute at the fixture's sizes - coordinates stay below 64, so the fp32 source coordinate is good
to one ulp(64) = 7.6e-6, neighbouring values differ by at most 1, a few ulps of blend arithmetic come on top.  disps_sens:
2e-5 * max|depth| on the pre-reciprocal value, i.e. 1e-4 relative after it (depth >= 0.5 of max 10); zeros stay zero.
mask8: exact (the fixture keeps every pre-threshold value 1e-3 away from 0.9).  x4: exactly what `vipe_enc_prep` makes
of the kernel's own images, and within one fp16 ulp (taken at the reference value) of (images_ref - mean) / std, plus
X4_CARRY / std.  X4_CARRY = 5 * 2^-24 is the most by which two fp32 evaluations of the blend
h0 * (w0 * a + w1 * b) + h1 * (w0 * c + w1 * d) can differ from the same taps and weights (values 0-1, weights summing
to 1) when one contracts products into sums and the other does not: per level two products whose half ulps sum to at
most 2^-25 + 2^-26 (they add up to at most 1, so only one reaches 0.5) and one sum rounded to 2^-25, i.e. 1.25 * 2^-24
for a row, the same again for the column blend, 2.5 * 2^-24 from the exact value for either side.  An fp16 cannot
absorb that near a normalised zero: there its ulp (2^-24 below 6e-5, 1.9e-7 at 1.8e-4) is finer than fp32 holds an image
value around 0.45 (3e-8) once divided by std, so the reference's own last bits move x4 by more than one ulp.  From
|v| = 2e-3 up the carry is under one ulp.  Measured on the MI355X: the images differ from the fixture by at most 1.8e-7
(3 * 2^-24), which in the "upscale" case is 1.40 fp16 ulps at one normalised value of 1.8e-4 out of 6720; every other
value of every case is within 0.51 ulps."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_ingest_reference.npz")
CASES = ["downscale", "upscale", "identity", "mixed_ratio"]
MEAN = torch.tensor([0.485, 0.456, 0.406])
STD = torch.tensor([0.229, 0.224, 0.225])
IMG_TOL = 2e-5
X4_CARRY = 5 * 2.0 ** -24  # module docstring: two fp32 evaluations of one bilinear blend of values 0-1


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Geometry:
    """What `frame_ingest` reads of a `StandardResize`, at sizes of the test's choosing."""

    def __init__(self, native, size, crop):
        self.native_size, self.size, self.crop = tuple(native), tuple(size), tuple(crop)
        self.out_size = (size[0] - crop[0] - crop[1], size[1] - crop[2] - crop[3])


def load_case(name):
    G = np.load(GOLD)
    g = {k: G[f"{name}/{k}"] for k in ("rgb", "mask", "depth", "geometry", "rgb_out", "mask_out", "mask8", "disps_sens")}
    h1, w1, top, bottom, left, right = (int(x) for x in g["geometry"])
    return g, Geometry(g["rgb"].shape[:2], (h1, w1), (top, bottom, left, right))


def run_kernel(geo, rgb, mask=None, depth=None, fill=None):
    """-> images, x4, mask8, disps_sens on the device (the last two prefilled: untouched when their input is None)."""
    from vipe_amd.slam.ingest import frame_ingest
    H, W = geo.out_size
    images = torch.empty((3, H, W), dtype=torch.float32, device=dev())
    x4 = torch.empty((H, W, 4), dtype=torch.float16, device=dev())
    mask8 = torch.zeros((H // 8, W // 8), dtype=torch.bool, device=dev())
    disps = torch.full((H // 8, W // 8), -7.0 if fill is None else fill, dtype=torch.float32, device=dev())
    frame_ingest(rgb, geo, images, x4, mask, mask8 if mask is not None else None, depth, disps if depth is not None else None)
    torch.cuda.synchronize()
    return images, x4, mask8, disps


def fp16_ulp(v):
    """Spacing of fp16 at |v| (subnormal spacing 2^-24 below 2^-14)."""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def check_against_reference(images, x4, mask8, disps, g):
    from vipe_amd.slam.encoders import normalize_images
    ref = torch.from_numpy(g["rgb_out"]).permute(2, 0, 1)
    err = (images.cpu() - ref).abs().max().item()
    print(f"images max|d| = {err:.3e}")
    assert err <= IMG_TOL, err
    assert torch.equal(x4, normalize_images(images[None])[0]), "x4 is not what vipe_enc_prep makes of images"
    want = ((ref - MEAN[:, None, None]) / STD[:, None, None]).permute(1, 2, 0)
    got = x4.cpu().float()
    assert bool((got[..., 3] == 0).all())
    d = (got[..., :3] - want).abs()
    over = (d - (fp16_ulp(want) + X4_CARRY / STD)).max().item()
    print(f"x4 max|d| in fp16 ulps of the reference value = {(d / fp16_ulp(want)).max().item():.3f}")
    assert over <= 0, over
    assert np.array_equal(mask8.cpu().numpy(), g["mask8"])
    ds, ds_ref = disps.cpu().numpy(), g["disps_sens"]
    assert np.array_equal(ds == 0, ds_ref == 0) and (ds_ref == 0).any()
    nz = ds_ref != 0
    pre = np.abs(1.0 / ds[nz].astype(np.float64) - 1.0 / ds_ref[nz].astype(np.float64)).max()
    rel = np.abs(ds[nz] / ds_ref[nz] - 1.0).max()
    print(f"depth max|d| before the reciprocal = {pre:.3e}, relative after = {rel:.3e}")
    assert pre <= 2e-5 * float(g["depth"].max()) and rel <= 1e-4, (pre, rel)


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_the_reference_fixture(name):
    g, geo = load_case(name)
    rgb, mask, depth = (torch.from_numpy(g[k]).to(dev()) for k in ("rgb", "mask", "depth"))
    assert mask.dtype == torch.bool
    check_against_reference(*run_kernel(geo, rgb, mask, depth), g)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16])
@pytest.mark.parametrize("name", ["downscale", "upscale"])
def test_uint8_and_fp16_frames(name, dtype):
    """The same values as 8-bit / half frames: every output equal, bit for bit, to the fp32 run on those values converted
    on the host (x / 255 in fp32 for bytes, the kernel's own IEEE division; fp16 -> fp32 is exact) - inside the fixture
    test's bounds with nothing to spare; the mask may arrive as uint8."""
    g, geo = load_case(name)
    rgb = torch.from_numpy(g["rgb"])
    low = (rgb * 255).round().to(torch.uint8) if dtype == torch.uint8 else rgb.half()
    as_f32 = low.float() / 255.0 if dtype == torch.uint8 else low.float()
    mask, depth = torch.from_numpy(g["mask"]).to(dev()), torch.from_numpy(g["depth"]).to(dev())
    a = run_kernel(geo, low.to(dev()), mask.to(torch.uint8), depth)
    b = run_kernel(geo, as_f32.to(dev()), mask, depth)
    err = (a[0] - b[0]).abs().max().item()
    print(f"{dtype}: images max|d| vs the fp32 run = {err:.3e}")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and bool((a[1][..., 3] == 0).all())
    assert torch.equal(a[2], b[2]) and np.array_equal(a[2].cpu().numpy(), g["mask8"])
    assert torch.equal(a[3], b[3])


def test_absent_mask_and_depth_leave_their_outputs_alone_and_two_views_fill_both():
    from vipe_amd.slam.ingest import StandardResize, ingest_frames
    from vipe_amd.slam.system import Frame
    g, geo = load_case("downscale")
    rgb = torch.from_numpy(g["rgb"]).to(dev())
    images, x4, mask8, disps = run_kernel(geo, rgb, fill=-7.0)
    assert not bool(mask8.any()) and bool((disps == -7.0).all())  # as prefilled
    full = run_kernel(geo, rgb, torch.from_numpy(g["mask"]).to(dev()), torch.from_numpy(g["depth"]).to(dev()))
    assert torch.equal(images, full[0]) and torch.equal(x4, full[1])

    # two views of one size through the host layer, at the policy's own geometry for 60 x 100 frames
    gen = torch.Generator().manual_seed(3)
    r = StandardResize(60, 100)
    H, W = r.out_size
    views = [Frame(rgb=torch.rand(60, 100, 3, generator=gen).to(dev()),
                   mask=(torch.rand(60, 100, generator=gen) > 0.02).to(dev()),
                   metric_depth=(0.5 + 9.5 * torch.rand(60, 100, generator=gen)).to(dev())) for _ in range(2)]
    im, x, m, d = ingest_frames(views, r, dev())
    assert im.shape == (2, 3, H, W) and x.shape == (2, H, W, 4) and m.shape == (2, H // 8, W // 8) and d.shape == m.shape
    for v in range(2):
        one = run_kernel(r, views[v].rgb, views[v].mask, views[v].metric_depth)
        assert torch.equal(im[v], one[0]) and torch.equal(x[v], one[1]) and torch.equal(m[v], one[2]) and torch.equal(d[v], one[3])
    assert not torch.equal(im[0], im[1]) and bool(m.any()) and not bool(m.all())
    views[1].mask = None  # the existing rule: masks only when every view carries one
    assert ingest_frames(views, r, dev())[2] is None
    views[0].metric_depth = views[1].metric_depth = None
    assert ingest_frames(views, r, dev())[3] is None


def test_large_coordinates_against_torch_at_1080p():
    """One 1080 x 1920 fp32 frame made on the device, through the policy's geometry (332 x 591, crop to 328 x 584), against
    torch's own F.interpolate + crop + slice composition on the same GPU.  images within 1e-6: source coordinates reach
    1900, where one ulp of `src` is 1.2e-4 of lambda - only the same `src` arithmetic agrees (torch's device kernel fuses
    scale * (dst + 0.5) - 0.5 into one multiply-add; 1.2e-7 measured; `scratch/ingest_time.py --unfused-src` measures the
    form with product and difference rounded separately).  x4 is `vipe_enc_prep` of the images here too.  Masks equal,
    except at cells one of whose four resized-mask pixels lies within 1e-4 of 0.9 in the torch composition (at most 0.1 %
    of the cells; the blob is chosen so that the composition has none)."""
    from vipe_amd.slam.ingest import StandardResize
    r = StandardResize(1080, 1920)
    assert r.size == (332, 591) and r.crop == (2, 2, 3, 4) and r.out_size == (328, 584)
    (h1, w1), (top, _, left, _), (H, W) = r.size, r.crop, r.out_size
    gen = torch.Generator(device=dev()).manual_seed(11)
    rgb = torch.rand(1080, 1920, 3, generator=gen, device=dev())
    depth = 0.5 + 9.5 * torch.rand(1080, 1920, generator=gen, device=dev())
    yy, xx = torch.meshgrid(torch.arange(1080, device=dev()).float(), torch.arange(1920, device=dev()).float(), indexing="ij")
    mask = ((yy - 500.3) / 310.7) ** 2 + ((xx - 1010.6) / 420.2) ** 2 > 1.0
    images, x4, mask8, disps = run_kernel(r, rgb, mask, depth)

    want = F.interpolate(rgb.permute(2, 0, 1)[None], (h1, w1), mode="bilinear")[0][:, top:top + H, left:left + W]
    d = (images - want).abs()
    err = d.max().item()
    c, y, x = np.unravel_index(int(d.argmax().item()), tuple(d.shape))
    print(f"images max|d| vs torch = {err:.3e} at channel {c}, row {y}, column {x}")
    assert err <= 1e-6, f"max|d| {err:.3e} at channel {c}, row {y}, column {x}"
    from vipe_amd.slam.encoders import normalize_images
    assert torch.equal(x4, normalize_images(images[None])[0])

    soft = F.interpolate(mask[None, None].float(), (h1, w1), mode="bilinear")[0, 0][top:top + H, left:left + W]
    soft8 = F.interpolate((soft > 0.9)[None, None].float(), (H // 8, W // 8), mode="bilinear")[0, 0]
    want8 = ~(soft8 > 0.9)
    near = (soft - 0.9).abs() < 1e-4
    unsure = near[3::8, 3::8] | near[3::8, 4::8] | near[4::8, 3::8] | near[4::8, 4::8] | ((soft8 - 0.9).abs() < 1e-4)
    assert int(unsure.sum()) == 0, "the blob was chosen so that torch's own composition is nowhere near the threshold"
    assert int(unsure.sum()) <= 0.001 * unsure.numel()
    assert bool(want8.any()) and not bool(want8.all())
    assert torch.equal(mask8[~unsure], want8[~unsure])


def test_slam_system_runs_from_native_resolution_frames():
    """`SLAMSystem.run(..., native_resolution=True)` on a 14-frame random clip rendered at 96 x 160 with intrinsics given at
    that size (random-init weights: pinned is the bookkeeping): one pose per frame, the buffer at the policy's size, the
    intrinsics stored forward and returned recovered, and keyframe 0 holding exactly what the ingest makes of frame 0."""
    from vipe_amd.ext.lietorch import SE3
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.ingest import StandardResize, ingest_frames
    from vipe_amd.slam.system import Frame, SLAMConfig, SLAMSystem

    gen = torch.Generator().manual_seed(8)
    T, H0, W0 = 14, 96, 160
    rgb = torch.rand(T, H0, W0, 3, generator=gen).to(dev())
    depth = (1.0 + 4.0 * torch.rand(T, H0, W0, generator=gen))
    depth[:, 10:30, 20:60] = 0.0
    depth = depth.to(dev())
    yy, xx = torch.meshgrid(torch.arange(H0).float(), torch.arange(W0).float(), indexing="ij")
    mask = (((yy - 40.2) / 21.3) ** 2 + ((xx - 90.4) / 33.1) ** 2 > 1.0).to(dev())
    intr = torch.tensor([144.0, 144.0, 80.0, 48.0])
    frames = []
    for t in range(T):
        pose = SE3(torch.tensor([[-0.05 * t, 0, 0, 0, 0, 0, 1.0]], device=dev())).inv()  # camera -> world
        frames.append(Frame(rgb=rgb[t], metric_depth=depth[t], intrinsics=intr, pose=SE3(pose.data[0]), mask=mask))
    r = StandardResize(H0, W0)
    H, W = r.out_size
    assert (H, W) == (336, 568)
    torch.manual_seed(0)
    cfg = SLAMConfig(buffer=40, filter_thresh=0.0, frontend_backend_iters=(), frontend=FrontendArgs(keyframe_thresh=0.0),
                     infill=InfillArgs(infill_chunk_size=4))
    sysm = SLAMSystem(dev(), cfg)
    out = sysm.run(frames, native_resolution=True)
    torch.cuda.synchronize()
    b = sysm.buffer
    assert out.trajectory.data.shape == (T, 7) and bool(torch.isfinite(out.trajectory.data).all())
    assert (out.trajectory.data[:, 3:].norm(dim=-1) - 1).abs().max().item() < 1e-4
    assert tuple(b.images.shape[-2:]) == (H, W) and tuple(b.fmaps.shape[-2:]) == (H // 8, W // 8)
    assert tuple(b.disps_sens.shape[-2:]) == (H // 8, W // 8) and tuple(b.masks.shape[-2:]) == (H // 8, W // 8)
    assert out.intrinsics.shape == (1, 4)
    assert torch.equal(out.intrinsics[0], r.recover_intrinsics(b.intrinsics[0]))
    assert torch.allclose(b.intrinsics[0].cpu(), r.forward_intrinsics(intr), rtol=1e-6, atol=0)
    assert torch.allclose(out.intrinsics[0].cpu(), intr, rtol=1e-6, atol=0)
    images, x4, masks, disps = ingest_frames([frames[0]], r, dev())
    assert int(b.tstamp[0]) == 0
    assert torch.equal(b.images[0], images.to(b.images.dtype)) and torch.equal(b.masks[0], masks) and torch.equal(b.disps_sens[0], disps)
    assert bool(masks.any()) and not bool(masks.all()) and bool((disps == 0).any()) and bool((disps > 0).any())
