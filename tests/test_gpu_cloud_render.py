"""`vipe_cloud_render` / `vipe_cloud_resolve` on the device against tests/cloud_render_reference.py: the exact scene against
its integer z-buffer bit for bit (ties included), the seeded cases under `compare_zbuf`'s criterion, the shapes that break
things at small size (all points on one pixel, footprints clipped at every border and corner, nothing drawn, points that
are not finite), splitting, repeating and batching compared bitwise, the resolve's optional outputs, the panorama's seam
and pole, MEI with k1 != 0, and `FusedCloud.render`."""
import numpy as np
import pytest
import torch

import cloud_render_reference as rr

pytestmark = pytest.mark.gpu

ARGS = ("xyz", "cams", "intrinsics", "camera", "geom", "point_size", "max_radius", "index_base")


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def render(case, zbuf=None, stats=None, points=None, images=None, **over):
    """one launch of the case (the rows `points` of its cloud with their own indices, the images `images`) into `zbuf` (a
    fresh one when None) -> (zbuf, stats), device tensors"""
    from vipe_amd.slam import ingest
    c = {**case, **over}
    xyz, cams, intr, base = c["xyz"], c["cams"], c["intrinsics"], c.get("index_base", 0)
    if points is not None:
        xyz, base = xyz[points], base + points.start
    if images is not None:
        cams, intr = cams[images], intr[images]
    H0, W0 = c["geom"][6:]
    zbuf = ingest.cloud_zbuffer(cams.shape[0], H0, W0, dev()) if zbuf is None else zbuf
    stats = ingest.cloud_render(t(xyz), t(cams), t(intr), c["camera"], c["geom"], zbuf, c["point_size"],
                                max_radius=c["max_radius"], index_base=base, stats=stats)
    torch.cuda.synchronize()
    return zbuf, stats


def exact_case(point_size, max_radius, index_base=0):
    sc = rr.exact_scene()
    return dict({k: sc[k] for k in ARGS[:5]}, point_size=point_size, max_radius=max_radius, index_base=index_base), sc


# ---- the exact scene ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("point_size,max_radius", rr.EXACT_DECIDED + [rr.EXACT_MIXED])
def test_exact_scene_bit_for_bit(point_size, max_radius):
    case, sc = exact_case(point_size, max_radius, index_base=5)
    want, stats = rr.exact_zbuf(sc, point_size, max_radius, index_base=5)
    zbuf, got = render(case)
    assert np.array_equal(zbuf.cpu().numpy(), want), "the integer z-buffer, ties included"
    assert got.tolist() == stats, "drawn, invalid, outside"


# ---- the seeded cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rr.CASES)
def test_seeded_cases(name):
    case, ref = rr.cached_case(name)
    zbuf, stats = render(case)
    pinned, loose = rr.compare_zbuf(zbuf.cpu().numpy(), ref, stats.cpu().numpy())
    print(f"{name}: {pinned} pixels pinned to the winner, {loose} within bounds, counters {stats.tolist()}")
    assert pinned > 0.5 * (pinned + loose)


# ---- shapes that break things -------------------------------------------------------------------------------------------

def _pixel_scene(px, py, Z, point_size, max_radius, H=23, W=41):
    """points that project onto the centres of the pixels (px, py) at depths Z through the exact scene's camera"""
    px, py, Z = (np.asarray(v, dtype=np.float64) for v in (px, py, Z))
    xyz = np.stack([(px - 20.5) / 32.0 * Z, (py - 11.5) / 32.0 * Z, Z], 1).astype(np.float32)
    return dict(xyz=xyz, cams=np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32), intrinsics=np.array([[32.0, 32.0, 20.5, 11.5]], np.float32),
                camera="pinhole", geom=rr.identity_geom(H, W), point_size=point_size, max_radius=max_radius, index_base=0)


def test_maximum_contention_all_points_on_one_pixel():
    M = 3000
    rng = np.random.default_rng(3)
    Z = rng.choice(np.array([1.0, 2.0, 4.0, 8.0]), size=M)
    Z[1234] = Z[2345] = 0.5  # the nearest, twice: the lower index wins
    case = _pixel_scene(np.full(M, 7.0), np.full(M, 5.0), Z, 0.0, 2)
    zbuf, stats = render(case)
    want = np.full((1, 23, 41), rr.EMPTY, np.int64)
    want[0, 5, 7] = rr.pack(0.5, 1234)
    assert np.array_equal(zbuf.cpu().numpy(), want) and stats.tolist() == [M, 0, 0]


def test_footprints_are_clipped_at_every_border_and_corner():
    H, W = 23, 41
    px = [0, W - 1, 0, W - 1, 20, 20, 0, W - 1, -2, W + 1, 20, 20, -3, W + 2]
    py = [0, 0, H - 1, H - 1, 0, H - 1, 11, 11, 11, 11, -2, H + 1, 11, 11]
    M = len(px)
    case = _pixel_scene(px, py, np.full(M, 1.0), 0.25, 2)  # q = 4: radius 2 everywhere
    zbuf, stats = render(case)
    want = np.full((H, W), np.iinfo(np.uint64).max, np.uint64)
    drawn = 0
    for m in range(M):
        y0, y1, x0, x1 = max(py[m] - 2, 0), min(py[m] + 2, H - 1), max(px[m] - 2, 0), min(px[m] + 2, W - 1)
        if y0 <= y1 and x0 <= x1:
            drawn += 1
            seg = want[y0:y1 + 1, x0:x1 + 1]
            np.minimum(seg, rr.pack(1.0, m).view(np.uint64), out=seg)
    assert drawn == M - 2, "centres two pixels outside still reach the image, three pixels outside do not"
    assert np.array_equal(zbuf.cpu().numpy()[0], want.view(np.int64)) and stats.tolist() == [drawn, 0, M - drawn]


def test_nothing_drawn_leaves_the_buffer_untouched():
    case = _pixel_scene([5, 5, 200, -300, 5], [5, 5, 5, 5, 4000], [-1.0, 0.05, 1.0, 1.0, 2.0], 0.25, 2)
    zbuf, stats = render(case)
    assert bool((zbuf == -1).all()) and stats.tolist() == [0, 2, 3]


def test_points_that_are_not_finite_are_outside():
    nan, inf = float("nan"), float("inf")
    xyz = np.array([[nan, 0, 1], [0, nan, 1], [0, 0, nan], [inf, 0, 1], [0, -inf, 1], [0, 0, inf], [0, 0, -inf], [nan, nan, nan],
                    [inf, inf, inf], [0.013, 0.021, 1.0]], np.float32)
    rot = np.array([[0.1, -0.2, 0.0, 0.05, 0.1, 0.15, 0.98]], np.float32)  # a general rotation: no zero in the matrix
    for cams in (np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32), rot):
        for camera in ("pinhole", "panorama"):
            case = dict(xyz=xyz, cams=cams, intrinsics=np.array([[32.0, 32.0, 20.5, 11.5]], np.float32), camera=camera,
                        geom=rr.identity_geom(23, 41), point_size=0.25, max_radius=2, index_base=0)
            zbuf, stats = render(case)
            ref = rr.cloud_render_ref(**case)
            assert ref["decided"].all() and ref["status"][0][:9].tolist() == [rr.OUTSIDE] * 9
            want = [int((ref["status"] == k).sum()) for k in range(3)]
            assert stats.tolist() == want and want[1] == 0 and want[2] >= 9, \
                f"{camera}: the nine points that are not finite count as outside"
            rr.compare_zbuf(zbuf.cpu().numpy(), ref, stats.cpu().numpy())
            assert bool((zbuf != -1).any()) == bool(want[0]), "only the finite point is drawn"


# ---- order, splitting, repetition, batching: compared bitwise -----------------------------------------------------------

def test_index_base_two_launches_over_the_halves_in_either_order():
    case, _ = rr.cached_case("pinhole_up_crop")
    M = case["xyz"].shape[0]
    whole, stats = render(case)
    a, b = slice(0, M // 3), slice(M // 3, M)
    for first, second in ((a, b), (b, a)):
        zbuf, st = render(case, points=first)
        render(case, zbuf=zbuf, stats=st, points=second)
        assert torch.equal(zbuf, whole) and torch.equal(st, stats)
    perm = np.random.default_rng(0).permutation(M)  # another point order: the indices move, depths and coverage do not
    shuffled, st = render(dict(case, xyz=case["xyz"][perm]))
    assert torch.equal(shuffled >> 32, whole >> 32) and torch.equal(st, stats)


def test_rendering_twice_changes_nothing():
    case, _ = rr.cached_case("mei_up_crop")
    zbuf, stats = render(case)
    once = zbuf.clone()
    render(case, zbuf=zbuf, stats=stats)
    B, M = case["cams"].shape[0], case["xyz"].shape[0]
    assert torch.equal(zbuf, once) and int(stats.sum()) == 2 * B * M


def test_images_one_by_one_equal_the_batch():
    case, _ = rr.cached_case("rig_two_views")
    whole, stats = render(case)
    total = torch.zeros_like(stats)
    for b in range(case["cams"].shape[0]):
        one, st = render(case, images=slice(b, b + 1))
        assert torch.equal(one[0], whole[b]), f"image {b}"
        total += st
    assert torch.equal(total, stats)


# ---- the resolve --------------------------------------------------------------------------------------------------------

def test_resolve_outputs():
    from vipe_amd.slam import ingest
    case, _ = rr.cached_case("pinhole_up_crop")
    base, M = case["index_base"], case["xyz"].shape[0]
    zbuf, _ = render(case)
    zb = zbuf.cpu().numpy()
    rgb_points = np.random.default_rng(1).integers(0, 256, (base + M, 3), dtype=np.uint8)
    d32, d16, rgb, index = rr.resolve_ref(zb, rgb_points)
    assert (index == -1).any() and (index >= base).any(), "empty and drawn pixels"
    depth, colour, idx = ingest.cloud_resolve(zbuf, t(rgb_points), dtype=torch.float32, want_index=True)
    assert np.array_equal(depth.cpu().numpy(), d32) and np.array_equal(colour.cpu().numpy(), rgb) and np.array_equal(idx.cpu().numpy(), index)
    assert depth.dtype == torch.float32 and colour.dtype == torch.uint8 and idx.dtype == torch.int32
    depth, colour, idx = ingest.cloud_resolve(zbuf)
    assert colour is None and idx is None and depth.dtype == torch.float16
    assert np.array_equal(depth.cpu().numpy(), d16), "fp16: the round-to-nearest-even of the fp32 image"
    assert (d32[index == -1] == 0).all() and (rgb[index == -1] == 0).all()
    # colours for fewer points than the buffer names: the pixels past them are 0, nothing faults
    short = rgb_points[:base + M // 2]
    _, _, rgb_short, _ = rr.resolve_ref(zb, short)
    _, colour, _ = ingest.cloud_resolve(zbuf, t(short))
    assert np.array_equal(colour.cpu().numpy(), rgb_short) and (rgb_short[index >= base + M // 2] == 0).all()
    assert (index >= base + M // 2).any()
    # no images: nothing to do
    depth, colour, idx = ingest.cloud_resolve(ingest.cloud_zbuffer(0, 5, 7, dev()), t(rgb_points), want_index=True)
    assert tuple(depth.shape) == (0, 5, 7) and tuple(colour.shape) == (0, 5, 7, 3) and tuple(idx.shape) == (0, 5, 7)


# ---- cameras ------------------------------------------------------------------------------------------------------------

def test_panorama_seam_and_pole():
    H, W = 24, 40
    xyz = np.array([[1e-3, 0.13, -2.0], [-1e-3, 0.13, -2.0], [0.07, -2.0, 0.05], [0.0, 2.0, 1e-4], [0.0, 0.0, 0.05]], np.float32)
    case = dict(xyz=xyz, cams=np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32), intrinsics=np.zeros((1, 4), np.float32),
                camera="panorama", geom=rr.identity_geom(H, W), point_size=2.0, max_radius=2, index_base=0)
    ref = rr.cloud_render_ref(**case)
    assert ref["decided"].all()
    zbuf, stats = render(case)
    zb = zbuf.cpu().numpy()
    assert np.array_equal(zb == -1, rr.reference_zbuf(ref) == -1) and stats.tolist() == [3, 2, 0]
    rr.compare_zbuf(zb, ref, stats.cpu().numpy())
    _, index, _ = rr.unpack(zb)
    assert set(np.nonzero((index[0] == 0) | (index[0] == 1))[1]) == {W - 3, W - 2, W - 1, 0, 1, 2}, "columns wrap at the seam"
    assert set(np.nonzero(index[0] == 2)[0]) == {0, 1, 2}, "rows are clipped at the pole"


def test_mei_with_distortion():
    case, ref = rr.cached_case("mei_up_crop")
    assert (case["intrinsics"][:, 4] > 0.3).all()
    pin = dict(case, camera="pinhole", intrinsics=np.ascontiguousarray(case["intrinsics"][:, :4]))
    zbuf, _ = render(case)
    other, _ = render(pin)
    assert not torch.equal(zbuf, other), "k1 takes part in the projection"


# ---- the public route ---------------------------------------------------------------------------------------------------

def test_fused_cloud_render_and_rescale():
    from vipe_amd.slam.interface import FusedCloud, rescale_fused_cloud
    case, _ = rr.cached_case("pinhole_up_crop")
    z = case["xyz"][:, 2]
    case = dict(case, xyz=case["xyz"][(z > 1.5) | (z < -1.0)])  # no point near the depth limit 0.1: it does not scale
    M = case["xyz"].shape[0]
    rng = np.random.default_rng(2)
    key = np.sort(rng.permutation(10 * M)[:M]).astype(np.int64)  # sorted: the cloud keeps the rows' order
    rgb_points = rng.integers(0, 256, (M, 3), dtype=np.uint8)
    voxel = case["point_size"]
    cloud = FusedCloud(t(case["xyz"]), t(rgb_points), torch.ones(M, dtype=torch.int32, device=dev()), t(key), voxel, [M, 0, 0, 0])
    zbuf, _ = render(case, index_base=0)
    d32, d16, rgb, index = rr.resolve_ref(zbuf.cpu().numpy(), rgb_points)
    depth, colour, idx = cloud.render(t(case["cams"]), t(case["intrinsics"]), "pinhole", case["geom"], max_radius=case["max_radius"],
                                      want_index=True)
    assert np.array_equal(depth.cpu().numpy(), d16) and np.array_equal(colour.cpu().numpy(), rgb) and np.array_equal(idx.cpu().numpy(), index)
    depth, colour, idx = cloud.render(t(case["cams"]), t(case["intrinsics"][0]), "pinhole", case["geom"], point_size=voxel,
                                      max_radius=case["max_radius"], dtype=torch.float32, color=False)
    assert np.array_equal(depth.cpu().numpy(), d32) and colour is None and idx is None, "one intrinsics row for all images"
    # the cloud and the cameras rescaled by a power of two: the same pixels, depths in the new units
    s = 4.0
    big = rescale_fused_cloud(cloud, s)
    cams = case["cams"].copy()
    cams[:, :3] *= np.float32(s)
    depth_s, _, idx_s = big.render(t(cams), t(case["intrinsics"]), "pinhole", case["geom"], max_radius=case["max_radius"],
                                   dtype=torch.float32, want_index=True)
    assert np.array_equal(idx_s.cpu().numpy(), index) and np.array_equal(depth_s.cpu().numpy(), d32 * np.float32(s))
