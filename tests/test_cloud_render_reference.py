"""The cloud renderer without a GPU: the float64 reference of tests/cloud_render_reference.py on its own scenes (the exact
scene against a z-buffer computed with integers, the cap on undecided pairs of every seeded case, the panorama's seam
and pole), `FusedCloud.render`'s and the wrappers' argument checks, the configuration's asserts and - through ctypes, the
library loads without a device - every VIPE_EINVAL path and the M == 0 / B == 0 path of `vipe_cloud_render` and
`vipe_cloud_resolve`."""
import ctypes

import numpy as np
import pytest
import torch

import cloud_render_reference as rr


# ---- the reference on its scenes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("point_size,max_radius", rr.EXACT_DECIDED + [rr.EXACT_MIXED])
def test_exact_scene_reference_equals_integers(point_size, max_radius):
    sc = rr.exact_scene()
    args = {k: sc[k] for k in ("xyz", "cams", "intrinsics", "camera", "geom")}
    ref = rr.cloud_render_ref(**args, point_size=point_size, max_radius=max_radius, index_base=5)
    want, stats = rr.exact_zbuf(sc, point_size, max_radius, index_base=5)
    got = rr.reference_zbuf(ref)
    assert np.array_equal(got, want), "float64 on dyadic numbers of a few bits is exact"
    assert [int((ref["status"] == k).sum()) for k in range(3)] == stats and sum(stats) == ref["status"].size
    assert min(stats) > 100, "drawn, invalid and outside pairs all occur"
    if (point_size, max_radius) in rr.EXACT_DECIDED:
        assert ref["decided"].all(), "every pair of the exact scene is decided"
        assert rr.compare_zbuf(want, ref, stats)[1] > 0
    else:
        assert set(np.unique(ref["r"][ref["status"] == rr.DRAWN])) == {0, 1, 2}, "radii by depth"
    depth, index, empty = rr.unpack(want)
    assert empty[3].all() and not empty[:3].all(), "the camera that looks away draws nothing"
    assert set(np.unique(depth[~empty])) <= {1.0, 2.0, 4.0}


def test_exact_scene_pins_the_tie_rule():
    """pixels on which the two nearest points have EQUAL depth: the lower index wins"""
    sc = rr.exact_scene()
    point_size, max_radius = rr.EXACT_DECIDED[1]
    ref = rr.cloud_render_ref(**{k: sc[k] for k in ("xyz", "cams", "intrinsics", "camera", "geom")}, point_size=point_size,
                              max_radius=max_radius)
    want, _ = rr.exact_zbuf(sc, point_size, max_radius)
    _, index, empty = rr.unpack(want)
    ties = 0
    for b in range(3):
        (pix, pt), _ = rr.coverage(ref, b)
        z = ref["z"][b]
        for p in np.unique(pix):
            zs, ids = z[pt[pix == p]], pt[pix == p]
            if (zs == zs.min()).sum() > 1:
                ties += 1
                assert index[b].reshape(-1)[p] == ids[zs == zs.min()].min()
    assert ties > 50, "several points per pixel, equal depths among them"
    M = sc["xyz"].shape[0]
    assert (index[~empty] < M - 40).any() and not np.isin(index[~empty], np.arange(M - 40, M)).all()


@pytest.mark.parametrize("name", rr.CASES)
def test_seeded_cases_keep_undecided_pairs_under_the_cap(name):
    case, ref = rr.cached_case(name)
    s = rr.summary(ref)
    drawn = ref["status"] == rr.DRAWN
    print(f"{name}: {s}; largest pixel bound {max(ref['evx'][drawn].max(), ref['evy'][drawn].max()):.2e}, "
          f"largest depth bound {ref['ez'][drawn].max():.2e}, undecided share of covering pairs "
          f"{100.0 * s['undecided_covering'] / s['covering']:.3f} %")
    assert s["undecided_covering"] <= 0.02 * s["covering"], "a condition on the inputs: at most 2 % of the covering pairs"
    if case["camera"] == "panorama":  # the whole sphere is the image: nothing finite is outside
        assert s["drawn"] > 500 and s["invalid"] > 15 and s["outside"] == 0
    else:
        assert s["drawn"] > 500 and s["invalid"] > 50 and s["outside"] > 50, "every outcome occurs"
    H, W, h1, w1, top, left, H0, W0 = case["geom"]
    r = ref["r"][drawn]
    if case["point_size"] == 0 or case["max_radius"] == 0:
        assert (r == 0).all()
    else:
        assert set(np.unique(r)) == set(range(case["max_radius"] + 1)), "every radius up to the cap"
    if top or left:  # points that land in the band the export replicate-pads: in front of column `left` of the SLAM grid
        x = (ref["vx"] * (w1 / W0) - 0.5 - left)[drawn]
        assert ((x < -0.5) & (ref["px"][drawn] >= 0)).sum() > 5, "points inside the crop band are drawn"
    zb = rr.reference_zbuf(ref)
    pinned, loose = rr.compare_zbuf(zb, ref)
    assert pinned > 0.5 * (pinned + loose), "the reference's own buffer passes its criterion; most winners are separated"


def test_panorama_seam_wraps_columns_and_not_rows_and_the_pole_is_guarded():
    H, W = 24, 40
    geom = rr.identity_geom(H, W)
    cams = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    intr = np.zeros((1, 4), np.float32)
    xyz = np.array([[1e-3, 0.13, -2.0],    # just left of the seam behind the camera: x near W - 0.5
                    [-1e-3, 0.13, -2.0],   # just right of it: x near -0.5
                    [0.07, -2.0, 0.05],    # towards the top row (phi small), off the pole by 0.025 rad
                    [0.0, 2.0, 1e-4],      # inside the pole guard: invalid
                    [0.0, 0.0, 0.05]], np.float32)  # within 0.1 of the camera: invalid
    ref = rr.cloud_render_ref(xyz, cams, intr, "panorama", geom, point_size=2.0, max_radius=2)
    assert ref["decided"].all()
    assert ref["status"][0].tolist() == [rr.DRAWN, rr.DRAWN, rr.DRAWN, rr.INVALID, rr.INVALID]
    assert ref["r"][0][:3].tolist() == [2, 2, 2]
    for m, centre in ((0, W - 1), (1, 0)):
        only = rr.cloud_render_ref(xyz[m:m + 1], cams, intr, "panorama", geom, point_size=2.0, max_radius=2)
        _, index, empty = rr.unpack(rr.reference_zbuf(only))
        rows, cols = np.nonzero(~empty[0])
        assert sorted(set(cols)) == sorted({(centre + d) % W for d in range(-2, 3)}), "the footprint wraps at the seam"
        assert len(set(rows)) == 5 and rows.min() > 0 and rows.max() < H - 1
    top = rr.cloud_render_ref(xyz[2:3], cams, intr, "panorama", geom, point_size=2.0, max_radius=2)
    _, _, empty = rr.unpack(rr.reference_zbuf(top))
    rows, _ = np.nonzero(~empty[0])
    assert sorted(set(rows)) == [0, 1, 2] and top["py"][0, 0] == 0, "rows are clipped at the pole, not wrapped"
    assert abs(top["z"][0, 0] - np.sqrt(0.07 ** 2 + 4.0 + 0.05 ** 2)) < 1e-6, "the panorama's depth is the range"


# ---- host code ----------------------------------------------------------------------------------------------------------

def test_config_asserts():
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    cpu = torch.device("cpu")
    d = SLAMConfig()
    assert (d.fused_depth, d.fused_depth_max_radius, d.fused_depth_color, d.fused_depth_sink) == (False, 2, False, None)
    ok = dict(fused_depth=True, fused_cloud=True, frame_depth=True, frame_depth_conf=True)
    SLAMSystem(cpu, SLAMConfig(**ok))
    SLAMSystem(cpu, SLAMConfig(**ok, fused_depth_color=True, fused_depth_max_radius=0))
    SLAMSystem(cpu, SLAMConfig(fused_depth_max_radius=9))  # off: the values are not looked at
    for bad in (dict(fused_cloud=False), dict(fused_depth_max_radius=5), dict(fused_depth_max_radius=-1),
                dict(fused_depth_color=True, fused_cloud_color=False)):
        with pytest.raises(AssertionError):
            SLAMSystem(cpu, SLAMConfig(**{**ok, **bad}))
    with pytest.raises(AssertionError):
        SLAMSystem(cpu, SLAMConfig(fused_depth=True))


def test_output_fields_default_to_none():
    from vipe_amd.slam.interface import SLAMOutput
    out = SLAMOutput(trajectory=None, intrinsics=None)
    assert out.fused_depths is None and out.fused_rgb is None


def test_render_params():
    from vipe_amd.slam.ingest import StandardResize, render_params
    r = StandardResize(160, 600)
    assert render_params(r) == (*r.out_size, *r.size, r.crop[0], r.crop[2], 160, 600)
    assert render_params((24, 40)) == (24, 40, 24, 40, 0, 0, 24, 40) == render_params(None, (24, 40))
    assert render_params((24, 40, 27, 45, 1, 2, 61, 97)) == (24, 40, 27, 45, 1, 2, 61, 97)
    for bad in ((1, 2, 3), (27, 45, 1, 2, 61, 97)):
        with pytest.raises(RuntimeError):
            render_params(bad)
    with pytest.raises(RuntimeError):
        render_params(None)


def test_wrappers_reject_cpu_tensors_and_bad_sizes():
    from vipe_amd.slam import ingest
    cpu = torch.device("cpu")
    zbuf = ingest.cloud_zbuffer(2, 5, 7, cpu)
    assert zbuf.dtype == torch.int64 and tuple(zbuf.shape) == (2, 5, 7) and bool((zbuf == -1).all())
    assert tuple(ingest.cloud_zbuffer(0, 5, 7, cpu).shape) == (0, 5, 7)
    for bad in ((-1, 5, 7), (1, 0, 7), (1, 5, 0)):
        with pytest.raises(RuntimeError):
            ingest.cloud_zbuffer(*bad, cpu)
    xyz, cams, intr = torch.zeros(3, 3), torch.zeros(2, 7), torch.zeros(2, 4)
    with pytest.raises(NotImplementedError):
        ingest.cloud_render(xyz, cams, intr, "pinhole", None, zbuf, 0.02)
    with pytest.raises(NotImplementedError):
        ingest.cloud_resolve(zbuf)


def test_fused_cloud_render_argument_checks():
    from vipe_amd.slam.interface import FusedCloud
    cloud = FusedCloud(torch.zeros(4, 3), None, torch.ones(4, dtype=torch.int32), torch.arange(4), 0.02, [4, 0, 0, 0])
    cams, intr = torch.zeros(2, 7), torch.tensor([32.0, 32.0, 20.5, 11.5])
    with pytest.raises(NotImplementedError):
        cloud.render(cams, intr, "pinhole", (23, 41))  # a host cloud: the kernel is HIP
    for bad in (dict(cams_w2c=torch.zeros(7)), dict(cams_w2c=torch.zeros(2, 6)), dict(intrinsics=torch.zeros(3, 4)),
                dict(size_or_resize=None), dict(size_or_resize=(1, 2, 3)), dict(point_size=-1.0)):
        kw = dict(cams_w2c=cams, intrinsics=intr, camera="pinhole", size_or_resize=(23, 41))
        kw.update(bad)
        with pytest.raises(RuntimeError):
            cloud.render(**kw)


# ---- the entry points' argument rules, through ctypes -------------------------------------------------------------------

OK, EINVAL = 0, -1
P = ctypes.c_void_p(64)  # never dereferenced: every call below returns before a launch
NULL = None


def _render(**over):
    from vipe_amd._lib import lib
    a = dict(xyz=P, M=0, index_base=0, cams=P, intr=P, intr_dim=4, camera=0, B=2, H=24, W=40, h1=27, w1=45, top=1, left=2,
             H0=61, W0=97, point_size=0.02, max_radius=2, zbuf=P, stats=P)
    assert set(over) <= set(a)
    a.update(over)
    return lib().vipe_cloud_render(a["xyz"], a["M"], a["index_base"], a["cams"], a["intr"], a["intr_dim"], a["camera"], a["B"],
                                   a["H"], a["W"], a["h1"], a["w1"], a["top"], a["left"], a["H0"], a["W0"], a["point_size"],
                                   a["max_radius"], a["zbuf"], a["stats"], None)


def test_cloud_render_argument_rules():
    assert _render() == OK, "M == 0: no launch"
    assert _render(M=5, B=0) == OK, "B == 0: no launch"
    assert _render(xyz=NULL, cams=NULL, intr=NULL, zbuf=NULL, stats=NULL) == OK, "M == 0 looks at no pointer"
    assert _render(index_base=2 ** 31 - 1) == OK and _render(M=0, B=65535) == OK
    for bad in (dict(M=-1), dict(B=-1), dict(B=65536), dict(index_base=-1), dict(index_base=2 ** 31 - 1, M=1),
                dict(index_base=5, M=2 ** 31 - 5), dict(H=0), dict(W0=0), dict(top=-1), dict(top=4), dict(left=6),
                dict(H0=(1 << 24) + 1, h1=24, w1=40, top=0, left=0), dict(camera=3), dict(camera=-1), dict(intr_dim=5),
                dict(camera=1, intr_dim=4), dict(camera=2), dict(point_size=-0.1), dict(point_size=float("inf")),
                dict(point_size=float("nan")), dict(max_radius=-1), dict(max_radius=5)):
        assert _render(**bad) == EINVAL, f"{bad} must be refused"
    assert _render(camera=2, h1=24, w1=40, top=0, left=0) == OK, "the panorama takes the identity crop (any output size)"
    assert _render(camera=1, intr_dim=5) == OK and _render(point_size=0.0, max_radius=0) == OK and _render(max_radius=4) == OK
    for name in ("xyz", "cams", "intr", "zbuf", "stats"):
        assert _render(M=1, **{name: NULL}) == EINVAL, f"{name} NULL with M, B > 0"


def _resolve(**over):
    from vipe_amd._lib import lib
    a = dict(zbuf=P, B=0, H0=61, W0=97, depth=P, dtype=0, rgb_points=P, M_total=10, rgb_out=P, index=P)
    assert set(over) <= set(a)
    a.update(over)
    return lib().vipe_cloud_resolve(a["zbuf"], a["B"], a["H0"], a["W0"], a["depth"], a["dtype"], a["rgb_points"], a["M_total"],
                                    a["rgb_out"], a["index"], None)


def test_cloud_resolve_argument_rules():
    assert _resolve() == OK and _resolve(dtype=1) == OK, "B == 0: no launch"
    assert _resolve(zbuf=NULL, depth=NULL, rgb_points=NULL, rgb_out=NULL, index=NULL) == OK, "B == 0 looks at no pointer"
    for bad in (dict(B=-1), dict(H0=0), dict(W0=0), dict(H0=-3), dict(M_total=-1), dict(dtype=2), dict(dtype=3), dict(dtype=-1),
                dict(B=65536, H0=65536, W0=65536), dict(B=1, zbuf=NULL), dict(B=1, depth=NULL),
                dict(B=1, rgb_points=NULL, M_total=10)):
        assert _resolve(**bad) == EINVAL, f"{bad} must be refused"
