"""The fused point cloud without a GPU: the float64 reference of tests/cloud_fuse_reference.py on its own scenes (the
exact scene against integers, the analytic surface, the cap on undecided pixels of every seeded case), the PLY writer,
`FusedCloud` / `rescale_fused_cloud`, the configuration's asserts, the wrappers' argument checks and - through ctypes,
the library loads without a device - every VIPE_EINVAL / N == 0 path of `vipe_cloud_fuse` and `vipe_cloud_extract`."""
import ctypes
import struct

import numpy as np
import pytest
import torch

import cloud_fuse_reference as cf
import depth_consistency_reference as cr
import depth_export_reference as dr


# ---- the reference on its scenes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("log2_inv,shift", [(4, (0, 0, 0)), (9, (0, 0, 0)), (-3, (3, 3, 0))])
def test_exact_scene_reference_equals_integers(log2_inv, shift):
    sc = cf.exact_scene(log2_inv_voxel=log2_inv, shift=shift)
    keys, sums, n_kept = cf.exact_table(sc)
    args = {k: sc[k] for k in ("disp", "poses", "rig", "intrinsics", "camera", "params", "rows", "voxel", "rgb")}
    ref = cf.cloud_fuse_ref(**args)
    assert ref["kept"].all() and ref["in_range"].all() and n_kept == ref["kept"].sum()
    # float64 on dyadic numbers of a few bits is exact: floor and offsets are the integers', whatever the margins say
    k2, inv = np.unique(cf.make_key(ref["idx"].reshape(-1, 3)), return_inverse=True)
    s2 = np.zeros((k2.shape[0], 7), np.int64)
    vals = np.concatenate([np.ones((inv.shape[0], 1), np.int64), ref["q"].reshape(-1, 3), ref["colour"].reshape(-1, 3)], 1)
    np.add.at(s2, inv.reshape(-1), vals)
    assert np.array_equal(k2, keys) and np.array_equal(s2, sums)
    if log2_inv == -3:
        assert keys.shape[0] <= 3, "the contention scene: all pixels in one to three voxels"
    if log2_inv == 9:
        assert keys.shape[0] == n_kept, "the overflow scene: a voxel per pixel"


def test_exact_scene_has_wrapping_hash_starts():
    keys, _, _ = cf.exact_table(cf.exact_scene())
    starts = np.array([cf.hash_start(k, 256) for k in keys])
    assert (starts >= 248).sum() >= 2, "keys whose probe sequence starts in the last slots of a 256-slot table"


def _analytic(corrupt_rect=None):
    sc = cr.analytic_scene("pinhole", V=1)
    disp = sc["disp"] if corrupt_rect is None else cr.corrupt(sc["disp"], 2, corrupt_rect)
    return dict(disp=disp, poses=sc["poses"], rig=sc["rig"], intrinsics=sc["intrinsics"], camera="pinhole",
                params=dr.identity_params(*cr.HW))


def test_analytic_scene_centroids_lie_on_the_surface_and_counts_add():
    sc, voxel = _analytic(), 0.05
    ref = cf.cloud_fuse_ref(**sc, rows=None, voxel=voxel)
    exp = cf.expected_table(ref)
    assert ref["kept"].all() and exp["n_undecided"] <= 0.02 * exp["n_kept"]
    xyz, _, count, _ = cf.extract_ref(exp["keys"], exp["sums"], voxel, min_count=1)
    gap = np.abs(xyz[:, 2] - cr.surface_z(xyz[:, 0].astype(np.float64), xyz[:, 1].astype(np.float64)))
    assert gap.max() <= np.sqrt(3) * voxel, "a centroid within one voxel diagonal of the surface"
    assert (xyz[:, 0] < 0).any() and (xyz[:, 0] > 0).any() and (xyz[:, 1] < 0).any(), "both signs of the world coordinates"
    # the same maps fused k times: every voxel's count (and every sum) k-fold
    k = 3
    ref3 = cf.cloud_fuse_ref(**sc, rows=np.tile(np.arange(6), k), voxel=voxel)
    exp3 = cf.expected_table(ref3)
    assert np.array_equal(exp3["keys"], exp["keys"]) and np.array_equal(exp3["sums"], k * exp["sums"])


def test_analytic_scene_gate_removes_the_corrupted_rectangle():
    row, rect = 2, (6, 18, 8, 30)
    sc = _analytic(rect)
    R = sc["disp"].shape[0]
    nbr = np.array([([q for q in range(R) if q != r] + [-1] * 8)[:8] for r in range(R)], dtype=np.int64)
    conf = cr.depth_consistency_ref(**sc, rows=None, nbr=nbr, tol=0.05)
    open_ = cf.cloud_fuse_ref(**sc, rows=None, voxel=0.05)
    gated = cf.cloud_fuse_ref(**sc, rows=None, voxel=0.05, conf=conf["byte"], min_agree=1)
    removed = open_["kept"] & ~gated["kept"]
    sure = (conf["undecided"] == 0) & ((conf["byte"] >> 4) > 0)  # seen by some neighbour, every pair decided
    inside = np.zeros_like(removed)
    inside[row, rect[0]:rect[1], rect[2]:rect[3]] = True
    assert sure.mean() > 0.8 and (inside & sure).sum() > 100
    assert np.array_equal(removed & sure, inside & sure), "exactly the pixels of the corrupted rectangle go"


@pytest.mark.parametrize("name", cf.CASES)
def test_seeded_cases_keep_undecided_pixels_under_the_cap(name):
    case, ref, exp = cf.cached_case(name)
    print(f"{name}: kept {exp['n_kept']}, undecided {exp['n_undecided']}, out of range {exp['n_out']}, voxels {exp['keys'].shape[0]}, "
          f"largest bound {ref['ds'][ref['kept']].max() if exp['n_kept'] else 0:.2e} voxels")
    assert exp["n_undecided"] <= 0.02 * exp["n_kept"], "a condition on the inputs: at most 2 % of the kept pixels"
    if name == "min_agree_8":
        assert exp["n_kept"] == 0
    else:
        assert exp["n_kept"] > 500 and exp["keys"].shape[0] > 50
    if name == "edge_entries":
        assert (ref["take"] & ~ref["kept"]).any(), "pixels whose disparity is not positive"
    assert (ref["take"].sum() == ref["take"][:, ::case["stride"], ::case["stride"]].sum())


# ---- host code ----------------------------------------------------------------------------------------------------------

def _cloud(colour=True, m=5):
    from vipe_amd.slam.interface import FusedCloud
    g = torch.Generator().manual_seed(1)
    key = torch.randperm(1000, generator=g)[:m].to(torch.int64) + (1 << 40)
    xyz = torch.randn(m, 3, generator=g)
    rgb = torch.randint(0, 256, (m, 3), generator=g, dtype=torch.uint8) if colour else None
    count = torch.randint(1, 100, (m,), generator=g, dtype=torch.int32)
    return FusedCloud(xyz, rgb, count, key, 0.02, [m, 1, 2, 3]), (xyz, rgb, count, key)


def _read_ply(path):
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    props = [l.split()[1:] for l in lines if l.startswith("property")]
    fmt = "<" + "".join({"float": "f", "uchar": "B", "int": "i"}[t] for t, _ in props)
    size = struct.calcsize(fmt)
    rows = [struct.unpack_from(fmt, raw, end + i * size) for i in range(n)]
    return lines, [name for _, name in props], rows, len(raw) - end, size


@pytest.mark.parametrize("colour", [True, False])
def test_ply_round_trip(tmp_path, colour):
    from vipe_amd.driver.artifacts import write_ply
    cloud, _ = _cloud(colour)
    path = str(tmp_path / "sub" / "cloud.ply")
    assert write_ply(path, cloud) == 5
    lines, names, rows, nbytes, size = _read_ply(path)
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"] and "element vertex 5" in lines and lines[-2] == "end_header"
    assert names == (["x", "y", "z", "red", "green", "blue", "count"] if colour else ["x", "y", "z", "count"])
    assert size == (19 if colour else 16) and nbytes == 5 * size
    for i, row in enumerate(rows):
        assert list(row[:3]) == cloud.xyz[i].tolist() and row[-1] == int(cloud.count[i])
        if colour:
            assert list(row[3:6]) == cloud.rgb[i].tolist()


def test_fused_cloud_sorts_by_key_and_rescales():
    from vipe_amd.slam.interface import rescale_fused_cloud
    cloud, (xyz, rgb, count, key) = _cloud()
    order = torch.argsort(key)
    assert torch.equal(cloud.key, key[order]) and torch.equal(cloud.xyz, xyz[order]) and torch.equal(cloud.rgb, rgb[order])
    assert torch.equal(cloud.count, count[order]) and len(cloud) == 5
    assert cloud.stats == dict(inserted=5, dropped_full=1, out_of_range=2, saturated=3)
    idx = torch.tensor([[3, -7, 11], [-(1 << 20) + 1, 0, (1 << 20) - 1]])
    cloud.key = torch.from_numpy(cf.make_key(idx.numpy()))
    assert torch.equal(cloud.voxel_index(), idx)
    cloud, _ = _cloud()
    big = rescale_fused_cloud(cloud, 2.5)
    assert torch.equal(big.xyz, cloud.xyz * 2.5) and big.voxel == pytest.approx(0.05) and cloud.voxel == 0.02
    assert torch.equal(big.key, cloud.key) and torch.equal(big.count, cloud.count) and torch.equal(big.rgb, cloud.rgb)
    assert big.stats == cloud.stats and big.stats is not cloud.stats
    assert _cloud(colour=False)[0].rgb is None and rescale_fused_cloud(_cloud(colour=False)[0], 2.0).rgb is None


def test_config_asserts():
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    cpu = torch.device("cpu")
    assert SLAMConfig().fused_cloud is False
    d = SLAMConfig()
    assert (d.fused_cloud_voxel, d.fused_cloud_min_agree, d.fused_cloud_stride, d.fused_cloud_capacity, d.fused_cloud_min_count,
            d.fused_cloud_color) == (0.02, 2, 1, 1 << 22, 2, True)
    ok = dict(fused_cloud=True, frame_depth=True, frame_depth_conf=True)
    SLAMSystem(cpu, SLAMConfig(**ok))
    SLAMSystem(cpu, SLAMConfig(fused_cloud_voxel=-1.0))  # off: the values are not looked at
    for bad in (dict(frame_depth=False, frame_depth_conf=False), dict(fused_cloud_voxel=0.0),
                dict(fused_cloud_voxel=float("inf")), dict(fused_cloud_voxel=float("nan")), dict(fused_cloud_min_agree=9),
                dict(fused_cloud_min_agree=-1), dict(fused_cloud_stride=0), dict(fused_cloud_stride=9),
                dict(fused_cloud_capacity=1000), dict(fused_cloud_capacity=0), dict(fused_cloud_min_count=0)):
        with pytest.raises(AssertionError):
            SLAMSystem(cpu, SLAMConfig(**{**ok, **bad}))
    with pytest.raises(AssertionError):
        SLAMSystem(cpu, SLAMConfig(fused_cloud=True, frame_depth=True))


def test_wrappers_reject_cpu_tensors_and_bad_tables():
    from vipe_amd.slam import ingest
    disp = torch.zeros(2, 8, 8)
    poses, rig, intr = torch.zeros(2, 7), torch.zeros(1, 7), torch.zeros(1, 4)
    table = (torch.full((64,), -1, dtype=torch.int64), torch.zeros(64, 8, dtype=torch.int32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(NotImplementedError):
        ingest.cloud_fuse(disp, poses, rig, intr, "pinhole", None, None, table, 0.02)
    with pytest.raises(NotImplementedError):
        ingest.cloud_extract(table, 0.02)
    with pytest.raises(RuntimeError):
        ingest.cloud_extract(table[:2], 0.02)
    for cap in (0, 48, -4, (1 << 30) + 1):
        with pytest.raises(RuntimeError):
            ingest.cloud_table(cap, torch.device("cpu"))
    keys, acc, stats = ingest.cloud_table(16, torch.device("cpu"))
    assert keys.tolist() == [-1] * 16 and tuple(acc.shape) == (16, 8) and not acc.any() and stats.tolist() == [0] * 4


# ---- the entry points' argument rules, through ctypes -------------------------------------------------------------------

OK, EINVAL = 0, -1
P = ctypes.c_void_p(64)  # never dereferenced: every call below returns before a launch
NULL = None


def _fuse(**over):
    from vipe_amd._lib import lib
    a = dict(disp=P, poses=P, rig=P, intr=P, intr_dim=4, camera=0, rows=NULL, conf=NULL, min_agree=2, rgb=NULL, rgb_dtype=3,
             stride=1, inv_voxel=50.0, keys=P, acc=P, cap=1 << 10, stats=P, N=0, R=4, V=1, H=24, W=40, h1=27, w1=45, top=1,
             left=2, H0=61, W0=97)
    assert set(over) <= set(a)
    a.update(over)
    return lib().vipe_cloud_fuse(a["disp"], a["poses"], a["rig"], a["intr"], a["intr_dim"], a["camera"], a["rows"], a["conf"],
                                 a["min_agree"], a["rgb"], a["rgb_dtype"], a["stride"], a["inv_voxel"], a["keys"], a["acc"],
                                 a["cap"], a["stats"], a["N"], a["R"], a["V"], a["H"], a["W"], a["h1"], a["w1"], a["top"],
                                 a["left"], a["H0"], a["W0"], None)


def test_cloud_fuse_argument_rules():
    assert _fuse() == OK, "N == 0: no launch"
    assert _fuse(disp=NULL, poses=NULL, rig=NULL, intr=NULL, keys=NULL, acc=NULL, stats=NULL) == OK, "N == 0 looks at no pointer"
    for bad in (dict(N=-1), dict(R=-1), dict(H=0), dict(W0=0), dict(top=-1), dict(top=4), dict(left=6), dict(V=0), dict(V=9),
                dict(R=5, V=2), dict(camera=3), dict(camera=-1), dict(intr_dim=5), dict(camera=1, intr_dim=4),
                dict(camera=2), dict(min_agree=-1), dict(min_agree=9), dict(stride=0), dict(stride=9), dict(inv_voxel=0.0),
                dict(inv_voxel=-1.0), dict(inv_voxel=float("inf")), dict(inv_voxel=float("nan")), dict(cap=0), dict(cap=1000),
                dict(cap=-8), dict(cap=1 << 31), dict(rgb=P, rgb_dtype=2), dict(rgb=P, rgb_dtype=7), dict(N=5, R=4),
                dict(N=65536, rows=P), dict(H0=4 * 65536, h1=24, w1=40, top=0, left=0)):
        assert _fuse(**bad) == EINVAL, f"{bad} must be refused"
    assert _fuse(camera=2, h1=24, w1=40, top=0, left=0) == OK, "the panorama takes the identity crop (any output size)"
    assert _fuse(camera=1, intr_dim=5) == OK and _fuse(rgb=NULL, rgb_dtype=99) == OK
    for name in ("disp", "poses", "rig", "intr", "keys", "acc", "stats"):
        assert _fuse(N=1, **{name: NULL}) == EINVAL, f"{name} NULL with N > 0"


def _extract(**over):
    from vipe_amd._lib import lib
    a = dict(keys=P, acc=P, cap=1 << 10, voxel=0.02, min_count=1, xyz=P, rgb=P, count=P, key=P, max_out=8, num=P)
    assert set(over) <= set(a)
    a.update(over)
    return lib().vipe_cloud_extract(a["keys"], a["acc"], a["cap"], a["voxel"], a["min_count"], a["xyz"], a["rgb"], a["count"],
                                    a["key"], a["max_out"], a["num"], None)


def test_cloud_extract_argument_rules():
    for bad in (dict(cap=0), dict(cap=48), dict(cap=-2), dict(cap=1 << 31), dict(voxel=0.0), dict(voxel=-0.1),
                dict(voxel=float("inf")), dict(voxel=float("nan")), dict(min_count=0), dict(min_count=-3), dict(max_out=-1),
                dict(keys=NULL), dict(acc=NULL), dict(num=NULL), dict(xyz=NULL), dict(count=NULL), dict(key=NULL)):
        assert _extract(**bad) == EINVAL, f"{bad} must be refused"
