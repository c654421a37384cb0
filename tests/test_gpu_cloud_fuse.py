"""`vipe_cloud_fuse` / `vipe_cloud_extract` on the device against tests/cloud_fuse_reference.py: the exact scene against its
integer table (keys, counts, all seven sums, the counters), the seeded cases under `compare_table`'s criterion, the shapes
that break things at small size (sizes that are no multiple of the 64 x 4 tile, one to three voxels for all pixels, a voxel
per pixel, a table smaller than the cloud, probe sequences that wrap, points out of range, a saturated voxel), the optional
inputs, order independence compared bitwise, and the extraction."""
import numpy as np
import pytest
import torch

import cloud_fuse_reference as cf

pytestmark = pytest.mark.gpu

GEOM = ("disp", "poses", "rig", "intrinsics", "camera", "params", "rows")


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def fuse(case, cap=1 << 16, table=None, **over):
    """one launch of the case into `table` (a fresh one of `cap` slots when None) -> table"""
    from vipe_amd.slam import ingest
    c = {**case, **over}
    table = ingest.cloud_table(cap, dev()) if table is None else table
    got = ingest.cloud_fuse(t(c["disp"]), t(c["poses"]), t(c["rig"]), t(c["intrinsics"]), c["camera"], c["params"], t(c["rows"]),
                            table, c["voxel"], conf=t(c.get("conf")), min_agree=c.get("min_agree", 0), rgb=t(c.get("rgb")),
                            stride=c.get("stride", 1))
    assert got is table
    torch.cuda.synchronize()
    return table


def host(table):
    return tuple(x.cpu().numpy() for x in table)


def content(table):
    """what a table holds, whatever the slots: (sorted keys, sums, counters)"""
    k, s, _ = cf.table_rows(*host(table)[:2])
    return k, s, table[2].cpu().numpy()


def same_content(a, b):
    return all(np.array_equal(x, y) for x, y in zip(content(a), content(b)))


def exact_expected(sc, **kw):
    keys, sums, n = cf.exact_table(sc, **kw)
    return dict(keys=keys, sums=sums, cand=np.zeros(len(keys), np.int64), q_und=np.zeros((len(keys), 3), np.int64), n_kept=n,
                n_undecided=0, n_out=0)


# ---- the exact scene and the shapes that break things -------------------------------------------------------------------

@pytest.mark.parametrize("log2_inv,shift,what", [(4, (0, 0, 0), "plain"), (-3, (3, 3, 0), "one to three voxels: contention"),
                                                 (9, (0, 0, 0), "a voxel per pixel: the LDS table overflows")])
def test_exact_scene(log2_inv, shift, what):
    sc = cf.exact_scene(log2_inv_voxel=log2_inv, shift=shift)
    exp = exact_expected(sc)
    table = fuse(sc)
    k, s, stats = content(table)
    assert np.array_equal(k, exp["keys"]) and np.array_equal(s, exp["sums"]), what
    assert stats.tolist() == [exp["n_kept"], 0, 0, 0]
    cf.compare_table(*host(table), exp, exact=True)


def test_table_smaller_than_the_cloud():
    sc = cf.exact_scene()
    exp = exact_expected(sc)
    assert exp["keys"].shape[0] > 64
    table = fuse(sc, cap=64)  # the run ends: every point gives up after 64 slots
    k, s, stats = content(table)
    assert stats[1] > 0 and stats[2] == 0 and stats[3] == 0 and stats.sum() == exp["n_kept"], "stored + dropped = kept"
    assert k.shape[0] == 64 and np.isin(k, exp["keys"]).all() and s[:, 0].sum() == stats[0]
    # a key inside the table is found by every later point (the probe limit covers all 64 slots) and a key outside a
    # full table never gets in: a stored voxel loses nothing, what was dropped are whole voxels
    pos = np.searchsorted(exp["keys"], k)
    assert np.array_equal(s, exp["sums"][pos]), "every stored voxel is exact"


def test_probe_sequence_wraps_at_the_end_of_the_table():
    from vipe_amd.slam import ingest
    sc = cf.exact_scene()
    exp = exact_expected(sc)
    cap = 8192
    starts = np.array([cf.hash_start(k, cap) for k in exp["keys"]])
    first = int(starts.max())
    assert first >= cap - 64, "a key of the scene starts in the last slots"
    table = ingest.cloud_table(cap, dev())
    dummy = cf.make_key(np.stack([np.arange(cap - first), np.full(cap - first, -900), np.full(cap - first, 900)], 1))
    assert not np.isin(dummy, exp["keys"]).any()
    table[0][first:] = t(dummy)  # the tail is taken by voxels the scene never touches
    table = fuse(sc, table=table)
    keys, acc, stats = host(table)
    k, s, slots = cf.table_rows(keys, acc)
    mine = np.isin(k, exp["keys"])
    assert np.array_equal(k[mine], exp["keys"]) and np.array_equal(s[mine], exp["sums"]) and not s[~mine].any()
    wrapped = slots[mine][starts == first]
    assert (wrapped < first).all(), "the keys that start at the tail wrapped to the front"
    assert stats.tolist() == [exp["n_kept"], 0, 0, 0]


def test_out_of_range_and_non_finite_points():
    sc = cf.exact_scene()
    disp = sc["disp"].copy()
    disp[0, :4] = np.float32(2.0 ** -30)     # depth 2^30: voxel index 2^34
    disp[0, 4:6] = np.float32(1.2e-38)       # X / d is finite, s overflows to infinity
    disp[0, 8] = np.float32("nan")           # skipped, not counted - and so is every pixel that has it as a tap (0 * nan)
    disp[0, 11] = np.float32(-1.0)           # skipped
    disp[1, 0, :5] = np.float32("inf")       # d = inf: X / d is not a number
    W = disp.shape[2]
    # the reference blends in float32 as the kernel does, non-finite taps included; the scene stays exact elsewhere
    ref = cf.cloud_fuse_ref(**{g: sc[g] for g in GEOM if g != "disp"}, disp=disp, voxel=sc["voxel"], rgb=sc["rgb"])
    kept, sel = ref["kept"], ref["in_range"]
    assert (kept & ~sel).sum() == 6 * W + 1 and 2 * W <= (~kept).sum() <= 3 * W + 5
    table = fuse(dict(sc, disp=disp))
    k, s, stats = content(table)
    assert stats.tolist() == [sel.sum(), 0, (kept & ~sel).sum(), 0]
    kk, inv = np.unique(cf.make_key(ref["idx"][sel]), return_inverse=True)
    ss = np.zeros((kk.shape[0], 7), np.int64)
    np.add.at(ss, inv.reshape(-1), np.concatenate([np.ones((sel.sum(), 1), np.int64), ref["q"][sel], ref["colour"][sel]], 1))
    assert np.array_equal(k, kk) and np.array_equal(s, ss)


def test_saturated_voxel_takes_nothing_more():
    from vipe_amd.slam import ingest
    sc = cf.exact_scene(log2_inv_voxel=-3, shift=(3, 3, 0))
    exp = exact_expected(sc)
    key = int(exp["keys"][0])
    table = ingest.cloud_table(256, dev())
    slot = cf.hash_start(key, 256)
    table[0][slot] = key
    preload = torch.tensor([cf.SATURATED, 11, 12, 13, 14, 15, 16, 0], dtype=torch.int32)
    table[1][slot] = preload.to(dev())
    table = fuse(sc, table=table)
    k, s, stats = content(table)
    at = int(np.searchsorted(k, key))
    assert s[at].tolist() == preload[:7].tolist(), "no sum of the saturated voxel changes"
    assert stats[3] == exp["sums"][0, 0] and stats[0] == exp["n_kept"] - stats[3] and stats[1] == 0
    others = np.arange(k.shape[0]) != at
    assert np.array_equal(k, exp["keys"]) and np.array_equal(s[others], exp["sums"][others])


# ---- the seeded cases ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", cf.CASES)
def test_seeded_case_matches_reference(name):
    case, ref, exp = cf.cached_case(name)
    assert exp["n_undecided"] <= 0.02 * exp["n_kept"], "the cap on undecided pixels, on the very inputs the device gets"
    table = fuse(case)
    firm, loose = cf.compare_table(*host(table), exp)
    stats = table[2].tolist()
    print(f"{name}: kept {exp['n_kept']}, undecided {exp['n_undecided']}; {firm} voxels compared exactly, {loose} within bounds; "
          f"counters {stats}")
    assert stats[1] == 0 and stats[3] == 0
    if exp["n_kept"]:
        assert firm > 0.8 * (firm + loose)
    else:
        assert stats == [0, 0, 0, 0] and not (table[0] != -1).any()


def test_optional_inputs():
    """conf NULL and given, min_agree 0 and 8, rgb NULL / uint8 / float32 (float16 is a seeded case), N = 0"""
    case, ref, exp = cf.cached_case("pinhole_up_crop")
    no_gate = fuse(dict(case, conf=None))
    open_gate = fuse(dict(case, min_agree=0))
    assert same_content(no_gate, open_gate) and no_gate[2][0] > exp["n_kept"]
    shut = fuse(dict(case, min_agree=8))
    assert shut[2].tolist() == [0, 0, 0, 0] and not (shut[0] != -1).any()
    grey = fuse(dict(case, rgb=None))
    k, s, _ = content(grey)
    assert not s[:, 4:].any() and np.array_equal(s[:, :4], content(fuse(case))[1][:, :4])
    as_bytes = cf.colour_bytes(case["rgb"]).astype(np.uint8)
    assert same_content(fuse(case), fuse(dict(case, rgb=as_bytes))), "float colours are converted as stated"
    empty = fuse(dict(case, rows=np.zeros(0, np.int64), conf=np.zeros((0, 61, 97), np.uint8), rgb=np.zeros((0, 61, 97, 3), np.uint8)))
    assert empty[2].tolist() == [0, 0, 0, 0] and not (empty[0] != -1).any()


# ---- order independence, compared bitwise after extraction --------------------------------------------------------------

def extracted(table, voxel, **kw):
    from vipe_amd.slam import ingest
    from vipe_amd.slam.interface import FusedCloud
    xyz, rgb, count, key, num = ingest.cloud_extract(table, voxel, **kw)
    return FusedCloud(xyz, rgb, count, key, voxel, table[2].tolist()), num


def same_cloud(a, b):
    return (torch.equal(a.key, b.key) and torch.equal(a.count, b.count) and torch.equal(a.rgb, b.rgb)
            and torch.equal(a.xyz.view(torch.int32), b.xyz.view(torch.int32)) and a.stats == b.stats)


def test_order_independence():
    case, _, _ = cf.cached_case("pinhole_up_crop")
    rows = case["rows"]
    N = rows.shape[0]
    whole, _ = extracted(fuse(case), case["voxel"])
    again, _ = extracted(fuse(case), case["voxel"])
    assert len(whole) > 100 and same_cloud(whole, again), "the same call twice into fresh tables"
    half = N // 2
    part = lambda sl: dict(case, rows=rows[sl], conf=case["conf"][sl], rgb=case["rgb"][sl])
    table = fuse(part(slice(0, half)))
    table = fuse(part(slice(half, N)), table=table)
    assert same_cloud(whole, extracted(table, case["voxel"])[0]), "one launch over N maps against two over the halves"
    perm = np.random.default_rng(0).permutation(N)
    assert same_cloud(whole, extracted(fuse(part(perm)), case["voxel"])[0]), "permuted rows"
    small, _ = extracted(fuse(case, cap=1 << 15), case["voxel"])
    assert same_cloud(whole, small), "another table size: other slots, the same cloud"


# ---- extraction ---------------------------------------------------------------------------------------------------------

def test_extraction():
    from vipe_amd.slam import ingest
    sc = cf.exact_scene()
    exp = exact_expected(sc)
    table = fuse(sc)
    for min_count in (1, 2, 3):
        cloud, num = extracted(table, sc["voxel"], min_count=min_count)
        xyz, rgb, count, key = cf.extract_ref(exp["keys"], exp["sums"], sc["voxel"], min_count)
        assert num == len(cloud) == key.shape[0] and (0 < num or min_count == 3)
        assert np.array_equal(cloud.key.cpu().numpy(), key), "sorted by key"
        assert np.array_equal(cloud.count.cpu().numpy(), count) and np.array_equal(cloud.rgb.cpu().numpy(), rgb)
        assert np.array_equal(cloud.xyz.cpu().numpy(), xyz), "the centroid is evaluated in double and rounded once"
        assert np.array_equal(cloud.voxel_index().cpu().numpy(), cf.key_index(key))
    M = exp["keys"].shape[0]
    xyz, rgb, count, key, num = ingest.cloud_extract(table, sc["voxel"], max_out=M + 7)
    assert num == M and (key[M:] == -1).all() and not xyz[M:].any() and not count[M:].any() and (key[:M] != -1).all()
    # max_out below M: num is still M; the wrapper's arrays have max_out rows, so the kernel is handed a longer buffer
    # here whose tail must stay untouched
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    short = 10
    bufs = (torch.full((M, 3), -7.0, device=dev()), torch.full((M, 3), 9, dtype=torch.uint8, device=dev()),
            torch.full((M,), -7, dtype=torch.int32, device=dev()), torch.full((M,), -7, dtype=torch.int64, device=dev()))
    n = torch.zeros(1, dtype=torch.int64, device=dev())
    check(lib().vipe_cloud_extract(ptr(table[0]), ptr(table[1]), table[0].shape[0], sc["voxel"], 1, *(ptr(b) for b in bufs), short,
                                   ptr(n), stream_ptr(n)), "vipe_cloud_extract")
    torch.cuda.synchronize()
    assert int(n) == M and (bufs[3][short:] == -7).all() and (bufs[0][short:] == -7).all() and (bufs[2][short:] == -7).all()
    assert (bufs[1][short:] == 9).all() and np.isin(bufs[3][:short].cpu().numpy(), exp["keys"]).all()
    assert len(set(bufs[3][:short].tolist())) == short
    xyz, rgb, count, key, num = ingest.cloud_extract(table, sc["voxel"], max_out=short)
    assert num == M and key.shape[0] == short
    # without colour, and an empty table
    xyz, rgb, count, key, num = ingest.cloud_extract(table, sc["voxel"], color=False)
    assert rgb is None and num == M
    xyz, rgb, count, key, num = ingest.cloud_extract(ingest.cloud_table(64, dev()), 0.1)
    assert num == 0 and xyz.shape == (0, 3) and rgb.shape == (0, 3) and count.shape == (0,) and key.shape == (0,)
    assert len(extracted(ingest.cloud_table(64, dev()), 0.1)[0]) == 0
