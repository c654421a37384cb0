"""Float64 reference, scenes and the float32 error bound of `vipe_cloud_fuse` / `vipe_cloud_extract` (a helper, not a test
module).

Definition (include/vipe_amd.h).  Per pixel (x, y) of map n of the export grid, with the taps of
tests/depth_export_reference.py:

    take   = x % stride == 0 and y % stride == 0 and rows[n] inside [0, R) and (no conf or (conf & 15) >= min_agree)
    d      = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * e)     the export's blend;  kept = take and d > 0
    (u, v) = (ix0 + lx1, iy0 + ly1);  ray = iproj(intrinsics[view], u, v)
    (Rm,t) = ((rig[view]^-1 G[slot])^-1;   X = Rm ray + t d;   Xw = X / d;   s = Xw * inv_voxel,  inv_voxel = f32(1 / voxel)
    i      = floor(s) per axis; in range iff |i| < 2^20 on all three;  q = min(255, floor((s - i) * 256))
    key    = (ix + 2^20) | (iy + 2^20) << 21 | (iz + 2^20) << 42
    table[key] += (1, qx, qy, qz, r, g, b);  a float colour c is int(clamp(c, 0, 1) * 255 + 0.5) in float32

Taps, weights AND the blend d are evaluated in float32 here, operation by operation as the kernel does (the library is
built without contraction): d is an input shared by kernel and reference, so `kept` is exact.  The colour bytes are exact
for the same reason.  Everything from the ray on is float64.

Decided pixels.  A pixel's voxel is DECIDED when on every axis the distance of s to the nearest integer exceeds the
float32 error bound ds of s (floor changes nowhere else, and the range limits are integers), or when some axis is out of
range by more than its bound.  Its offset q on an axis is decided when the distance of 256 s to the nearest integer
exceeds 256 ds.  An undecided pixel may land in any voxel floor(s -+ ds) per axis (its candidates, at most 8).

Error bound of s, from the kernel's operation count; u = 2^-24, every product and sum rounded on its own.
 transform   (rig^-1 G)^-1 through lie_math.h: the bookkeeping of depth_consistency_reference._Chain (a load normalises
             the quaternion: 5u; an inverse re-normalises: +5u and rotates t; a product adds its operands' errors + 13u);
             the matrix entries then lie within eR = 4 eq + 8u, the translation within et.
 ray         depth_consistency_reference._ray: pinhole 2u relative, MEI (20 + 15 A) u relative, panorama 36u absolute.
 X           seven roundings: 7u (sum |Rm_ij b_j| + |t_i| d) + eR sum |b_j| + sum |Rm_ij| eb_j + et d;  d itself is exact
 Xw = X / d  one correctly rounded division: dX / d + u |Xw|
 s           one product with the float32 inv_voxel (the same number on both sides): dXw * inv_voxel + u |s|
The bound is doubled (second-order terms, the float64 reference's own roundings).  At the test sizes (points within about
6 units, voxels of 0.04 to 0.1) it comes out at 2e-3 to 4e-3 of a voxel, so 0.7 to 1.6 % of the kept pixels lie that close to a voxel face on one of the
three axes, under the 2 % cap that tests/test_cloud_fuse_reference.py verifies per case (a pixel whose blended
disparity is nearly zero has a larger bound: 0.16 voxels at most in `edge_entries`).  The derivation was written down
before the first device run and not changed since.
"""
import numpy as np

import depth_consistency_reference as cr
import depth_export_reference as dr

U = cr.U
SAFETY = 2.0
BIAS = 1 << 20
EMPTY = -1
SATURATED = 1 << 23
PROBE_LIMIT = 128
HASH_MUL = 0x9E3779B97F4A7C15
STATS = ("inserted", "dropped_full", "out_of_range", "saturated")


def hash_start(key, cap):
    """the first slot the kernel probes for `key` in a table of `cap` slots"""
    return (((int(key) * HASH_MUL) & (2 ** 64 - 1)) >> 32) & (cap - 1)


def make_key(idx):
    """int64 [...,3] voxel indices -> int64 keys"""
    idx = np.asarray(idx, dtype=np.int64)
    return (idx[..., 0] + BIAS) | ((idx[..., 1] + BIAS) << 21) | ((idx[..., 2] + BIAS) << 42)


def key_index(key):
    key = np.asarray(key, dtype=np.int64)
    return np.stack([((key >> (21 * i)) & 0x1FFFFF) - BIAS for i in range(3)], axis=-1)


def colour_bytes(rgb):
    """rgb uint8 / float16 / float32 [...] -> int64 bytes as the kernel converts them"""
    rgb = np.asarray(rgb)
    if rgb.dtype == np.uint8:
        return rgb.astype(np.int64)
    c = rgb.astype(np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(c), np.float32(0), np.minimum(np.maximum(c, np.float32(0)), np.float32(1)))
    return (c * np.float32(255) + np.float32(0.5)).astype(np.float32).astype(np.int64)


def blend32(m, params):
    """one map [H,W] float32 -> (d [H0,W0] float32 in the kernel's arithmetic, u, v [H0,W0] float64)"""
    h1, w1, top, left, H0, W0 = params
    H, W = m.shape
    y0, y1, ly0, ly1 = dr.axis_taps(h1, H0, top, H)
    x0, x1, lx0, lx1 = dr.axis_taps(w1, W0, left, W)
    a, b, c, e = m[y0][:, x0], m[y0][:, x1], m[y1][:, x0], m[y1][:, x1]
    wy0, wy1, wx0, wx1 = ly0[:, None], ly1[:, None], lx0[None, :], lx1[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * e)
    assert d.dtype == np.float32
    u = np.broadcast_to((x0 + lx1.astype(np.float64))[None, :], (H0, W0))
    v = np.broadcast_to((y0 + ly1.astype(np.float64))[:, None], (H0, W0))
    return d, u, v


def cloud_fuse_ref(disp, poses, rig, intrinsics, camera, params, rows, voxel, conf=None, min_agree=0, rgb=None, stride=1):
    """-> dict of per-pixel arrays [N,H0,W0(,3)]: take, kept (bool), xw (float64 world point), s, ds (float64: the voxel
    coordinate and its doubled float32 bound), idx (int64 voxel index, 0 where not finite), q (int64), m_s, m_q (margin
    of s / of 256 s to the nearest integer), in_range, decided, q_decided [..,3] (bool), colour (int64 bytes, 0 without
    rgb), and inv_voxel"""
    code = cr.CAMERA_CODE.get(camera, camera)
    disp = np.asarray(disp)
    assert disp.dtype == np.float32 and disp.ndim == 3
    poses, rig = np.asarray(poses, dtype=np.float32), np.asarray(rig, dtype=np.float32)
    intrinsics = np.asarray(intrinsics, dtype=np.float32)
    R, H, W = disp.shape
    V = rig.shape[0]
    h1, w1, top, left, H0, W0 = params
    rows = np.arange(R, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    N = rows.shape[0]
    inv = float(np.float32(1.0 / voxel))
    grid = (np.arange(H0)[:, None] % stride == 0) & (np.arange(W0)[None, :] % stride == 0)
    out = dict(take=np.zeros((N, H0, W0), bool), kept=np.zeros((N, H0, W0), bool), in_range=np.zeros((N, H0, W0), bool),
               decided=np.ones((N, H0, W0), bool), q_decided=np.ones((N, H0, W0, 3), bool),
               idx=np.zeros((N, H0, W0, 3), np.int64), q=np.zeros((N, H0, W0, 3), np.int64),
               colour=np.zeros((N, H0, W0, 3), np.int64), inv_voxel=inv)
    for name in ("xw", "s", "ds", "m_s", "m_q"):
        out[name] = np.zeros((N, H0, W0, 3))
    if rgb is not None:
        out["colour"] = colour_bytes(rgb)
    for n in range(N):
        r = int(rows[n])
        if not 0 <= r < R:
            continue
        p, vw = divmod(r, V)
        d32, u, v = blend32(disp[r], params)
        take = grid if conf is None else grid & ((np.asarray(conf[n]) & 15) >= min_agree)
        with np.errstate(invalid="ignore"):
            kept = take & (d32 > 0)
        d = np.where(kept, d32.astype(np.float64), 1.0)
        T = (cr._Chain.load(rig[vw]).inv() * cr._Chain.load(poses[p])).inv()
        Rm, t, eR, et = cr._qmatrix(T.q), T.t, 4 * T.eq + 8 * U, T.et
        ray, eb = cr._ray(code, intrinsics[vw], u, v, H, W)
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            for i in range(3):
                X = Rm[i, 0] * ray[0] + Rm[i, 1] * ray[1] + Rm[i, 2] * ray[2] + t[i] * d
                dX = (7 * U * (np.abs(Rm[i, 0] * ray[0]) + np.abs(Rm[i, 1] * ray[1]) + np.abs(Rm[i, 2] * ray[2]) + np.abs(t[i]) * d)
                      + eR * (np.abs(ray[0]) + np.abs(ray[1]) + np.abs(ray[2]))
                      + np.abs(Rm[i, 0]) * eb[0] + np.abs(Rm[i, 1]) * eb[1] + np.abs(Rm[i, 2]) * eb[2] + et * d)
                xw = X / d
                dxw = dX / d + U * np.abs(xw)
                s = xw * inv
                ds = SAFETY * (dxw * inv + U * np.abs(s))
                out["xw"][n, ..., i], out["s"][n, ..., i], out["ds"][n, ..., i] = xw, s, ds
        s, ds = out["s"][n], out["ds"][n]
        fin = np.isfinite(s) & (np.abs(s) < 2.0 ** 40)  # beyond: certainly out of range, and not an int64 any more
        sf = np.where(fin, s, 0.0)
        fl = np.floor(sf)
        out["idx"][n] = fl.astype(np.int64)
        out["q"][n] = np.minimum(255, np.floor((sf - fl) * 256.0).astype(np.int64))
        out["m_s"][n] = np.abs(sf - np.rint(sf))
        out["m_q"][n] = np.abs(sf * 256.0 - np.rint(sf * 256.0))
        in_range = (fin & (np.abs(fl) < BIAS)).all(-1)
        out_sure = (~fin | (np.abs(s) - ds > BIAS)).any(-1)
        out["take"][n], out["kept"][n], out["in_range"][n] = take, kept, kept & in_range
        out["decided"][n] = ~kept | out_sure | (out["m_s"][n] > ds).all(-1)
        out["q_decided"][n] = out["m_q"][n] > 256.0 * ds
    return out


def expected_table(ref):
    """the reference's pixels -> dict: keys [K] int64 (sorted), sums [K,7] int64 over the DECIDED in-range pixels, cand
    [K] (undecided pixels that may land in the voxel), q_und [K,3] (decided pixels of the voxel whose q is undecided on
    that axis), n_kept, n_out (decided out-of-range pixels), n_undecided.  Voxels that only undecided pixels can reach
    are listed too, with zero sums."""
    kept, dec = ref["kept"], ref["decided"]
    sel = kept & dec & ref["in_range"]
    keys_px = make_key(ref["idx"][sel])
    vals = np.concatenate([np.ones((keys_px.shape[0], 1), np.int64), ref["q"][sel], ref["colour"][sel]], axis=1)
    und = kept & ~dec
    cand_keys = []
    s_u, e_u = ref["s"][und], ref["ds"][und]
    for s, e in zip(s_u, e_u):
        opts = [sorted({int(np.floor(s[i] - e[i])), int(np.floor(s[i] + e[i]))}) for i in range(3)]
        for ix in opts[0]:
            for iy in opts[1]:
                for iz in opts[2]:
                    if max(abs(ix), abs(iy), abs(iz)) < BIAS:
                        cand_keys.append(int(make_key(np.array([ix, iy, iz]))))
    keys = np.unique(np.concatenate([keys_px, np.array(cand_keys, dtype=np.int64)]))
    pos = np.searchsorted(keys, keys_px)
    sums = np.zeros((keys.shape[0], 7), np.int64)
    np.add.at(sums, pos, vals)
    q_und = np.zeros((keys.shape[0], 3), np.int64)
    np.add.at(q_und, pos, (~ref["q_decided"][sel]).astype(np.int64))
    cand = np.zeros(keys.shape[0], np.int64)
    np.add.at(cand, np.searchsorted(keys, np.array(cand_keys, dtype=np.int64)), 1)
    return dict(keys=keys, sums=sums, cand=cand, q_und=q_und, n_kept=int(kept.sum()), n_undecided=int(und.sum()),
                n_out=int((kept & dec & ~ref["in_range"]).sum()))


def table_rows(keys, acc):
    """a device table (numpy: keys [cap] int64, acc [cap,8] int32) -> (sorted keys [K], sums [K,7] int64, slots [K]); every
    key sits in one slot only and an empty slot holds zeros"""
    keys, acc = np.asarray(keys), np.asarray(acc)
    assert keys.dtype == np.int64 and acc.dtype == np.int32 and acc.shape == (keys.shape[0], 8)
    used = keys != EMPTY
    assert not acc[~used].any(), "an empty slot holds no sums"
    assert not acc[:, 7].any(), "the eighth lane is unused"
    k = keys[used]
    order = np.argsort(k)
    assert np.unique(k).shape[0] == k.shape[0], "a voxel lives in one slot only"
    sums = acc[used][:, :7].view(np.uint32).astype(np.int64)  # 32-bit patterns read as unsigned
    return k[order], sums[order], np.nonzero(used)[0][order]


def compare_table(keys, acc, stats, exp, exact=False):
    """the criterion of the device tests.  Per voxel k: |D_k| <= count <= |D_k| + cand_k; a voxel no undecided pixel can
    reach has the reference's count and colour sums exactly and each sum of q within the number of its pixels whose q is
    undecided on that axis; counts and drop counters add up to the kept pixels.  `exact`: nothing is undecided and every
    sum is the reference's.  -> (voxels compared exactly, voxels compared loosely); raises AssertionError"""
    gk, gs, _ = table_rows(keys, acc)
    stats = [int(v) for v in np.asarray(stats)]
    assert sum(stats) == exp["n_kept"], f"inserted + drops {stats} must add up to the {exp['n_kept']} kept pixels"
    assert int(gs[:, 0].sum()) == stats[0], "the counts add up to the inserted points"
    assert exp["n_out"] <= stats[2] <= exp["n_out"] + exp["n_undecided"], "out-of-range count"
    if stats[1] == 0 and stats[3] == 0:
        assert np.isin(gk, exp["keys"]).all(), "a voxel the reference cannot reach"
    got = np.zeros((exp["keys"].shape[0], 7), np.int64)  # the device's sums in the reference's order, zero where absent
    present = np.isin(exp["keys"], gk)
    got[present] = gs[np.searchsorted(gk, exp["keys"][present])]
    if exp["keys"].shape[0] == 0:
        return 0, 0
    if stats[1] == 0 and stats[3] == 0:
        lo, hi = exp["sums"][:, 0], exp["sums"][:, 0] + exp["cand"]
        bad = (got[:, 0] < lo) | (got[:, 0] > hi)
        assert not bad.any(), (f"{int(bad.sum())} voxel counts outside their bounds, first key {exp['keys'][bad][0]}: "
                               f"got {got[bad][0, 0]}, bounds {lo[bad][0]}..{hi[bad][0]}")
        firm = exp["cand"] == 0
        assert (got[firm][:, [0, 4, 5, 6]] == exp["sums"][firm][:, [0, 4, 5, 6]]).all(), "count / colour sums of untouched voxels"
        assert (np.abs(got[firm][:, 1:4] - exp["sums"][firm][:, 1:4]) <= exp["q_und"][firm]).all(), "offset sums of untouched voxels"
        if exact:
            assert exp["n_undecided"] == 0 and not exp["q_und"].any() and (got == exp["sums"]).all()
        return int(firm.sum()), int((~firm).sum())
    # points were dropped: what is stored never exceeds the reference (exact scenes: a stored voxel holds a subset)
    assert (got[:, 0] <= exp["sums"][:, 0] + exp["cand"]).all()
    return 0, int(present.sum())


# ---- the exact scene ----------------------------------------------------------------------------------------------------

EXACT_HW = (23, 41)


def exact_scene(seed=0, N=3, log2_inv_voxel=4, shift=(0.0, 0.0, 0.0)):
    """pinhole fx = fy = 32, cx = 20.5, cy = 11.5 on 23 x 41 maps, identity export, poses that are pure translations by
    multiples of 1/16, disparities drawn from {1, 1/2, 1/4}, uint8 colours, voxel = 2^-log2_inv_voxel: rays are odd
    multiples of 1/64, points and voxel coordinates dyadic numbers of a few bits - every quantity of the kernel is exact
    in float32.  `shift` (multiples of 1/16) moves the cloud."""
    rng = np.random.default_rng(seed)
    H, W = EXACT_HW
    disp = rng.choice(np.array([1.0, 0.5, 0.25], np.float32), size=(N, H, W))
    tw = rng.integers(-24, 25, size=(N, 3)) / 16.0 + np.asarray(shift)  # camera centres in the world
    poses = np.zeros((N, 7), np.float32)
    poses[:, :3] = -tw  # world -> camera of a pure translation
    poses[:, 6] = 1.0
    rig = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    intr = np.array([[32.0, 32.0, 20.5, 11.5]], np.float32)
    rgb = rng.integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    return dict(disp=disp, poses=poses, rig=rig, intrinsics=intr, camera="pinhole", params=dr.identity_params(H, W),
                rows=None, voxel=2.0 ** -log2_inv_voxel, rgb=rgb, centres=tw)


def exact_table(sc, stride=1, rows=None):
    """the table of the exact scene in integers: every voxel coordinate s is scaled by 2^20 to an int64 (asserted exact),
    floor and offset are shifts -> (keys [K] sorted, sums [K,7] int64, n_kept)"""
    N, H, W = sc["disp"].shape
    rows = range(N) if rows is None else rows
    inv = 1.0 / sc["voxel"]
    fx, fy, cx, cy = (float(x) for x in sc["intrinsics"][0])
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    take = (np.arange(H)[:, None] % stride == 0) & (np.arange(W)[None, :] % stride == 0)
    ks, vs = [], []
    for r in rows:
        if not 0 <= r < N:
            continue
        depth = 1.0 / sc["disp"][r].astype(np.float64)
        pts = np.stack([(uu - cx) / fx * depth, (vv - cy) / fy * depth, depth], -1) + sc["centres"][r]
        S = pts * inv * 2.0 ** 20
        Si = np.rint(S).astype(np.int64)
        assert (Si == S).all(), "the scene is not exact"
        i = Si >> 20
        q = np.minimum(255, ((Si - (i << 20)) * 256) >> 20)
        assert (np.abs(i) < BIAS).all()
        ks.append(make_key(i)[take])
        vs.append(np.concatenate([np.ones((H, W, 1), np.int64), q, sc["rgb"][r].astype(np.int64)], -1)[take])
    ks, vs = np.concatenate(ks), np.concatenate(vs)
    keys, posn = np.unique(ks, return_inverse=True)
    sums = np.zeros((keys.shape[0], 7), np.int64)
    np.add.at(sums, posn, vs)
    return keys, sums, int(ks.shape[0])


def extract_ref(keys, sums, voxel, min_count=1):
    """expected output of `vipe_cloud_extract` for table rows (sorted keys, sums [K,7]) -> (xyz float32 [M,3], rgb uint8
    [M,3], count int32 [M], key int64 [M]) sorted by key"""
    keep = sums[:, 0] >= min_count
    k, s = keys[keep], sums[keep]
    cnt = s[:, 0].astype(np.float64)
    v = np.float64(np.float32(voxel))
    xyz = ((key_index(k).astype(np.float64) + (s[:, 1:4] / cnt[:, None] + 0.5) / 256.0) * v).astype(np.float32)
    rgb = ((s[:, 4:7] + (s[:, 0] // 2)[:, None]) // s[:, 0][:, None]).astype(np.uint8)
    return xyz, rgb, s[:, 0].astype(np.int32), k


# ---- seeded cases -------------------------------------------------------------------------------------------------------

# name -> (case of depth_consistency_reference, voxel, min_agree, stride, colour dtype or None)
SEEDED = {
    "pinhole_identity": ("pinhole_identity", 0.05, 2, 1, np.uint8),
    "pinhole_up_crop": ("pinhole_up_crop", 0.05, 1, 1, np.float32),
    "pinhole_down": ("pinhole_down", 0.08, 1, 1, None),
    "mei_up_crop": ("mei_up_crop", 0.05, 2, 2, np.uint8),
    "panorama_identity": ("panorama_identity", 0.1, 1, 1, np.float16),
    "rig_two_views": ("rig_two_views", 0.05, 1, 3, np.uint8),
    "edge_entries": ("edge_entries", 0.05, 0, 1, np.uint8),   # rows with -1, R and repeats; d <= 0 pixels; the gate open
    "stride2_no_conf": ("pinhole_up_crop", 0.04, None, 2, None),  # conf NULL
    "min_agree_8": ("k8", 0.05, 8, 1, None),                      # nothing passes: five neighbours at most
}
CASES = list(SEEDED)
_CACHE = {}


def seeded_case(name):
    """-> dict of `cloud_fuse_ref`'s arguments: the scene and the rows of a case of depth_consistency_reference (the
    surface seen from six slots - world x and y of both signs - or the panorama's shell), gated by that case's
    reference bytes"""
    base, voxel, min_agree, stride, cdt = SEEDED[name]
    case, cref = cr.cached_case(base)
    N = cref["byte"].shape[0]
    H0, W0 = case["params"][4:]
    rgb = None
    if cdt is not None:
        rng = np.random.default_rng(len(name))
        rgb = rng.integers(0, 256, (N, H0, W0, 3), dtype=np.uint8) if cdt == np.uint8 else \
            rng.uniform(-0.1, 1.1, (N, H0, W0, 3)).astype(cdt)  # some values beyond [0, 1]: the clamp
    return dict(disp=case["disp"], poses=case["poses"], rig=case["rig"], intrinsics=case["intrinsics"], camera=case["camera"],
                params=case["params"], rows=case["rows"], voxel=voxel, conf=None if min_agree is None else cref["byte"],
                min_agree=min_agree or 0, rgb=rgb, stride=stride)


def cached_case(name):
    """-> (case, reference, expected table): computed once per process, shared by the tests, never modified"""
    if name not in _CACHE:
        case = seeded_case(name)
        ref = cloud_fuse_ref(**case)
        _CACHE[name] = (case, ref, expected_table(ref))
    return _CACHE[name]
