"""Float64 reference, scenes and the float32 error bounds of `vipe_cloud_render` / `vipe_cloud_resolve` (a helper, not a
test module).

Definition (include/vipe_amd.h).  Per point m (index index_base + m) and image b, with (Rm, t) = cams[b] (quaternion
normalised) and geom = (H, W, h1, w1, top, left, H0, W0):

    Xc      = Rm X + t;  not finite: OUTSIDE;  not valid (Z > 0.1 | the panorama's range and pole rule): INVALID
    z       = Xc.z (pinhole, MEI), |Xc| (panorama);  (x, y) = proj(intrinsics[b], Xc)
    v       = ((x + off) + 0.5) / scale per axis, p = floor(v);  unless -max_radius - 1 <= p <= n_out + max_radius: OUTSIDE
    q       = (0.5 point_size) foc / z,  foc = fx / scale_x (pinhole, MEI), W0 / (2 pi) (panorama);  r = min(max_radius, int(q))
    pixels  = [px - r, px + r] x [py - r, py + r], rows clipped, columns clipped (panorama: modulo W0);  none: OUTSIDE
    zbuf[b][y][x] = min(zbuf[b][y][x], float32_bits(z) << 32 | index_base + m)

scale, off, 0.5 point_size and the intrinsics are the float32 numbers the kernel holds; everything else is float64.

Error bounds, from the kernel's operation count; u = 2^-24, every product and sum rounded on its own (the library is built
without contraction), all doubled (`SAFETY`: second-order terms and the reference's own roundings).
 matrix      one rotation matrix from a quaternion that is normalised on load: depth_consistency_reference._Chain.load
             gives eq = 5u, the entries lie within eR = 4 eq + 8u = 28u; t is exact
 Xc          three products and three sums per row, none fused: dX_i = 6u (sum |Rm_ij X_j| + |t_i|) + eR sum |X_j|
 validity    dZ against |Z - 0.1|; the panorama's two tests as depth_consistency_reference._project bounds them
 z           dZ (pinhole, MEI);  dr = dX + dY + dZ + 4u r (panorama)
 projection  depth_consistency_reference._project: (ex, ey)
 v           two sums and one division behind x: ev = (ex + u |x + off| + u |x + off + 0.5|) / scale + u |v|; p is
             decided when |v - rint(v)| > ev (the range limits are integers too), or v lies outside the band by more
 q           the division fx / scale_x (u), one product (u), one division (u) and z's error: eq = q (3u + dz / z); r is
             decided when int(q - eq) == int(q + eq) or q - eq >= max_radius; point_size = 0 gives q = 0 exactly
A pair is DECIDED when every margin its outcome rests on exceeds its bound.  At the seeded scenes (points within about 10
units, focal lengths of 18 to 91 output pixels) the largest ev over the drawn pairs comes out at 2e-4 to 1.2e-3 pixels
(pinhole, MEI; the nearest points) and 5e-2 to 9e-2 pixels (panorama: the points next to the pole guard, where 1 / rho is
large), the largest depth bound at 7e-5 to 1e-4 units: 0.05 to 0.34 % of the pairs that cover a pixel are undecided, under
the 2 % cap tests/test_cloud_render_reference.py verifies (and prints) per case.  The derivation was written down before
the first device run.

The exact scene.  Pinhole fx = fy = 32, cx = 20.5, cy = 11.5 on 23 x 41 images, identity export; cameras with identity
or half-turn quaternions and translations by multiples of 1/16 in x and y; points X = odd / 64, Y = odd / 64, Z in
{1, 2, 4}: x + 0.5 is an odd multiple of 1/8, 1/16 or 1/32 off an integer - every quantity of the kernel is exact in
float32 and the z-buffer follows in integers (`exact_zbuf`).  With point_size a power of two q = 16 point_size / Z is a power
of two as well: it sits ON the radius threshold unless it is below 1 or at least max_radius + its bound.  The
configurations of `EXACT_DECIDED` (radius 0, 1, 2 everywhere) are decided throughout; `EXACT_MIXED` (point_size 1/8:
radii 2, 1, 0 by depth) is exact in the kernel and in float64 all the same and is compared with the integers only.
"""
import numpy as np

import depth_consistency_reference as cr
import depth_export_reference as dr

U = cr.U
SAFETY = cr.SAFETY
DRAWN, INVALID, OUTSIDE = 0, 1, 2
STATS = ("drawn", "invalid", "outside")
EMPTY = -1  # all ones


def identity_geom(H, W):
    return (H, W, H, W, 0, 0, H, W)


def export_geom(params, HW=dr.HW):
    """(h1, w1, top, left, H0, W0) of depth_export_reference on maps of `HW` -> the eight numbers of the entry point"""
    return (*HW, *params)


def pack(z, index):
    """float depth, index -> the z-buffer's int64 (the uint64 pattern)"""
    bits = np.asarray(z, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((bits << np.uint64(32)) | np.asarray(index).astype(np.uint64)).view(np.int64)


def unpack(zbuf):
    """int64 z-buffer -> (depth float32, index int64 (-1 where empty), empty bool)"""
    zb = np.ascontiguousarray(zbuf).view(np.uint64)
    empty = zb == np.uint64(0xFFFFFFFFFFFFFFFF)
    depth = (zb >> np.uint64(32)).astype(np.uint32).view(np.float32)
    index = (zb & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.where(empty, np.float32(0), depth), np.where(empty, -1, index), empty


def cloud_render_ref(xyz, cams, intrinsics, camera, geom, point_size, max_radius, index_base=0):
    """-> dict of per-pair arrays [B,M]: status (DRAWN / INVALID / OUTSIDE), decided, z and ez (depth and its bound), px,
    py, r (the pixel and the radius; meaningful where the pair is valid), the thresholded quantities vx, vy, q with their
    bounds evx, evy, eq and the validity margin over its bound m_valid, and for the undecided pairs the conservative
    ranges px_lo, px_hi, py_lo, py_hi, r_hi; plus geom, camera, max_radius, index_base"""
    code = cr.CAMERA_CODE.get(camera, camera)
    xyz = np.asarray(xyz)
    assert xyz.dtype == np.float32 and xyz.ndim == 2 and xyz.shape[1] == 3
    cams, intrinsics = np.asarray(cams, dtype=np.float32), np.asarray(intrinsics, dtype=np.float32)
    H, W, h1, w1, top, left, H0, W0 = geom
    sx = float(np.float32(w1) / np.float32(W0))
    sy = float(np.float32(h1) / np.float32(H0))
    half = float(np.float32(0.5) * np.float32(point_size))
    mr = int(max_radius)
    B, M = cams.shape[0], xyz.shape[0]
    X = xyz.astype(np.float64).T
    fin_in = np.isfinite(X).all(0)
    assert np.abs(X[:, fin_in]).max(initial=0.0) < 1e30, "finite coordinates stay far from float32's overflow"
    Xs = np.where(fin_in[None], X, 0.0)
    out = {k: np.zeros((B, M)) for k in ("z", "ez", "vx", "vy", "evx", "evy", "q", "eq", "m_valid")}
    out.update({k: np.zeros((B, M), np.int64) for k in ("status", "px", "py", "r", "px_lo", "px_hi", "py_lo", "py_hi", "r_hi")})
    out["decided"] = np.zeros((B, M), bool)
    for b in range(B):
        G = cr._Chain.load(cams[b])
        Rm, t, eR = cr._qmatrix(G.q), G.t, 4 * G.eq + 8 * U
        Xc = Rm @ Xs + t[:, None]
        dX = 6 * U * (np.abs(Rm) @ np.abs(Xs) + np.abs(t)[:, None]) + eR * np.abs(Xs).sum(0)[None]
        P = cr._project(code, intrinsics[b], Xc, dX, H, W)
        valid, m_valid = P["valid"], P["mvalid"]
        if code == cr.PANORAMA:
            z = np.sqrt((Xc * Xc).sum(0))
            dz = dX.sum(0) + 4 * U * z
            foc = float(np.float32(W0)) / (2.0 * cr.PI_F)
        else:
            z, dz = Xc[2], dX[2]
            foc = float(intrinsics[b, 0]) / sx
        zs = np.where(valid, z, 1.0)
        with np.errstate(invalid="ignore", over="ignore"):
            ax, ay = P["x"] + left, P["y"] + top
            vx, vy = (ax + 0.5) / sx, (ay + 0.5) / sy
            evx = P["ex"] / sx + SAFETY * U * ((np.abs(ax) + np.abs(ax + 0.5)) / sx + np.abs(vx))
            evy = P["ey"] / sy + SAFETY * U * ((np.abs(ay) + np.abs(ay + 0.5)) / sy + np.abs(vy))
        vx, vy = np.clip(np.where(valid, vx, 0.0), -1e9, 1e9), np.clip(np.where(valid, vy, 0.0), -1e9, 1e9)
        evx, evy = np.where(valid, evx, 0.0), np.where(valid, evy, 0.0)
        px, py = np.floor(vx).astype(np.int64), np.floor(vy).astype(np.int64)
        lo = -mr - 1
        in_band = (px >= lo) & (px <= W0 + mr) & (py >= lo) & (py <= H0 + mr)
        out_sure = (vx < lo - evx) | (vx > W0 + mr + 1 + evx) | (vy < lo - evy) | (vy > H0 + mr + 1 + evy)
        p_dec = (np.abs(vx - np.rint(vx)) > evx) & (np.abs(vy - np.rint(vy)) > evy)
        q = half * foc / zs
        eq = SAFETY * q * (3 * U + dz / zs)
        r = np.minimum(mr, np.floor(np.minimum(q, mr + 1.0))).astype(np.int64)
        r_lo = np.minimum(mr, np.floor(np.minimum(np.maximum(q - eq, 0.0), mr + 1.0))).astype(np.int64)
        r_hi = np.minimum(mr, np.floor(np.minimum(q + eq, mr + 1.0))).astype(np.int64)
        y0, y1 = np.maximum(py - r, 0), np.minimum(py + r, H0 - 1)
        x0, x1 = (px - r, px + r) if code == cr.PANORAMA else (np.maximum(px - r, 0), np.minimum(px + r, W0 - 1))
        drawn = fin_in & valid & in_band & (y0 <= y1) & (x0 <= x1)
        out["status"][b] = np.where(~fin_in, OUTSIDE, np.where(~valid, INVALID, np.where(drawn, DRAWN, OUTSIDE)))
        out["decided"][b] = ~fin_in | ((m_valid > 1) & (~valid | out_sure | (p_dec & (r_lo == r_hi))))
        out["z"][b], out["ez"][b], out["m_valid"][b] = zs, SAFETY * dz, m_valid
        out["vx"][b], out["vy"][b], out["evx"][b], out["evy"][b], out["q"][b], out["eq"][b] = vx, vy, evx, evy, q, eq
        out["px"][b], out["py"][b], out["r"][b], out["r_hi"][b] = px, py, r, r_hi
        out["px_lo"][b], out["px_hi"][b] = np.floor(vx - evx).astype(np.int64), np.floor(vx + evx).astype(np.int64)
        out["py_lo"][b], out["py_hi"][b] = np.floor(vy - evy).astype(np.int64), np.floor(vy + evy).astype(np.int64)
    out.update(geom=tuple(geom), camera=code, max_radius=mr, index_base=int(index_base))
    return out


def _entries(ref, b, sel, x_lo, x_hi, y_lo, y_hi, reach):
    """the (pixel, point) entries of image b for the points `sel`: columns [x_lo, x_hi], rows [y_lo, y_hi] per point,
    clipped (panorama: columns modulo W0) -> (pix, point) int64 arrays; `reach` bounds the rectangles' half extent"""
    H0, W0 = ref["geom"][6:]
    pano = ref["camera"] == cr.PANORAMA
    pix, pts = [], []
    for dy in range(0, 2 * reach + 3):
        yy = y_lo + dy
        oky = (yy <= y_hi) & (yy >= 0) & (yy < H0)
        for dx in range(0, 2 * reach + 3):
            xx = x_lo + dx
            ok = oky & (xx <= x_hi)
            if pano:
                xx = np.mod(xx, W0)
            else:
                ok &= (xx >= 0) & (xx < W0)
            pix.append((yy * W0 + xx)[ok])
            pts.append(sel[ok])
    assert ((x_hi - x_lo) <= 2 * reach + 2).all() and ((y_hi - y_lo) <= 2 * reach + 2).all()
    return np.concatenate(pix), np.concatenate(pts)


def coverage(ref, b):
    """image b -> (pixD, ptD): entries of the decided drawn pairs; (pixU, ptU): entries the undecided pairs might have"""
    mr = ref["max_radius"]
    st, dec = ref["status"][b], ref["decided"][b]
    D = np.nonzero(dec & (st == DRAWN))[0]
    px, py, r = ref["px"][b][D], ref["py"][b][D], ref["r"][b][D]
    pixD, ptD = _entries(ref, b, D, px - r, px + r, py - r, py + r, mr)
    Un = np.nonzero(~dec)[0]
    rh = ref["r_hi"][b][Un]
    pixU, ptU = _entries(ref, b, Un, ref["px_lo"][b][Un] - rh, ref["px_hi"][b][Un] + rh, ref["py_lo"][b][Un] - rh,
                         ref["py_hi"][b][Un] + rh, mr)
    return (pixD, ptD), (pixU, ptU)


def reference_zbuf(ref):
    """the z-buffer of the reference's own decisions (every pair taken as the reference has it) -> int64 [B,H0,W0]"""
    H0, W0 = ref["geom"][6:]
    B = ref["status"].shape[0]
    out = np.full((B, H0 * W0), np.iinfo(np.uint64).max, np.uint64)
    for b in range(B):
        sel = np.nonzero(ref["status"][b] == DRAWN)[0]
        px, py, r = ref["px"][b][sel], ref["py"][b][sel], ref["r"][b][sel]
        pix, pts = _entries(ref, b, sel, px - r, px + r, py - r, py + r, ref["max_radius"])
        np.minimum.at(out[b], pix, pack(ref["z"][b][pts], pts + ref["index_base"]).view(np.uint64))
    return out.view(np.int64).reshape(B, H0, W0)


def summary(ref):
    """-> dict: pairs, counts per status over the decided pairs, undecided, covering (pairs that cover a pixel or,
    undecided, might) and undecided_covering"""
    dec, st = ref["decided"], ref["status"]
    B = st.shape[0]
    cov = und = 0
    for b in range(B):
        (_, ptD), (_, ptU) = coverage(ref, b)
        cov += np.unique(ptD).shape[0] + np.unique(ptU).shape[0]
        und += np.unique(ptU).shape[0]
    res = {name: int((dec & (st == k)).sum()) for k, name in enumerate(STATS)}
    res.update(pairs=int(st.size), undecided=int((~dec).sum()), covering=int(cov), undecided_covering=int(und))
    return res


def compare_zbuf(zbuf, ref, stats=None):
    """the criterion of the device tests on a z-buffer [B,H0,W0] int64 that started empty and took exactly the launches
    the reference describes.  Per pixel, with D the decided pairs that cover it and Uc the undecided pairs that might:
    empty on the device only if D is empty; otherwise its index belongs to D or Uc, its depth equals that pair's
    reference z within the pair's bound and is no farther than min over D of (z + bound); where Uc is empty and the
    nearest member of D is separated from all others by more than the bounds, the index is the reference's winner.
    `stats` (the launch's three counters): each within the undecided pairs of the reference's count, summing to B M.
    -> (pixels whose index was pinned to the winner, other non-empty pixels); raises AssertionError"""
    H0, W0 = ref["geom"][6:]
    B, M = ref["status"].shape
    zbuf = np.asarray(zbuf)
    assert zbuf.dtype == np.int64 and zbuf.shape == (B, H0, W0)
    depth, index, empty = unpack(zbuf.reshape(B, -1))
    pinned = loose = 0
    for b in range(B):
        (pixD, ptD), (pixU, ptU) = coverage(ref, b)
        z, ez = ref["z"][b], ref["ez"][b]
        nD = np.bincount(pixD, minlength=H0 * W0)
        nU = np.bincount(pixU, minlength=H0 * W0)
        bad = empty[b] & (nD > 0)
        assert not bad.any(), f"image {b}: pixel {np.nonzero(bad)[0][0]} is empty, {nD[bad][0]} decided pairs cover it"
        full = np.nonzero(~empty[b])[0]
        pt = index[b][full] - ref["index_base"]
        assert ((pt >= 0) & (pt < M)).all(), f"image {b}: an index outside the launch's points"
        keys = np.concatenate([pixD * M + ptD, pixU * M + ptU])
        member = np.isin(full * M + pt, keys)
        assert member.all(), (f"image {b}: pixel {full[~member][0]} shows point {pt[~member][0]}, which does not cover it")
        err = np.abs(depth[b][full].astype(np.float64) - z[pt])
        assert (err <= ez[pt]).all(), f"image {b}: depth off by {err.max():.3e}, bound {ez[pt][err.argmax()]:.3e}"
        hi = np.full(H0 * W0, np.inf)
        np.minimum.at(hi, pixD, (z + ez)[ptD])
        assert (depth[b][full] <= hi[full]).all(), f"image {b}: a pixel shows a point behind a decided nearer one"
        # the reference's winner per pixel, and whether it is separated from every other decided pair
        order = np.lexsort((ptD, z[ptD], pixD))
        spix, spt = pixD[order], ptD[order]
        first = np.ones(spix.shape[0], bool)
        first[1:] = spix[1:] != spix[:-1]
        winner = np.full(H0 * W0, -1, np.int64)
        winner[spix[first]] = spt[first]
        second_lo = np.full(H0 * W0, np.inf)
        np.minimum.at(second_lo, spix[~first], (z - ez)[spt[~first]])
        w = winner[full]
        sure = (nU[full] == 0) & (w >= 0)
        sure[sure] &= second_lo[full][sure] > (z + ez)[w[sure]]
        wrong = sure & (pt != w)
        assert not wrong.any(), f"image {b}: pixel {full[wrong][0]} shows point {pt[wrong][0]}, the winner is {w[wrong][0]}"
        pinned += int(sure.sum())
        loose += int((~sure).sum())
    if stats is not None:
        stats = [int(v) for v in np.asarray(stats)]
        s = summary(ref)
        assert sum(stats) == B * M, f"the counters {stats} must add up to the {B * M} pairs"
        for k, name in enumerate(STATS):
            assert s[name] <= stats[k] <= s[name] + s["undecided"], f"{name}: {stats[k]}, reference {s[name]} + at most {s['undecided']}"
    return pinned, loose


def resolve_ref(zbuf, rgb_points=None):
    """expected output of `vipe_cloud_resolve` -> (depth float32, depth float16, rgb uint8 or None, index int32)"""
    depth, index, empty = unpack(np.asarray(zbuf))
    rgb = None
    if rgb_points is not None:
        rgb_points = np.asarray(rgb_points)
        ok = (index >= 0) & (index < rgb_points.shape[0])
        rgb = np.where(ok[..., None], rgb_points[np.where(ok, index, 0)], 0).astype(np.uint8) if rgb_points.shape[0] else \
            np.zeros(index.shape + (3,), np.uint8)
    with np.errstate(over="ignore"):
        return depth, depth.astype(np.float16), rgb, index.astype(np.int32)


# ---- the exact scene ----------------------------------------------------------------------------------------------------

EXACT_HW = (23, 41)
EXACT_DECIDED = [(2.0 ** -5, 2), (0.5, 1), (1.0, 2)]  # (point_size, max_radius): q = .5 / Z, 8 / Z, 16 / Z -> r = 0, 1, 2
EXACT_MIXED = (2.0 ** -3, 2)                           # q = 2 / Z: r = 2, 1, 0 at Z = 1, 2, 4 - on the threshold

# (sign of x and y, sign of z, tx, ty): identity, identity shifted, half turn about z, half turn about y (looks away)
_EXACT_CAMS = [((1, 1, 1), (0, 0)), ((1, 1, 1), (3, -2)), ((-1, -1, 1), (1, 1)), ((-1, 1, -1), (0, 0))]
_EXACT_QUAT = {(1, 1, 1): (0, 0, 0, 1), (-1, -1, 1): (0, 0, 1, 0), (-1, 1, -1): (0, 1, 0, 0)}


def exact_scene(seed=0, M=700, n_dup=40):
    """-> dict(xyz, cams, intrinsics, camera, geom, ints): points with X = odd / 64, Y = odd / 64, Z in {1, 2, 4} spread
    over the image and a border around it, the last `n_dup` of them copies of the first (equal depth on one pixel, two
    indices); `ints` = (Xn, Yn, Z) the integers"""
    rng = np.random.default_rng(seed)
    H, W = EXACT_HW
    Z = rng.choice(np.array([1, 2, 4]), size=M)
    Xn = (2 * rng.integers(-27 * Z, 27 * Z) + 1).astype(np.int64)  # x = 32 X / Z + 20.5 in about [-6.5, 47.5]
    Yn = (2 * rng.integers(-17 * Z, 17 * Z) + 1).astype(np.int64)
    Xn[-n_dup:], Yn[-n_dup:], Z[-n_dup:] = Xn[:n_dup], Yn[:n_dup], Z[:n_dup]
    xyz = np.stack([Xn / 64.0, Yn / 64.0, Z.astype(np.float64)], 1).astype(np.float32)
    cams = np.array([[tx / 16.0, ty / 16.0, 0.0, *_EXACT_QUAT[s]] for s, (tx, ty) in _EXACT_CAMS], np.float32)
    intr = np.tile(np.array([[32.0, 32.0, 20.5, 11.5]], np.float32), (len(_EXACT_CAMS), 1))
    return dict(xyz=xyz, cams=cams, intrinsics=intr, camera="pinhole", geom=identity_geom(H, W), ints=(Xn, Yn, Z.astype(np.int64)))


def exact_zbuf(sc, point_size, max_radius, index_base=0, points=None):
    """the exact scene's z-buffer and counters in integers -> (zbuf int64 [B,H0,W0], [drawn, invalid, outside]); `points`
    restricts the launch to those rows (indices stay index_base + m)"""
    H0, W0 = EXACT_HW
    Xn, Yn, Z = sc["ints"]
    sel = np.arange(Xn.shape[0]) if points is None else np.asarray(points)
    qn = point_size * 16.0
    assert qn * 8 == int(qn * 8), "point_size: a power of two down to 1/128"
    out = np.full((len(_EXACT_CAMS), H0 * W0), np.iinfo(np.uint64).max, np.uint64)
    stats = [0, 0, 0]
    zbits = {1: 0x3F800000, 2: 0x40000000, 4: 0x40800000}
    for b, ((sxy, _, sz), (tx, ty)) in enumerate(_EXACT_CAMS):
        for m in sel:
            if sz < 0:
                stats[INVALID] += 1
                continue
            z = int(Z[m])
            x8 = 4 * (sxy * int(Xn[m]) + 4 * tx) // z + 164   # 8 x = 8 (32 Xc / Z + 20.5), an integer: Z divides 4
            y8 = 4 * (sxy * int(Yn[m]) + 4 * ty) // z + 92
            assert (4 * (sxy * int(Xn[m]) + 4 * tx)) % z == 0
            px, py = (x8 + 4) >> 3, (y8 + 4) >> 3
            r = min(max_radius, int(qn / z))
            x0, x1, y0, y1 = max(px - r, 0), min(px + r, W0 - 1), max(py - r, 0), min(py + r, H0 - 1)
            if not (-max_radius - 1 <= px <= W0 + max_radius and -max_radius - 1 <= py <= H0 + max_radius) or x0 > x1 or y0 > y1:
                stats[OUTSIDE] += 1
                continue
            stats[DRAWN] += 1
            val = np.uint64((zbits[z] << 32) | (index_base + int(m)))
            for yy in range(y0, y1 + 1):
                seg = out[b, yy * W0 + x0:yy * W0 + x1 + 1]
                np.minimum(seg, val, out=seg)
    return out.view(np.int64).reshape(-1, H0, W0), stats


# ---- seeded cases -------------------------------------------------------------------------------------------------------

# name -> (camera, views, export parameters, point_size, max_radius, index_base)
SEEDED = {
    "pinhole_identity": ("pinhole", 1, dr.identity_params(*dr.HW), 0.3, 2, 0),
    "pinhole_up_crop": ("pinhole", 1, dr.UP_CROP, 0.12, 4, 1000),
    "pinhole_down": ("pinhole", 1, dr.DOWN, 0.5, 2, 0),
    "pinhole_radius0": ("pinhole", 1, dr.UP_CROP, 0.3, 0, 0),
    "pinhole_size0": ("pinhole", 1, dr.UP_CROP, 0.0, 2, 7),
    "mei_up_crop": ("mei", 1, dr.UP_CROP, 0.08, 2, 0),
    "panorama_identity": ("panorama", 1, dr.identity_params(*dr.HW), 0.6, 2, 0),
    "panorama_resize": ("panorama", 1, (dr.HW[0], dr.HW[1], 0, 0, 37, 70), 0.5, 4, 0),
    "rig_two_views": ("pinhole", 2, dr.UP_CROP, 0.08, 2, 0),
}
CASES = list(SEEDED)
_CACHE = {}


def compose_cams(poses, rig, pairs):
    """rows rig[v]^-1 G[p] for (p, v) in `pairs`, composed in float64 and rounded to the float32 rows the kernel is given"""
    rows = []
    for p, v in pairs:
        G = cr._Chain.load(rig[v]).inv() * cr._Chain.load(poses[p])
        rows.append(np.concatenate([G.t, G.q]))
    return np.array(rows, np.float32)


def seeded_case(name, M=1500):
    """-> dict of `cloud_render_ref`'s arguments.  Cameras: three slots of depth_consistency_reference's analytic scene
    (two slots x two views for the rig; the panorama's own scene).  Points: most on the surface those cameras look at (the
    panorama: on its shell), beyond the image on every side and inside the crop band; one in eight behind the cameras or
    within 0.1 of them."""
    camera, V, params, point_size, max_radius, index_base = SEEDED[name]
    rng = np.random.default_rng(len(name) + 17)
    if camera == "panorama":
        sc = cr.panorama_scene()
        d = rng.standard_normal((M, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        s = 1.0 / np.sqrt((d[:, 0] / 5.0) ** 2 + (d[:, 1] / 3.2) ** 2 + (d[:, 2] / 4.1) ** 2)
        pts = d * s[:, None] * rng.uniform(0.15, 1.2, (M, 1))  # ranges of 0.5 to 6: every radius up to the cap
        G0 = cr._Chain.load(sc["poses"][0])  # the first camera: its centre and its axes in the world
        R0 = cr._qmatrix(G0.q)
        c0 = -R0.T @ G0.t
        pole = np.array([0.0, 1.0, 0.0]) + 2e-3 * rng.standard_normal((40, 3)) * [1.0, 0.0, 1.0]
        pts[:40] = c0 + 3.0 * np.where(np.arange(40)[:, None] % 2 == 0, 1.0, -1.0) * (pole @ R0)  # either pole, in and out of the guard
        pts[40:80] = c0 + d[40:80] * rng.uniform(0.07, 0.13, (40, 1))  # either side of the range guard
    else:
        sc = cr.analytic_scene(camera, V=V, seed=sorted(cr.CAMERA_CODE).index(camera) + 3 * V)
        xy = rng.uniform([-2.7, -1.8], [2.7, 1.8], (M, 2))
        pts = np.concatenate([xy, cr.surface_z(xy[:, 0], xy[:, 1])[:, None]], 1)
        pts *= rng.uniform(0.3, 2.2, (M, 1))  # along the rays from the origin: depths of 1 to 10, every radius up to the cap
        k = M // 8
        pts[:k, 2] = rng.uniform(-3.0, 0.3, k)  # behind the cameras and around Z = 0.1
    pairs = [(0, 0), (0, 1), (3, 0), (3, 1)] if V == 2 else [(0, 0), (2, 0), (5, 0)]
    cams = compose_cams(sc["poses"], sc["rig"], pairs)
    intr = np.stack([sc["intrinsics"][v] for _, v in pairs])
    return dict(xyz=pts.astype(np.float32), cams=cams, intrinsics=intr, camera=camera, geom=export_geom(params),
                point_size=point_size, max_radius=max_radius, index_base=index_base)


def cached_case(name):
    """-> (case, reference): computed once per process, shared by the tests, never modified"""
    if name not in _CACHE:
        case = seeded_case(name)
        _CACHE[name] = (case, cloud_render_ref(**case))
    return _CACHE[name]
