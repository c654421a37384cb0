"""Float64 reference, seeded cases and the float32 error bounds of `vipe_depth_consistency` (a helper, not a test module).

Definition (include/vipe_amd.h).  out[n] [H0,W0] uint8 rates the map `vipe_depth_export` makes of disp[rows[n]] [H,W].
Per output pixel, with the taps (iy0, iy1, ly0, ly1), (ix0, ix1, lx0, lx1) of tests/depth_export_reference.py:

    d       = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * e)           the export's blend; d <= 0: the byte is 0
    (u, v)  = (ix0 + lx1, iy0 + ly1)                                           the clamped source coordinate
    ray b   = iproj(intrinsics[view of r], u, v)                               camera.cuh; pinhole / MEI: (X0, Y0, 1)
    for each neighbour row q = nbr[n, k] inside [0, R), q != r:
        T = (rig[vq]^-1 G[pq]) (rig[vr]^-1 G[pr])^-1 = (Rm, t)                 slot p = row // V, view = row % V
        X1      = Rm b + t d
        valid   = X1.z > 0.1 (pinhole, MEI);  |X1| > 0.1 and |(X1.x, X1.z)| > 1e-3 |X1| (panorama)
        (x',y') = proj(intrinsics[vq], X1);  d' = d / X1.z (pinhole, MEI), d / |X1| (panorama)
        visible = valid and 0 <= floor(y') <= H - 2 and (0 <= floor(x') <= W - 2, or - panorama - columns modulo W)
        agrees  = visible and some tap t of disp[q] at (y0 | y0 + 1, x0 | x0 + 1) has t > 0 and |d' - t| <= tol d'
    out = agree_count | visible_count << 4

`axis_taps` evaluates scale, src and the weights in float32 exactly as the kernel does (the convention of
depth_export_reference: they are inputs of the blend, and u, v are exact sums of them); tol and the constants 0.1, 1e-3,
pi are the float32 values the kernel holds.  Everything else is float64, with explicit indexing.

Decided pairs.  Every decision above compares a float32 quantity with a threshold.  For each pair the reference returns
its MARGINS - the distance of x', y' to the nearest integer (floor changes nowhere else, and the visibility borders are
integers; a position that is outside the grid by more than its bound is decided without it), the distance of the
validity quantity to its threshold, | |d' - t| - tol d' | / d' for the taps - and calls the pair DECIDED when every margin
that its decision rests on exceeds the float32 error bound of that quantity.  A decided pair that differs on the GPU is a
finding, not noise.  (The panorama's seam, x' >= W - 0.5 -> x' - W, needs no margin: either side names the columns
W - 1 and 0.)

Error bounds, from the kernel's operation count; u = 2^-24, products and sums rounded one by one (no contraction).
 blend       |dd| <= g4 S (depth_export_reference); a pixel is decided at all when |d| > g4 S or all its taps are <= 0.
 transform   term_transforms of term_geom.cuh on lie_math.h: a quaternion is normalised when loaded (sum of four
             squares 4u, sqrt 1u, reciprocal 1u, product 1u: each component within 5u relative, 5u in 2-norm - the
             float64 reference normalises the same float32 input), an inverse re-normalises (+5u), a product adds its
             operands' errors, 4u per component = 8u in 2-norm for its four-term sums, and 5u for the normalisation
             (+13u).  Rotating p costs (16u + 4 eq) |p| on top of p's own error (about ten roundings on terms below
             3 |p| / 2; |dR(q)/dq| <= 4), a translation sum u (|tA| + |tB|).  `_Chain` carries (eq, et) through the
             five operations of term_transforms; the matrix entries then lie within eR = 4 eq + 8u, t within et.
 ray         pinhole (u - cx) / fx: 2u relative.  MEI: ub, vb 2u; r2 6u; q = sqrt(1 + (1 - k1^2) r2) 6u; factor 15u;
             factor - k1 amplifies that by A = factor / |factor - k1|: (20 + 15 A) u relative.  Panorama: theta within
             5 pi u, phi within 3 pi u (grid offsets, the float32 quotient 2 pi / wd, one product), sinf / cosf within
             2 ulp = 4u: every component within 36u absolute.
 X1          seven roundings: 7u (sum |Rm_ij b_j| + |t_i| d) + eR sum |b_j| + sum |Rm_ij| eb_j + et d + |t_i| dd
 projection  pinhole: 1 / Z, X *, fx *, + cx: fx / Z (dX + |X / Z| dZ) + 3u |fx X / Z| + u |x'|.  MEI: the same with
             rbase = Z + k1 r, dr <= dX + dY + dZ + 4u r, drbase <= dZ + k1 dr + 2u (|Z| + k1 r).  Panorama: atan2f
             within 4 ulp at pi = 16u; x' = atan2(X, Z) fx + c: fx ((dX + dZ) / rho + 16u) + 2 pi u fx + 2u wd, y'
             likewise with drho <= dX + dZ + 3u rho, (drho + dY) / r and ht.
 d'          relative: dd / d + dZ / Z + u (pinhole, MEI), dd / d + dr / r + u (panorama, dr as above)
 tap test    (1 + tol) dd'/d' + u |d' - t| / d' + u tol (the difference and the product tol d' are rounded once each)
 validity    dZ against |Z - 0.1|; dr against |r - 0.1| and drho + 1e-3 dr + 1e-3 u r against |rho - 1e-3 r|
Every bound is doubled: second-order terms of this first-order analysis and the float64 reference's own roundings
(2^-53 against 2^-24) are far below the other half.  At the test sizes ((24, 40) maps, focal lengths near 40 px) the
position bound comes out near 1e-3 px, well under the 3e-3 px at which the undecided share would pass its 2 % cap.
The bounds were written down before the first device run.
"""
import numpy as np

import depth_export_reference as dr

U = 2.0 ** -24
PINHOLE, MEI, PANORAMA = 0, 1, 2
CAMERA_CODE = {"pinhole": PINHOLE, "mei": MEI, "panorama": PANORAMA}
MIN_DEPTH = float(np.float32(0.1))
POLE_EPS = float(np.float32(1e-3))
PI_F = float(np.float32(np.pi))
SAFETY = 2.0
SENTINEL = 0xA5  # what the tests prefill `out` with: a row outside [0, R) keeps it
HW = dr.HW
UP_CROP, DOWN = dr.UP_CROP, dr.DOWN


# ---- SE3 in float64 on rows [tx, ty, tz, qx, qy, qz, qw], with the error bookkeeping of the float32 chain -------------

def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _qact(q, p):
    uv = 2.0 * np.cross(q[:3], p)
    return p + q[3] * uv + np.cross(q[:3], uv)


def _qmatrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


class _Chain:
    """an SE3 element in float64 with bounds (eq, et) on what the float32 chain of lie_math.h has lost on the way"""

    def __init__(self, t, q, et, eq):
        self.t, self.q, self.et, self.eq = t, q, et, eq

    @staticmethod
    def load(row):
        row = np.asarray(row, dtype=np.float64)
        q = row[3:7]
        return _Chain(row[:3].copy(), q / np.linalg.norm(q), 0.0, 5 * U)

    @staticmethod
    def _act_err(eq, pn, ep):
        return (16 * U + 4 * eq) * pn + ep

    def inv(self):
        q = self.q * np.array([-1.0, -1.0, -1.0, 1.0])
        eq = self.eq + 5 * U
        return _Chain(-_qact(q, self.t), q, _Chain._act_err(eq, np.linalg.norm(self.t), self.et), eq)

    def __mul__(self, o):
        q = _qmul(self.q, o.q)
        q = q / np.linalg.norm(q)
        tn, on = np.linalg.norm(self.t), np.linalg.norm(o.t)
        et = self.et + _Chain._act_err(self.eq, on, o.et) + U * (tn + on)
        return _Chain(self.t + _qact(self.q, o.t), q, et, self.eq + o.eq + 13 * U)


def relative_transform(poses, rig, pr, vr, pq, vq):
    """-> (Rm [3,3], t [3], eR, et): T = (rig[vq]^-1 G[pq]) (rig[vr]^-1 G[pr])^-1 in the order term_transforms builds it"""
    Gi, Gj = _Chain.load(poses[pr]), _Chain.load(poses[pq])
    Gij = Gj * Gi.inv()
    T = (_Chain.load(rig[vq]).inv() * Gij) * _Chain.load(rig[vr])
    return _qmatrix(T.q), T.t, 4 * T.eq + 8 * U, T.et


# ---- cameras ------------------------------------------------------------------------------------------------------------

def _ray(camera, K, u, v, H, W):
    """-> (b [3,...], eb [3,...]): the ray of camera.cuh's iproj and its float32 error per component"""
    if camera == PANORAMA:
        theta = ((u + 0.5) - 0.5 * W) * (2.0 * PI_F / W)
        phi = (v + 0.5) * (PI_F / H)
        sp = np.sin(phi)
        b = np.stack([sp * np.sin(theta), -np.cos(phi), sp * np.cos(theta)])
        return b, np.full_like(b, 36 * U)
    fx, fy, cx, cy = (float(x) for x in K[:4])
    ub, vb = (u - cx) / fx, (v - cy) / fy
    if camera == PINHOLE:
        b = np.stack([ub, vb, np.ones_like(ub)])
        return b, np.stack([2 * U * np.abs(ub), 2 * U * np.abs(vb), np.zeros_like(ub)])
    k1 = float(K[4])
    r2 = ub * ub + vb * vb
    q = np.sqrt(1.0 + (1.0 - k1 * k1) * r2)
    factor = (k1 + q) / (1.0 + r2)
    g = factor / (factor - k1)
    rel = (20 + 15 * np.abs(g)) * U
    b = np.stack([ub * g, vb * g, np.ones_like(ub)])
    return b, np.stack([rel * np.abs(b[0]), rel * np.abs(b[1]), np.zeros_like(ub)])


def _project(camera, K, X, dX, H, W):
    """X [3,...] and its error dX -> dict: x, y, ex, ey (positions and their bounds), valid, mvalid (margin / bound of the
    validity decision, > 1 = decided), dq_over_d (d' / d) and edq (relative error of d' without the blend's share)"""
    Xx, Xy, Xz = X
    dx, dy, dz = dX
    with np.errstate(divide="ignore", invalid="ignore"):
        if camera == PANORAMA:
            rho = np.sqrt(Xx * Xx + Xz * Xz)
            r = np.sqrt(rho * rho + Xy * Xy)
            drho = dx + dz + 3 * U * rho
            dr = dx + dy + dz + 4 * U * r
            valid = (r > MIN_DEPTH) & (rho > POLE_EPS * r)
            m1 = np.abs(r - MIN_DEPTH) / (SAFETY * dr)
            m2 = np.abs(rho - POLE_EPS * r) / (SAFETY * (drho + POLE_EPS * dr + POLE_EPS * U * r))
            fx, fy = W / (2.0 * PI_F), H / PI_F
            x = np.arctan2(Xx, Xz) * fx + (0.5 * W - 0.5)
            x = np.where(x >= W - 0.5, x - W, x)
            y = np.arctan2(rho, -Xy) * fy - 0.5
            ex = fx * ((dx + dz) / rho + 16 * U) + 2 * np.pi * U * fx + 2 * U * W
            ey = fy * ((drho + dy) / r + 16 * U) + 2 * np.pi * U * fy + 2 * U * H
            return dict(x=x, y=y, ex=SAFETY * ex, ey=SAFETY * ey, valid=valid, mvalid=np.minimum(m1, m2), scale=1.0 / r,
                        escale=dr / r + U)
        fx, fy, cx, cy = (float(v) for v in K[:4])
        valid = Xz > MIN_DEPTH
        mvalid = np.abs(Xz - MIN_DEPTH) / (SAFETY * dz)
        Z = np.where(Xz < MIN_DEPTH, 1.0, Xz)  # proj's clamp: the position of an invalid point is never used
        if camera == PINHOLE:
            den, dden = Z, dz
        else:
            k1 = float(K[4])
            r = np.sqrt(Xx * Xx + Xy * Xy + Z * Z)
            dr = dx + dy + dz + 4 * U * r
            den = Z + k1 * r
            dden = dz + abs(k1) * dr + 2 * U * (np.abs(Z) + abs(k1) * r)
        px, py = fx * Xx / den, fy * Xy / den
        x, y = px + cx, py + cy
        ex = fx / np.abs(den) * (dx + np.abs(Xx / den) * dden) + 3 * U * np.abs(px) + U * np.abs(x)
        ey = fy / np.abs(den) * (dy + np.abs(Xy / den) * dden) + 3 * U * np.abs(py) + U * np.abs(y)
        return dict(x=x, y=y, ex=SAFETY * ex, ey=SAFETY * ey, valid=valid, mvalid=mvalid, scale=1.0 / Xz,
                    escale=dz / np.abs(Xz) + U)


# ---- the reference ------------------------------------------------------------------------------------------------------

def depth_consistency_ref(disp, poses, rig, intrinsics, camera, params, rows, nbr, tol):
    """-> dict: byte [N,H0,W0] uint8 (0 where nothing is written), written [N] bool (rows[n] inside [0, R)), and per
    (n, k, pixel) pair: active [N,K] (the neighbour entry names a row to test), visible, agree, decided [N,K,H0,W0] bool,
    the margins over their bounds m_valid, m_pos, m_tap [N,K,H0,W0] (inf where a margin does not enter the decision),
    col0 [N,K,H0,W0] (the first tap column of a visible pair, -1 elsewhere),
    undecided [N,H0,W0] (number of the pixel's undecided pairs).  `camera` is a name or a VIPE_CAM_* code."""
    camera = CAMERA_CODE.get(camera, camera)
    disp = np.asarray(disp)
    assert disp.dtype == np.float32 and disp.ndim == 3
    poses, rig = np.asarray(poses, dtype=np.float32), np.asarray(rig, dtype=np.float32)
    intrinsics = np.asarray(intrinsics, dtype=np.float32)
    R, H, W = disp.shape
    V = rig.shape[0]
    h1, w1, top, left, H0, W0 = params
    nbr = np.asarray(nbr, dtype=np.int64)
    N, K = nbr.shape
    rows = np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    tol = float(np.float32(tol))
    y0, y1, ly0, ly1 = dr.axis_taps(h1, H0, top, H)
    x0, x1, lx0, lx1 = dr.axis_taps(w1, W0, left, W)
    wy0, wy1 = ly0.astype(np.float64)[:, None], ly1.astype(np.float64)[:, None]
    wx0, wx1 = lx0.astype(np.float64)[None, :], lx1.astype(np.float64)[None, :]
    u = np.broadcast_to((x0 + lx1.astype(np.float64))[None, :], (H0, W0))
    v = np.broadcast_to((y0 + ly1.astype(np.float64))[:, None], (H0, W0))
    m64 = disp.astype(np.float64)

    out = dict(byte=np.zeros((N, H0, W0), np.uint8), written=np.zeros(N, bool), active=np.zeros((N, K), bool),
               undecided=np.zeros((N, H0, W0), np.int64))
    for name in ("visible", "agree", "decided"):
        out[name] = np.zeros((N, K, H0, W0), bool)
    for name in ("m_valid", "m_pos", "m_tap"):
        out[name] = np.full((N, K, H0, W0), np.inf)
    out["col0"] = np.full((N, K, H0, W0), -1, np.int64)  # the first tap column of a visible pair
    for n in range(N):
        r = int(rows[n])
        if not 0 <= r < R:
            continue
        out["written"][n] = True
        pr, vr = divmod(r, V)
        a, b = m64[r][y0][:, x0], m64[r][y0][:, x1]
        c, e = m64[r][y1][:, x0], m64[r][y1][:, x1]
        d = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * e)
        S = wy0 * (wx0 * np.abs(a) + wx1 * np.abs(b)) + wy1 * (wx0 * np.abs(c) + wx1 * np.abs(e))
        Spos = wy0 * (wx0 * (a > 0) + wx1 * (b > 0)) + wy1 * (wx0 * (c > 0) + wx1 * (e > 0))
        dd = dr.G4 * S
        pos = d > 0
        d_decided = (np.abs(d) > SAFETY * dd) | (Spos == 0)  # no weighted tap is positive: exactly <= 0 on both sides
        dsafe = np.where(pos, d, 1.0)
        ray, eb = _ray(camera, intrinsics[vr], u, v, H, W)
        agree_n, visible_n = np.zeros((H0, W0), np.int64), np.zeros((H0, W0), np.int64)
        for k in range(K):
            q = int(nbr[n, k])
            if not 0 <= q < R or q == r:
                continue
            out["active"][n, k] = True
            pq, vq = divmod(q, V)
            Rm, t, eR, et = relative_transform(poses, rig, pr, vr, pq, vq)
            X = np.stack([Rm[i, 0] * ray[0] + Rm[i, 1] * ray[1] + Rm[i, 2] * ray[2] + t[i] * dsafe for i in range(3)])
            dX = np.stack([7 * U * (np.abs(Rm[i, 0] * ray[0]) + np.abs(Rm[i, 1] * ray[1]) + np.abs(Rm[i, 2] * ray[2])
                                    + np.abs(t[i]) * dsafe)
                           + eR * (np.abs(ray[0]) + np.abs(ray[1]) + np.abs(ray[2]))
                           + np.abs(Rm[i, 0]) * eb[0] + np.abs(Rm[i, 1]) * eb[1] + np.abs(Rm[i, 2]) * eb[2]
                           + et * dsafe + np.abs(t[i]) * dd for i in range(3)])
            P = _project(camera, intrinsics[vq], X, dX, H, W)
            valid = P["valid"] & pos
            x, y, ex, ey = P["x"], P["y"], P["ex"], P["ey"]
            xf, yf = np.floor(x), np.floor(y)
            with np.errstate(invalid="ignore"):
                in_y = (yf >= 0) & (yf <= H - 2)
                in_x = np.ones_like(in_y) if camera == PANORAMA else (xf >= 0) & (xf <= W - 2)
                out_sure = (y < -ey) | (y > H - 1 + ey)
                if camera != PANORAMA:
                    out_sure |= (x < -ex) | (x > W - 1 + ex)
                m_pos = np.minimum(np.abs(x - np.rint(x)) / ex, np.abs(y - np.rint(y)) / ey)
            visible = valid & in_y & in_x
            yi = np.where(visible, yf, 0).astype(np.int64)
            xi = np.where(visible, xf, 0).astype(np.int64)
            c0, c1 = (xi % W, (xi + 1) % W) if camera == PANORAMA else (xi, xi + 1)
            dq = dsafe * P["scale"]
            with np.errstate(divide="ignore", invalid="ignore"):
                e_rel = SAFETY * ((1 + tol) * (dd / dsafe + P["escale"]) + U * tol)
                agree = np.zeros_like(visible)
                sure_yes = np.zeros_like(visible)
                sure_no = np.ones_like(visible)
                m_tap = np.full(visible.shape, np.inf)
                for ty_, tx_ in ((yi, c0), (yi, c1), (yi + 1, c0), (yi + 1, c1)):
                    tv = m64[q][np.minimum(ty_, H - 1), tx_]
                    diff = np.abs(dq - tv) / dq
                    ok = (tv > 0) & (diff <= tol)
                    margin = np.abs(diff - tol) / (e_rel + SAFETY * U * diff)
                    margin = np.where(tv > 0, margin, np.inf)  # a non-positive tap never agrees: exact
                    agree |= ok
                    sure_yes |= ok & (margin > 1)
                    sure_no &= ~ok & (margin > 1)
                    m_tap = np.minimum(m_tap, margin)
            agree &= visible
            taps_sure = sure_yes | sure_no
            valid_sure = P["mvalid"] > 1
            decided = d_decided & (~pos | (valid_sure & (~P["valid"] | out_sure | ((m_pos > 1) & (~visible | taps_sure)))))
            out["visible"][n, k], out["agree"][n, k], out["decided"][n, k] = visible, agree, decided
            out["m_valid"][n, k] = np.where(pos, P["mvalid"], np.inf)
            out["m_pos"][n, k] = np.where(valid & ~out_sure, m_pos, np.inf)
            out["m_tap"][n, k] = np.where(visible, m_tap, np.inf)
            out["col0"][n, k] = np.where(visible, c0, -1)
            agree_n += agree
            visible_n += visible
            out["undecided"][n] += ~decided
        out["byte"][n] = (agree_n | (visible_n << 4)).astype(np.uint8)
    return out


def summary(ref):
    """-> dict of pair counts over the active pairs: total, undecided, and of the decided ones agree / visible but not /
    not visible"""
    act = np.broadcast_to(ref["active"][:, :, None, None], ref["decided"].shape) & ref["written"][:, None, None, None]
    dec = ref["decided"] & act
    return dict(total=int(act.sum()), undecided=int((act & ~ref["decided"]).sum()), agree=int((dec & ref["agree"]).sum()),
                visible_only=int((dec & ref["visible"] & ~ref["agree"]).sum()), hidden=int((dec & ~ref["visible"]).sum()))


def compare(got, ref, sentinel=SENTINEL):
    """the criterion of the device tests: a map whose row is outside [0, R) keeps the sentinel; a pixel whose pairs are all
    decided has the reference's byte; elsewhere each nibble differs by at most the number of the pixel's undecided
    pairs.  -> (number of pixels compared exactly, number compared loosely); raises AssertionError"""
    got = np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == ref["byte"].shape
    for n, w in enumerate(ref["written"]):
        if not w:
            assert (got[n] == sentinel).all(), f"map {n}: its row is out of range, the map must stay untouched"
    wr = ref["written"]
    g, b, und = got[wr].astype(np.int64), ref["byte"][wr].astype(np.int64), ref["undecided"][wr]
    exact = und == 0
    bad = exact & (g != b)
    assert not bad.any(), (f"{int(bad.sum())} decided pixels differ, first at {np.argwhere(bad)[0].tolist()}: "
                           f"got {g[bad][0]:#04x}, reference {b[bad][0]:#04x}")
    loose = ~exact
    assert (np.abs((g & 15) - (b & 15))[loose] <= und[loose]).all(), "agree count beyond the undecided pairs"
    assert (np.abs((g >> 4) - (b >> 4))[loose] <= und[loose]).all(), "visible count beyond the undecided pairs"
    return int(exact.sum()), int(loose.sum())


# ---- scenes -------------------------------------------------------------------------------------------------------------

def _se3_row(t, w):
    """world -> camera row from a translation and a rotation vector (float32, as the buffer holds it)"""
    w = np.asarray(w, dtype=np.float64)
    th = np.linalg.norm(w)
    q = np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]]) if th > 0 else np.array([0, 0, 0, 1.0])
    return np.concatenate([np.asarray(t, dtype=np.float64), q]).astype(np.float32)


def surface_z(x, y):
    return 4.0 + 0.6 * np.sin(0.9 * x) + 0.4 * np.cos(1.1 * y)


def _rays_world(camera, K, pose, H, W):
    """pixel-centre rays of a view (u, v integer) in world coordinates -> (origin [3], dirs [3,H,W], scale [H,W]) where
    disparity = 1 / (s * scale): scale is the ray's z (pinhole, MEI: depth along the axis) or its length (panorama)"""
    uu, vv = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    b, _ = _ray(camera, K, uu, vv, H, W)
    G = _Chain.load(pose)
    Rm = _qmatrix(G.q)  # world -> camera
    dirs = np.einsum("ji,jhw->ihw", Rm, b)  # camera -> world: the transpose
    origin = -Rm.T @ G.t
    scale = np.linalg.norm(b, axis=0) if camera == PANORAMA else b[2]
    return origin, dirs, scale


def raycast_disps(camera, intrinsics, poses, rig, H, W, surface=surface_z):
    """disparities [P*V,H,W] float32 of the surface z = surface(x, y) seen from every (slot, view): the root of
    o.z + s dir.z = surface(o + s dir) by bisection on s in (0, 40] (the surface lies in front of every test camera and
    every ray crosses it once there; rays that do not reach it get disparity 0)"""
    P, V = poses.shape[0], rig.shape[0]
    out = np.zeros((P * V, H, W), np.float32)
    for p in range(P):
        for vw in range(V):
            G = _Chain.load(rig[vw]).inv() * _Chain.load(poses[p])
            pose = np.concatenate([G.t, G.q])
            o, dirs, scale = _rays_world(camera, intrinsics[vw], pose, H, W)
            f = lambda s: o[2] + s * dirs[2] - surface(o[0] + s * dirs[0], o[1] + s * dirs[1])
            lo, hi = np.full((H, W), 1e-6), np.full((H, W), 40.0)
            hit = (f(lo) < 0) & (f(hi) > 0)
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                neg = f(mid) < 0
                lo, hi = np.where(neg, mid, lo), np.where(neg, hi, mid)
            s = 0.5 * (lo + hi)
            with np.errstate(divide="ignore"):
                out[p * V + vw] = np.where(hit & (s * scale > 0), 1.0 / (s * scale), 0.0).astype(np.float32)
    return out


def analytic_scene(camera="pinhole", V=1, P=6, H=HW[0], W=HW[1], seed=0):
    """six slots looking at the surface: baselines of about 0.25 units, rotations of about 0.03 rad, irrational enough
    that no pair has a zero baseline or an integer pixel shift -> dict(disp, poses, rig, intrinsics, camera)"""
    rng = np.random.default_rng(seed)
    poses = np.stack([_se3_row([0.25 * (p - 2.3) + 0.03 * rng.standard_normal(), 0.11 * np.sin(1.7 * p) + 0.02, 0.07 * np.cos(p)],
                               0.03 * rng.standard_normal(3) + 1e-3) for p in range(P)])
    rig = np.stack([_se3_row([0, 0, 0], [0, 0, 0])] + [_se3_row([0.21 * v, 0.013, -0.017], [0.011, -0.04 * v, 0.007])
                                                       for v in range(1, V)])
    if camera == "panorama":
        intr = np.zeros((V, 4), np.float32)
    else:
        f = 1.05 * W
        intr = np.stack([np.array([f * (1 + 0.02 * v), f * (1 - 0.01 * v), W / 2 - 0.37 + v, H / 2 + 0.29 - v]
                                  + ([0.35 + 0.05 * v] if camera == "mei" else []), dtype=np.float32) for v in range(V)])
        if camera == "mei":  # the pinhole-equivalent focal length is f / (1 + k1)
            intr[:, :2] *= 1 + intr[:, 4:5]
    code = CAMERA_CODE[camera]
    disp = raycast_disps(code, intr, poses, rig, H, W)
    return dict(disp=disp, poses=poses.astype(np.float32), rig=rig.astype(np.float32), intrinsics=intr, camera=camera)


def corrupt(disp, row, rect, factor=1.4):
    """a copy with disp[row] multiplied by `factor` inside rect = (y0, y1, x0, x1)"""
    out = disp.copy()
    y0, y1, x0, x1 = rect
    out[row, y0:y1, x0:x1] *= np.float32(factor)
    return out


def seeded_case(name):
    """the cases of tests/test_gpu_depth_consistency.py and of the CPU caps test -> dict(disp, poses, rig, intrinsics,
    camera, params, rows, nbr, tol).  The scene is `analytic_scene`; about a third of one neighbour map per case is
    corrupted (x 1.4 on a rectangle, 4 % noise elsewhere on it) so that every branch - agree, visible without
    agreement, not visible - is taken by at least 5 % of the pairs."""
    camera, V, params, K = {
        "pinhole_identity": ("pinhole", 1, dr.identity_params(*HW), 4),
        "pinhole_up_crop": ("pinhole", 1, UP_CROP, 4),
        "pinhole_down": ("pinhole", 1, DOWN, 4),
        "mei_identity": ("mei", 1, dr.identity_params(*HW), 4),
        "mei_up_crop": ("mei", 1, UP_CROP, 4),
        "panorama_identity": ("panorama", 1, dr.identity_params(*HW), 4),
        "panorama_resize": ("panorama", 1, (HW[0], HW[1], 0, 0, 37, 83), 4),
        "rig_two_views": ("pinhole", 2, UP_CROP, 4),
        "k1": ("pinhole", 1, dr.identity_params(*HW), 1),
        "k8": ("pinhole", 1, UP_CROP, 8),
        "edge_entries": ("pinhole", 1, UP_CROP, 4),
    }[name]
    sc = analytic_scene(camera, V=V, seed=sorted(CAMERA_CODE).index(camera) + 3 * V)
    if camera == "panorama":  # the whole sphere: a shell around the cameras instead of the surface in front of them
        sc = panorama_scene()
    disp, P = sc["disp"], sc["poses"].shape[0]
    R = P * V
    rng = np.random.default_rng(len(name))
    H, W = HW
    for row in (1 * V, 4 * V):  # two neighbour maps: a scaled rectangle and noise on the rest
        noise = (1 + 0.04 * rng.standard_normal((H, W))).astype(np.float32)
        disp[row] *= noise
        disp[row, 3:19, 6:30] *= np.float32(1.4)
    if name == "edge_entries":
        disp[2, 5:9, :] = 0.0          # zero and negative neighbour taps
        disp[2, 12:15, 10:20] *= -1.0
        disp[0, 0:6, 0:10] = 0.0       # d <= 0 source pixels (whole tap neighbourhoods)
        disp[3, 10:, 25:] *= -1.0
        rows = np.array([0, 3, 3, -1, 5, R, 2], dtype=np.int64)   # repeats, -1 and R keep the sentinel
        nbr = np.array([[1, 2, -1, 4], [3, 2, R, 4], [0, 1, 2, 5], [0, 1, 2, 3], [5, 5, 4, -7], [0, 1, 2, 3], [0, 1, 3, 4]],
                       dtype=np.int64)  # none, out of range, q == r
    else:
        rows = None if name in ("pinhole_identity", "k1") else np.arange(R, dtype=np.int64)[::-1].copy()
        src = np.arange(R) if rows is None else rows
        nbr = np.full((R, K), -1, dtype=np.int64)
        for i, r in enumerate(src):  # same-view rows of the other slots, nearest slot first
            slot, view = divmod(int(r), V)
            others = sorted((abs(p - slot), p) for p in range(P) if p != slot)
            for k, (_, p) in enumerate(others[:K]):
                nbr[i, k] = p * V + view
            if K == 8:  # more entries than other slots: the rest stays -1 and two repeat a neighbour
                nbr[i, 5], nbr[i, 6] = nbr[i, 0], nbr[i, 1]
    return dict(disp=disp, poses=sc["poses"], rig=sc["rig"], intrinsics=sc["intrinsics"], camera=camera, params=params,
                rows=rows, nbr=nbr, tol=0.05)


def panorama_scene(P=6, H=HW[0], W=HW[1]):
    """cameras inside the ellipsoid shell |(x / 5, y / 3.2, z / 4.1)| = 1, ranges by bisection: neighbours project across the
    seam (the cameras are yawed apart) and the first and last rows look at the poles"""
    poses = np.stack([_se3_row([0.25 * (p - 2.3), 0.09 * np.sin(1.7 * p) + 0.02, 0.12 * np.cos(p)],
                               [0.013 * p, 0.03 * (p - 2) + 1e-3, -0.021]) for p in range(P)])
    rig = np.stack([_se3_row([0, 0, 0], [0, 0, 0])])
    intr = np.zeros((1, 4), np.float32)
    out = np.zeros((P, H, W), np.float32)
    for p in range(P):
        o, dirs, scale = _rays_world(PANORAMA, intr[0], poses[p].astype(np.float64), H, W)
        f = lambda s: ((o[0] + s * dirs[0]) / 5.0) ** 2 + ((o[1] + s * dirs[1]) / 3.2) ** 2 + ((o[2] + s * dirs[2]) / 4.1) ** 2 - 1
        lo, hi = np.zeros((H, W)), np.full((H, W), 20.0)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            neg = f(mid) < 0
            lo, hi = np.where(neg, mid, lo), np.where(neg, hi, mid)
        out[p] = (1.0 / (0.5 * (lo + hi) * scale)).astype(np.float32)
    return dict(disp=out, poses=poses.astype(np.float32), rig=rig.astype(np.float32), intrinsics=intr, camera="panorama")


CASES = ["pinhole_identity", "pinhole_up_crop", "pinhole_down", "mei_identity", "mei_up_crop", "panorama_identity",
         "panorama_resize", "rig_two_views", "k1", "k8", "edge_entries"]

_CACHE = {}


def cached_case(name):
    """-> (case, reference): computed once per process, shared by the tests, never modified"""
    if name not in _CACHE:
        case = seeded_case(name)
        _CACHE[name] = (case, depth_consistency_ref(**case))
    return _CACHE[name]
