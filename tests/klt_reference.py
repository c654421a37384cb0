"""Float64 restatement, seeded inputs and error bounds of the sparse tracker kernels `vipe_klt_pyramid`,
`vipe_klt_detect` and `vipe_klt_track` (a helper, not a test module).  include/vipe_amd.h states the arithmetic; every
function here takes `dt`: np.float64 is the reference, np.float32 runs the very same statements in the kernel's precision
(numpy's own summation order), which is what `TRACK_BOUND` is measured with.

Inputs: an analytic texture (a sum of 40 sinusoids below 0.35 cycles / pixel) evaluated at warped coordinates, so every
frame is exact and the true position of every point in every frame is known."""
import numpy as np

EPS32 = 2.0 ** -23
OOB, LOW_TEXTURE, RESIDUAL, FB, MASKED, DIVERGED = 1, 2, 4, 8, 16, 32
SENTINEL = -12345.0

# ---- bounds, counted from the operations (u = EPS32 / 2 per rounding) --------------------------------------------------
# Pyramid, |level - ref| <= pyramid_c(l) * EPS32 * 255.  Level 0: three products and two sums of values <= 255 (five
# roundings, 2.5 EPS32 * 255), one more product for float input (3 EPS32).  A binomial pass: (p0 + p4), (p1 + p3), the sum
# of the two (<= 10 * 255), 6 * p2, the last sum (<= 16 * 255) - five roundings of values <= 16 * 255, scaled by 1/16
# (exact): 2.5 EPS32 * 255; the weights sum to one, so the error of the inputs passes through unamplified.  Two passes
# per level: 5 EPS32 * 255.
def pyramid_c(level):
    return 3 + 5 * level


# Corner response, |resp - ref| <= RESPONSE_C * EPS32 * (a + c).  A gradient is one subtraction of exact values (relative
# u; the halving is exact), a product of two gradients 3u, a sum of 25 terms in any order at most 24 u of the sum of the
# magnitudes: a, c carry 27 u = 13.5 EPS32 relative, b 13.5 EPS32 * (a + c) / 2 (|gx gy| <= (gx^2 + gy^2) / 2).  The
# smaller eigenvalue moves by at most the Frobenius norm of the perturbation <= |da| + |dc| + 2 |db| <= 27 EPS32 (a + c).
# The closed form adds (a + c), (a - c), two squares, their sum, the root and the final difference: seven roundings of
# values <= (a + c), 3.5 EPS32 (a + c).  Rounded up to the next power of two.
RESPONSE_C = 32

# Tracked positions: 16 x the largest float32-against-float64 difference of THIS module over `track_cases()` (the factor
# covers another summation order and the differently associated bilinear weights); tests/test_klt_reference.py recomputes
# it.  An input for which it exceeds 0.01 px is ill-conditioned and gets replaced, not tolerated.
TRACK_BOUND = 16 * 1.2e-5  # measured: 1.13e-5 px
TRACK_BOUND_LIMIT = 0.01

GRAY = (np.float32(0.299), np.float32(0.587), np.float32(0.114))  # the kernel's f32 constants, exactly


# ---- inputs -------------------------------------------------------------------------------------------------------------
class Texture:
    """sum of `n` sinusoids, frequencies in [0.02, 0.35) cycles / pixel, amplitude ~ 1 / f, mapped to 0-255 (clipped at
    three standard deviations); callable at any real coordinates"""

    def __init__(self, seed=0, n=40):
        rng = np.random.default_rng(seed)
        f = rng.uniform(0.02, 0.35, n)
        th = rng.uniform(0.0, 2 * np.pi, n)
        self.fx, self.fy = f * np.cos(th), f * np.sin(th)
        self.ph = rng.uniform(0.0, 2 * np.pi, n)
        self.amp = 1.0 / (f + 0.05)
        self.sigma = np.sqrt(0.5 * np.sum(self.amp ** 2))

    def __call__(self, x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        s = np.zeros(np.broadcast(x, y).shape)
        for fx, fy, ph, a in zip(self.fx, self.fy, self.ph, self.amp):
            s += a * np.cos(2 * np.pi * (fx * x + fy * y) + ph)
        return np.clip(127.5 + 127.5 * s / (3 * self.sigma), 0.0, 255.0)


class Warp:
    """p -> centre + scale * R(angle) (p - centre) + t: translation (3.3, -2.6) px, 1 degree, 1 % per step"""

    def __init__(self, H, W, steps=1.0, t=(3.3, -2.6), angle_deg=1.0, scale=1.01):
        self.c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
        a, s = np.deg2rad(angle_deg * steps), scale ** steps
        self.M = s * np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        self.t = np.asarray(t, np.float64) * steps

    def forward(self, pts):
        return (np.asarray(pts, np.float64) - self.c) @ self.M.T + self.c + self.t

    def inverse(self, pts):
        return (np.asarray(pts, np.float64) - self.c - self.t) @ np.linalg.inv(self.M).T + self.c


def render(tex, H, W, warp=None, dtype=np.float32):
    """the texture seen through `warp` -> rgb [H,W,3]: float32 in 0-1, or uint8 (rounded)"""
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    p = np.stack([xx, yy], -1).reshape(-1, 2)
    if warp is not None:
        p = warp.inverse(p)
    g = tex(p[:, 0], p[:, 1]).reshape(H, W)
    if dtype == np.uint8:
        return np.repeat(np.rint(g).astype(np.uint8)[..., None], 3, -1)
    return np.repeat((g / 255.0).astype(np.float32)[..., None], 3, -1)


def lattice(H, W, step=8, first=16, offset=0.25):
    """points on a `step` lattice from `first` to H - first / W - first, offset by `offset` (96 x 128: 9 x 13 = 117)"""
    ys, xs = np.arange(first, H - first + 1, step), np.arange(first, W - first + 1, step)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel()], -1).astype(np.float64) + offset


def make_pair(H=96, W=128, seed=0, dtype=np.float32):
    """-> (rgb_a, rgb_b, warp): the texture and the texture through one step of the warp"""
    tex, warp = Texture(seed), Warp(H, W)
    return render(tex, H, W, None, dtype), render(tex, H, W, warp, dtype), warp


def make_sequence(T=6, H=96, W=128, seed=0, dtype=np.float32):
    """-> ([rgb_k], [warp_k]): frame k sees the texture through k steps of the warp"""
    tex = Texture(seed)
    warps = [Warp(H, W, steps=k) for k in range(T)]
    return [render(tex, H, W, w, dtype) for w in warps], warps


# ---- the arithmetic -----------------------------------------------------------------------------------------------------
def pyramid_sizes(H, W, levels):
    sizes = []
    for _ in range(levels):
        sizes.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return sizes


def _binom5(p0, p1, p2, p3, p4, dt):
    return (((p0 + p4) + dt(4) * (p1 + p3)) + dt(6) * p2) * dt(0.0625)


def pyramid_ref(rgb, levels, dt=np.float64):
    """rgb [H,W,3] uint8 / float32 -> list of `levels` arrays of dtype dt"""
    c = rgb.astype(dt)
    g = (dt(GRAY[0]) * c[..., 0] + dt(GRAY[1]) * c[..., 1]) + dt(GRAY[2]) * c[..., 2]
    if rgb.dtype != np.uint8:
        g = g * dt(255)
    out = [g]
    for _ in range(1, levels):
        src = out[-1]
        h, w = src.shape
        h2, w2 = (h + 1) // 2, (w + 1) // 2
        xs = [np.clip(2 * np.arange(w2) + k - 2, 0, w - 1) for k in range(5)]
        ys = [np.clip(2 * np.arange(h2) + k - 2, 0, h - 1) for k in range(5)]
        t = _binom5(*[src[:, x] for x in xs], dt)  # rows first: [h, w2]
        out.append(_binom5(*[t[y] for y in ys], dt))
    return out


def flatten(pyr):
    return np.concatenate([p.ravel() for p in pyr])


def _lambda_min(a, b, c, dt):
    hd = dt(0.5) * (a - c)
    return dt(0.5) * (a + c) - np.sqrt(hd * hd + b * b)


def response_ref(img, dt=np.float64):
    """-> (response [H,W], a + c [H,W]) of the 5 x 5 structure tensor, zero outside the image"""
    img = img.astype(dt)
    H, W = img.shape
    xi, yi = np.arange(W), np.arange(H)
    gx = dt(0.5) * (img[:, np.minimum(xi + 1, W - 1)] - img[:, np.maximum(xi - 1, 0)])
    gy = dt(0.5) * (img[np.minimum(yi + 1, H - 1)] - img[np.maximum(yi - 1, 0)])
    sums = []
    for prod in (gx * gx, gx * gy, gy * gy):
        pad = np.zeros((H + 4, W + 4), dt)
        pad[2:-2, 2:-2] = prod
        s = np.zeros((H, W), dt)
        for dy in range(5):
            for dx in range(5):
                s = s + pad[dy:dy + H, dx:dx + W]
        sums.append(s)
    a, b, c = sums
    return _lambda_min(a, b, c, dt), a + c


def detect_ref(img, cell, border, min_eig, mask=None, busy=None, dt=np.float64):
    """-> (out [ncy*ncx,3] (x, y, response) or (-1, -1, 0), clear [ncy*ncx] bool).  `clear` is False where the deciding
    quantity lies within its bound of a tie or of the threshold: another pixel whose response, each taken at the
    favourable end of its bound, reaches the winner's, or a contender within its bound of `min_eig`."""
    resp, apc = response_ref(img, dt)
    H, W = resp.shape
    ncx, ncy = -(-W // cell), -(-H // cell)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    elig = (xx >= border) & (xx <= W - 1 - border) & (yy >= border) & (yy <= H - 1 - border)
    if mask is not None:
        elig &= np.asarray(mask) != 0
    bound = RESPONSE_C * EPS32 * apc.astype(np.float64)
    out = np.zeros((ncy * ncx, 3), dt)
    out[:, :2] = -1
    clear = np.ones(ncy * ncx, bool)
    for cid in range(ncy * ncx):
        if busy is not None and busy[cid]:
            continue
        sl = (slice((cid // ncx) * cell, (cid // ncx + 1) * cell), slice((cid % ncx) * cell, (cid % ncx + 1) * cell))
        r, e, bd = resp[sl], elig[sl], bound[sl]
        r64 = r.astype(np.float64)
        qual = e & (r / dt(25) >= dt(min_eig))
        if not qual.any():
            clear[cid] = not (e & (np.abs(r64 / 25 - min_eig) <= bd / 25)).any()
            continue
        best = np.where(qual, r, -np.inf)
        k = int(np.argmax(best))  # first occurrence of the maximum in row-major order: lowest row, then lowest column
        py, px = divmod(k, r.shape[1])
        out[cid] = (sl[1].start + px, sl[0].start + py, r[py, px])
        contenders = e & (r64 + bd >= r64[py, px] - bd[py, px]) & ((r64 + bd) / 25 >= min_eig)
        clear[cid] = contenders.sum() == 1 and abs(r64[py, px] / 25 - min_eig) > bd[py, px] / 25
    return out, clear


def _sample(img, x, y, dt):
    h, w = img.shape
    flx, fly = np.floor(x), np.floor(y)
    fx, fy = x - flx, y - fly
    xi = np.clip(np.nan_to_num(flx, nan=-1.0), -1, w).astype(np.int64)
    yi = np.clip(np.nan_to_num(fly, nan=-1.0), -1, h).astype(np.int64)
    xa, xb = np.clip(xi, 0, w - 1), np.clip(xi + 1, 0, w - 1)
    ya, yb = np.clip(yi, 0, h - 1), np.clip(yi + 1, 0, h - 1)
    v00, v01, v10, v11 = img[ya, xa], img[ya, xb], img[yb, xa], img[yb, xb]
    top, bot = v00 + fx * (v01 - v00), v10 + fx * (v11 - v10)
    return top + fy * (bot - top)


def _inside(x, y, b, w, h):
    with np.errstate(invalid="ignore"):
        return (x >= b) & (x <= (w - 1) - b) & (y >= b) & (y <= (h - 1) - b)


def _edge_margin(x, y, b, w, h):
    """distance of (x, y) to the nearest of the four limits of `_inside`"""
    return np.minimum(np.minimum(np.abs(x - b), np.abs((w - 1) - b - x)), np.minimum(np.abs(y - b), np.abs((h - 1) - b - y)))


def track_ref(pyr_a, pyr_b, pts, *, win_radius, n_iters, eps, border, min_eig, max_residual, fb_thresh, max_flow, mask=None,
              fb_ref=None, status=None, cell=0, n_cells=0, dt=np.float64, bound=None):
    """One pass of `vipe_klt_track` over lists of level arrays -> dict(out [N,2], status [N] uint8, resid [N],
    busy [n_cells] uint8 (backward pass with cell > 0) or None, clear [N] bool).  `clear` (meaningful for dt = float64) is
    False where a deciding quantity lies within its bound of its threshold; `bound` is the position bound (TRACK_BOUND,
    for the backward pass the caller's accumulated one)."""
    bound = TRACK_BOUND if bound is None else bound
    pyr_a, pyr_b = [p.astype(dt) for p in pyr_a], [p.astype(dt) for p in pyr_b]
    L = len(pyr_a)
    H, W = pyr_a[0].shape
    p = np.asarray(pts).astype(dt).reshape(-1, 2)
    N = p.shape[0]
    r = win_radius
    side = 2 * r + 1
    nwin = side * side
    oy, ox = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij")
    ox, oy = ox.ravel().astype(dt)[None], oy.ravel().astype(dt)[None]
    px, py = p[:, 0:1], p[:, 1:2]
    dx, dy = np.zeros((N, 1), dt), np.zeros((N, 1), dt)
    oob = np.zeros(N, bool)
    margin = np.full(N, np.inf)
    one = dt(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for l in range(L - 1, -1, -1):
            scale = dt(1.0 / (1 << l))
            cx, cy = px * scale, py * scale
            A, B = pyr_a[l], pyr_b[l]
            h, w = A.shape
            sx, sy = cx + ox, cy + oy
            tI = _sample(A, sx, sy, dt)
            tx = dt(0.5) * (_sample(A, sx + one, sy, dt) - _sample(A, sx - one, sy, dt))
            ty = dt(0.5) * (_sample(A, sx, sy + one, dt) - _sample(A, sx, sy - one, dt))
            ga, gb, gc = [(u * v).sum(1, keepdims=True, dtype=dt) for u, v in ((tx, tx), (tx, ty), (ty, ty))]
            det = ga * gc - gb * gb
            active = np.ones((N, 1), bool)
            for _ in range(n_iters):
                e = tI - _sample(B, (cx + dx) + ox, (cy + dy) + oy, dt)
                bx, by = (e * tx).sum(1, keepdims=True, dtype=dt), (e * ty).sum(1, keepdims=True, dtype=dt)
                ok = det > 0
                sdet = np.where(ok, det, one)
                ux = np.where(ok & active, (gc * bx - gb * by) / sdet, dt(0))
                uy = np.where(ok & active, (ga * by - gb * bx) / sdet, dt(0))
                dx, dy = dx + ux, dy + uy
                if eps > 0:
                    active = active & ~(ux * ux + uy * uy < dt(eps) * dt(eps))
                    if not active.any():
                        break
            bl = dt(border) * scale
            qx, qy = cx + dx, cy + dy
            oob |= ~(_inside(cx, cy, bl, w, h) & _inside(qx, qy, bl, w, h))[:, 0]
            m = _edge_margin(qx, qy, bl, w, h)[:, 0].astype(np.float64)  # c = p * 2^-l and its test are exact
            margin = np.minimum(margin, np.where(np.isfinite(m), m, 0.0) / bound)
            if l > 0:
                dx, dy = dx * dt(2), dy * dt(2)
        qx, qy = px + dx, py + dy
        res = np.abs(tI - _sample(pyr_b[0], qx + ox, qy + oy, dt)).sum(1, dtype=dt) / dt(nwin)
        lam = (_lambda_min(ga, gb, gc, dt) / dt(nwin))[:, 0]
        d2 = (dx * dx + dy * dy)[:, 0]
        out = np.concatenate([qx, qy], 1)
        busy = None
        if fb_ref is None:
            st = np.where(oob, OOB, 0)
            st |= np.where(lam < dt(min_eig), LOW_TEXTURE, 0)
            st |= np.where(res > dt(max_residual), RESIDUAL, 0)
            st |= np.where(~np.isfinite(d2) | (d2 > dt(max_flow) * dt(max_flow)), DIVERGED, 0)
            # margins of the four decisions, each as a multiple of its own bound
            apc = (ga + gc)[:, 0].astype(np.float64)
            delta = 4 * EPS32 * 255.0  # a bilinear sample: four roundings of values <= 255
            lt_bound = (64 * EPS32 * apc + 4 * delta * np.sqrt(nwin * apc)) / nwin + 1e-30
            margin = np.minimum(margin, np.abs(lam.astype(np.float64) - min_eig) / lt_bound)
            b0 = pyr_b[0].astype(np.float64)
            gmax = 2.0 * max(np.abs(np.diff(b0, axis=0)).max(), np.abs(np.diff(b0, axis=1)).max())
            margin = np.minimum(margin, np.abs(res.astype(np.float64) - max_residual) / (bound * gmax + 16 * EPS32 * 255.0))
            margin = np.minimum(margin, np.abs(np.sqrt(d2.astype(np.float64)) - max_flow) / bound)
            if mask is not None:
                rx, ry = np.floor(qx[:, 0] + dt(0.5)), np.floor(qy[:, 0] + dt(0.5))
                inimg = (rx >= 0) & (rx <= W - 1) & (ry >= 0) & (ry <= H - 1)
                ix, iy = np.where(inimg, rx, 0).astype(np.int64), np.where(inimg, ry, 0).astype(np.int64)
                st |= np.where(inimg & (np.asarray(mask)[iy, ix] == 0), MASKED, 0)
                m64 = np.pad(np.asarray(mask) != 0, 1, constant_values=True)  # outside the image nothing is masked
                for sx_ in (-bound, bound):  # unclear where q moved by its bound rounds to a pixel of another mask value
                    for sy_ in (-bound, bound):
                        jx = np.clip(np.floor(np.nan_to_num(qx[:, 0].astype(np.float64)) + sx_ + 0.5), -1, W).astype(np.int64)
                        jy = np.clip(np.floor(np.nan_to_num(qy[:, 0].astype(np.float64)) + sy_ + 0.5), -1, H).astype(np.int64)
                        here = m64[np.clip(iy, 0, H - 1) + 1, np.clip(ix, 0, W - 1) + 1] | ~inimg
                        margin = np.where(m64[jy + 1, jx + 1] != here, 0.0, margin)
            st = st.astype(np.uint8)
        else:
            ref = np.asarray(fb_ref).astype(dt).reshape(-1, 2)
            ex, ey = qx[:, 0] - ref[:, 0], qy[:, 0] - ref[:, 1]
            dist2 = ex * ex + ey * ey
            st = np.asarray(status).astype(np.int64) | np.where(~(dist2 <= dt(fb_thresh) * dt(fb_thresh)), FB, 0)
            st = st.astype(np.uint8)
            margin = np.abs(np.sqrt(dist2.astype(np.float64)) - fb_thresh) / (2 * bound)
            if cell > 0:
                busy = np.zeros(n_cells, np.uint8)
                ix = np.clip(np.floor(p[:, 0] + dt(0.5)), 0, W - 1).astype(np.int64)
                iy = np.clip(np.floor(p[:, 1] + dt(0.5)), 0, H - 1).astype(np.int64)
                keep = st == 0
                busy[(iy[keep] // cell) * (-(-W // cell)) + ix[keep] // cell] = 1
        clear = np.nan_to_num(margin, nan=0.0) > 1.0
    return dict(out=out, status=st, resid=res, busy=busy, clear=clear)


def track_fb_ref(pyr_a, pyr_b, pts, params, mask=None, cell=0, dt=np.float64, bound=None):
    """forward, then backward with the status step -> dict(out, status, resid, busy, clear, back)"""
    H, W = pyr_a[0].shape
    n_cells = (-(-H // cell)) * (-(-W // cell)) if cell else 0
    f = track_ref(pyr_a, pyr_b, pts, mask=mask, dt=dt, bound=bound, **params)
    b = track_ref(pyr_b, pyr_a, f["out"], fb_ref=pts, status=f["status"], cell=cell, n_cells=n_cells, dt=dt, bound=bound,
                  **params)
    return dict(out=f["out"], status=b["status"], resid=f["resid"], busy=b["busy"], clear=f["clear"] & b["clear"],
                back=b["out"])


# ---- the cases the device tests run, shared so that TRACK_BOUND is measured on exactly them ----------------------------
def track_params(r=4, **kw):
    """KLTSparseTracks' defaults, with eps = 0 (exactly n_iters iterations per level: the form the parity tests use)"""
    p = dict(win_radius=r, n_iters=10, eps=0.0, border=8, min_eig=4.0, max_residual=12.0, fb_thresh=0.5, max_flow=64.0)
    p.update(kw)
    return p


DETECT_CASES = [(96, 128, 16), (90, 130, 16), (72, 104, 8)]  # (H, W, cell): whole cells, ragged last cells, small cells
_CACHE = {}


def pair_pyramids(H=96, W=128, levels=3, seed=0, dtype=np.float32):
    """-> (rgb_a, rgb_b, warp, pyr_a, pyr_b) with float64 pyramids, computed once"""
    key = (H, W, levels, seed, np.dtype(dtype).name)
    if key not in _CACHE:
        a, b, warp = make_pair(H, W, seed, dtype)
        _CACHE[key] = (a, b, warp, rounded(pyramid_ref(a, levels)), rounded(pyramid_ref(b, levels)))
    return _CACHE[key]


def rounded(pyr):
    """the levels rounded to float32: what the device tests hand to the kernel AND to the float64 reference, so both
    start from the same numbers"""
    return [p.astype(np.float32) for p in pyr]


FLAT_RECT = (28, 58, 16, 48)        # rows, columns painted flat (gray 100) in BOTH frames: LOW_TEXTURE
UNRELATED_RECT = (60, 90, 64, 100)  # replaced by another texture in the SECOND frame only: RESIDUAL or FB
MASK_STRIP = (0, 96, 106, 112)      # not usable in the second frame: MASKED at the destination


def status_case(levels=3):
    """-> (pyr_a, pyr_b (float32 levels), pts, mask [H,W] uint8 of the second frame, params): points on a 6-pixel lattice
    from 6 px inside the frame, so the outer ring lies within border + 2 px of every edge"""
    if "status" not in _CACHE:
        H, W = 96, 128
        a, b, _ = make_pair(H, W)
        a, b = a.copy(), b.copy()
        y0, y1, x0, x1 = FLAT_RECT
        a[y0:y1, x0:x1] = b[y0:y1, x0:x1] = np.float32(100.0 / 255.0)
        y0, y1, x0, x1 = UNRELATED_RECT
        b[y0:y1, x0:x1] = render(Texture(seed=9), H, W)[y0:y1, x0:x1]
        mask = np.ones((H, W), np.uint8)
        y0, y1, x0, x1 = MASK_STRIP
        mask[y0:y1, x0:x1] = 0
        pts = lattice(H, W, step=6, first=6)
        _CACHE["status"] = (rounded(pyramid_ref(a, levels)), rounded(pyramid_ref(b, levels)), pts, mask, track_params(4))
    return _CACHE["status"]


def point_bounds(pyr_a, pyr_b, pts, params, mask=None):
    """per point max(TRACK_BOUND, 16 x |float32 - float64| of the reference's forward and backward results): where the
    iteration does not settle (a window on unrelated texture) the reference's own two precisions drift apart, and a
    decision that hangs on such a position is not clear"""
    r64 = track_fb_ref(pyr_a, pyr_b, pts, params, mask)
    r32 = track_fb_ref(pyr_a, pyr_b, pts, params, mask, dt=np.float32)
    with np.errstate(invalid="ignore"):
        d = np.maximum(np.abs(r32["out"].astype(np.float64) - r64["out"]).max(1),
                       np.abs(r32["back"].astype(np.float64) - r64["back"]).max(1))
    return np.maximum(TRACK_BOUND, 16 * np.nan_to_num(d, nan=np.inf))


def many_points(n=300, H=96, W=128, seed=3):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(16, W - 17, n), rng.uniform(16, H - 17, n)], -1)


def track_cases():
    """[(name, pts, params)] on `pair_pyramids()`: the lattice at r = 2, 4, 7, one point, 300 points"""
    lat = lattice(96, 128)
    return [("r2", lat, track_params(2)), ("r4", lat, track_params(4)), ("r7", lat, track_params(7)),
            ("n1", lat[58:59], track_params(4)), ("n300", many_points(), track_params(4))]


def measure_track_bound():
    """16 x the largest float32-against-float64 difference of the reference's forward result over `track_cases()`
    (points the float64 run flags are left out: their positions are not compared anywhere)"""
    _, _, _, pa, pb = pair_pyramids()
    worst = 0.0
    for _, pts, prm in track_cases():
        r64 = track_ref(pa, pb, pts, dt=np.float64, **prm)
        r32 = track_ref(pa, pb, pts, dt=np.float32, **prm)
        ok = r64["status"] == 0
        worst = max(worst, float(np.abs(r32["out"].astype(np.float64) - r64["out"])[ok].max()))
    return 16 * worst


# ---- the numpy reference behind the interface of vipe_amd.ext.klt_ext (KLTSparseTracks(_kernels=...)) ------------------
class NumpyKernels:
    """`pyramid`, `detect`, `track` with klt_ext's signatures on CPU torch tensors, computed by the float64 reference.
    `excluded` counts the decisions that were not clear, `decisions` all of them."""

    def __init__(self, dt=np.float64):
        self.dt, self.excluded, self.decisions = dt, 0, 0

    @staticmethod
    def _levels(pyr, H, W, levels):
        out, off = [], 0
        for h, w in pyramid_sizes(H, W, levels):
            out.append(pyr[off:off + h * w].reshape(h, w))
            off += h * w
        return out

    def pyramid(self, rgb, levels, out=None):
        import torch
        return torch.from_numpy(flatten(pyramid_ref(rgb.numpy(), levels, self.dt)))

    def detect(self, img, cell, border, min_eig, mask=None, cell_busy=None, out=None):
        import torch
        res, clear = detect_ref(img.numpy(), cell, border, min_eig, None if mask is None else mask.numpy(),
                                None if cell_busy is None else cell_busy.numpy(), self.dt)
        self.excluded += int((~clear).sum())
        self.decisions += len(clear)
        return torch.from_numpy(res)

    def track(self, pyr_a, pyr_b, H, W, levels, pts, *, mask=None, fb_ref=None, status=None, cell=0, cell_busy=None,
              out=None, resid=None, **params):
        import torch
        a, b = self._levels(pyr_a.numpy(), H, W, levels), self._levels(pyr_b.numpy(), H, W, levels)
        r = track_ref(a, b, pts.numpy(), mask=None if mask is None else mask.numpy(),
                      fb_ref=None if fb_ref is None else fb_ref.numpy(), status=None if status is None else status.numpy(),
                      cell=cell if cell_busy is not None else 0, n_cells=0 if cell_busy is None else cell_busy.numel(),
                      dt=self.dt, **params)
        self.excluded += int((~r["clear"]).sum())
        self.decisions += len(r["clear"])
        if fb_ref is not None:
            status.copy_(torch.from_numpy(r["status"]))
            if cell_busy is not None:
                cell_busy.copy_(torch.maximum(cell_busy, torch.from_numpy(r["busy"])))
        else:
            status = torch.from_numpy(r["status"])
        return torch.from_numpy(r["out"]), status, torch.from_numpy(r["resid"])


# ---- the 6-frame sequence through KLTSparseTracks, shared by the CPU test (numpy reference) and the device test --------
SEQ_MASK_RECT = (40, 60, 70, 95)  # rows 40..59, columns 70..94 are NOT usable, in every frame


def sequence_inputs(T=6, H=96, W=128):
    """-> (frames [T] of rgb float32 [H,W,3], mask [H,W] uint8 (1 = usable), warps), computed once"""
    key = ("seq", T, H, W)
    if key not in _CACHE:
        frames, warps = make_sequence(T, H, W)
        mask = np.ones((H, W), np.uint8)
        y0, y1, x0, x1 = SEQ_MASK_RECT
        mask[y0:y1, x0:x1] = 0
        _CACHE[key] = (frames, mask, warps)
    return _CACHE[key]


def run_sequence(kernels=None, device="cpu", frames=None, mask=None, resize=None, **kw):
    """KLTSparseTracks (levels 3, eps 0, otherwise its defaults) over the sequence -> (tracker, status bytes per frame)"""
    import torch
    from vipe_amd.slam.sparse_tracks import KLTSparseTracks
    from vipe_amd.slam.system import Frame
    if frames is None:
        frames, mask, _ = sequence_inputs()
    args = dict(levels=3, eps=0.0, resize=resize)
    args.update(kw)
    tr = KLTSparseTracks(1, device=device, _kernels=kernels, **args)
    statuses = []
    for f in frames:
        m = None if mask is None else torch.from_numpy(mask).bool().to(device)
        tr.track_image([Frame(rgb=torch.from_numpy(f).to(device), mask=m)])
        statuses.append(tr.last_status[0])
    return tr, statuses
