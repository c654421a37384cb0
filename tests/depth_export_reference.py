"""Float64 reference, seeded inputs and the error bound of `vipe_depth_export` (a helper, not a test module).

Definition (include/vipe_amd.h): out[n] [H0,W0] from disp[rows[n]] [H,W].  Per axis, with n_res = h1 | w1,
n_out = H0 | W0, off = top | left, n_in = H | W, for output index dst:

    scale = float32(n_res) / float32(n_out)                       one float32 division
    src   = max(fma(scale, dst + 0.5, -0.5), 0)                   one float32 rounding
    src   = clamp(src - off, 0, n_in - 1)                         exact
    i0 = int(src), i1 = min(i0 + 1, n_in - 1), l1 = src - i0, l0 = 1 - l1      (float32)

    d     = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * e),   a, b = disp[iy0, ix0 | ix1], c, e = disp[iy1, ix0 | ix1]
    depth = depth_scale / d  where d > 0,  0 elsewhere

`axis_taps` evaluates scale, src, l0 and l1 in float32 exactly as the kernel does: the taps and weights are INPUTS of
the blend, shared by kernel and reference.  The fused multiply-add is the float64 expression rounded once to float32 -
scale * (dst + 0.5) is exact in float64 (two 24-bit significands) and so is the sum with -0.5 while it spans at most 53
bits, i.e. for scale >= 2^-5 (asserted).  Blend and division are evaluated in float64, written with explicit indexing.

Error bound of the float32 kernel.  u = 2^-24 is the unit roundoff, all weights are >= 0.  In the kernel's blend every
tap value passes through four roundings (its product with lx, the inner sum, the product with ly, the outer sum), so
    |d_k - d| <= g4 * S,   g4 = 4u / (1 - 4u),   S = ly0 * (lx0 |a| + lx1 |b|) + ly1 * (lx0 |c| + lx1 |e|)
(the standard gamma_n bound of a rounded sum of products with n roundings per term; S = d for positive maps).  The
division is correctly rounded: depth_k = (depth_scale / d_k) (1 + e), |e| <= u.  With rho = g4 * S / d < 1
    |depth_k - depth| <= depth * ((1 + u) / (1 - rho) - 1)
which is the bound, times (1 + 2^-20) for the float64 reference's own roundings (about 10 * 2^-53 relative) - to first
order 5 u of the result, 2.5 of its float32 epsilons.  It holds while d and the
products stay in float32's normal range (|disp| in [1e-30, 1e30], asserted by `depth_bound`); where d <= 0 in the
reference the kernel's value is only pinned when all four taps are <= 0 (then both are exactly 0) - `depth_bound` returns
inf for the other d <= 0 pixels and for rho >= 1 (cancellation between taps of mixed sign), which the tests' positive
maps never have.
"""
import numpy as np

U32 = 2.0 ** -24
G4 = 4 * U32 / (1 - 4 * U32)

# the cases of tests/test_gpu_depth_export.py and tests/test_depth_export_reference.py: (H, W) = (24, 40) maps, the
# smallest that still span more than one 64 x 4 tile in both directions after export
HW = (24, 40)
UP_CROP = (27, 45, 1, 2, 61, 97)     # (h1, w1, top, left, H0, W0): upsampling, crop bands of 1 | 2 rows and 2 | 3 columns
DOWN = (27, 45, 1, 2, 13, 19)        # the same source, native size below SLAM resolution
SENTINEL = float("nan")


def identity_params(H, W):
    return (H, W, 0, 0, H, W)


def make_disps(R, H=HW[0], W=HW[1], seed=0):
    """disparities 1 / U(1, 5), float32 [R,H,W]"""
    rng = np.random.default_rng(seed)
    return (1.0 / rng.uniform(1.0, 5.0, (R, H, W))).astype(np.float32)


def axis_taps(n_res, n_out, off, n_in):
    """-> (i0, i1 int64 [n_out], l0, l1 float32 [n_out]) in the kernel's float32 arithmetic"""
    f32 = np.float32
    scale = f32(n_res) / f32(n_out)
    assert scale >= 2.0 ** -5, "the float64 evaluation of the fused multiply-add is only exact for scale >= 2^-5"
    dst = np.arange(n_out, dtype=np.float32) + f32(0.5)
    src = (np.float64(scale) * dst.astype(np.float64) - 0.5).astype(np.float32)  # the fma: one rounding
    src = np.maximum(src, f32(0.0))
    src = np.minimum(np.maximum(src - f32(off), f32(0.0)), f32(n_in - 1))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (f32(1.0) - l1).astype(np.float32)
    return i0, i1, l0, l1


def _blend64(maps, params):
    """-> (d, S) float64 [N,H0,W0]: the blend of the maps and of their absolute values"""
    h1, w1, top, left, H0, W0 = params
    N, H, W = maps.shape
    assert top >= 0 and left >= 0 and top + H <= h1 and left + W <= w1
    y0, y1, ly0, ly1 = axis_taps(h1, H0, top, H)
    x0, x1, lx0, lx1 = axis_taps(w1, W0, left, W)
    m = maps.astype(np.float64)
    d = np.empty((N, H0, W0), dtype=np.float64)
    S = np.empty_like(d)
    for Y in range(H0):
        a, b = m[:, y0[Y]][:, x0], m[:, y0[Y]][:, x1]
        c, e = m[:, y1[Y]][:, x0], m[:, y1[Y]][:, x1]
        wy0, wy1 = np.float64(ly0[Y]), np.float64(ly1[Y])
        wx0, wx1 = lx0.astype(np.float64), lx1.astype(np.float64)
        d[:, Y] = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * e)
        S[:, Y] = wy0 * (wx0 * np.abs(a) + wx1 * np.abs(b)) + wy1 * (wx0 * np.abs(c) + wx1 * np.abs(e))
    return d, S


def _select(disp, rows):
    disp = np.asarray(disp)
    assert disp.dtype == np.float32 and disp.ndim == 3
    return disp if rows is None else disp[np.asarray(rows, dtype=np.int64)]


def depth_export_ref(disp, params, rows=None, depth_scale=1.0):
    """float64 -> [N,H0,W0]: depth of disp[rows[n]] (disp[n] without rows); `rows` entries must lie inside [0, R).
    `depth_scale` is taken as the float32 the kernel receives."""
    d, _ = _blend64(_select(disp, rows), params)
    s = np.float64(np.float32(depth_scale))
    out = np.zeros_like(d)
    np.divide(s, d, out=out, where=d > 0)
    return out


def depth_bound(disp, params, rows=None, depth_scale=1.0):
    """the per-pixel bound derived above -> float64 [N,H0,W0]; 0 where all four taps are <= 0 (exact zeros), inf where
    the derivation does not hold"""
    maps = _select(disp, rows)
    nz = np.abs(maps[maps != 0])
    assert nz.size == 0 or (nz.min() >= 1e-30 and nz.max() <= 1e30), "outside the normal range the bound does not hold"
    d, S = _blend64(maps, params)
    nonpos, _ = _blend64(np.where(maps > 0, np.float32(1.0), np.float32(0.0)), params)  # 0 iff no weighted tap is > 0
    s = abs(np.float64(np.float32(depth_scale)))
    bound = np.full_like(d, np.inf)
    ok = d > 0
    rho = np.where(ok, G4 * S / np.where(ok, d, 1.0), 1.0)
    good = ok & (rho < 1)
    bound[good] = (s / d[good]) * ((1 + U32) / (1 - rho[good]) - 1) * (1 + 2.0 ** -20)
    bound[nonpos == 0] = 0.0
    return bound


def torch_composition(disp, params, depth_scale=1.0):
    """The same map as torch operators in the tensor's dtype and on its device: replicate-pad the cropped maps back to
    (h1, w1), F.interpolate(bilinear, align_corners=False) to (H0, W0), reciprocal where positive.  disp [N,H,W]"""
    import torch
    import torch.nn.functional as F
    h1, w1, top, left, H0, W0 = params
    N, H, W = disp.shape
    x = F.pad(disp[:, None], (left, w1 - W - left, top, h1 - H - top), mode="replicate")
    d = F.interpolate(x, size=(H0, W0), mode="bilinear", align_corners=False)[:, 0]
    return torch.where(d > 0, depth_scale / d, torch.zeros_like(d))
