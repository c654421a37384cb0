"""Float64 reference, seeded inputs and the error bound of `vipe_convex_upsample` (a helper, not a test module).

Definition (DROID-SLAM's cvx_upsample): for mask row s, coarse pixel (y, x), sub-pixel (dy, dx) in 0..7, tap
k = ky*3 + kx with ky, kx in 0..2 and channel c

    out[r, 8y+dy, 8x+dx, c] = sum_k softmax_k(mask[s, y, x, k*64 + dy*8 + dx]) * data[r, y+ky-1, x+kx-1, c]

with data read as zero outside the grid and r = rows[s] (r = s without rows).  `cvx_upsample_ref` is written straight
from that line with explicit indexing - not with unfold: tests/test_cvx_reference.py compares it with the unfold
composition, so the tap and sub-pixel indexing of the oracle is checked independently of the kernel.
"""
import numpy as np

EPS32 = 2.0 ** -23

# Error bound of the float32 kernel: |out - ref| <= C_BOUND * EPS32 * max_k |data_k| (per channel, over the 3 x 3
# neighbourhood with the zeros of the padding).  With u = EPS32 / 2 the unit roundoff, x_k = max - logit_k >= 0,
# a_k = exp(-x_k), A = sum a_k >= 1 (the largest logit contributes exactly 1) and D = max_k |data_k|, the kernel computes
#   t_k = fl(logit_k - max)          one rounding: |t_k + x_k| <= u x_k, so exp(t_k) = a_k (1 + d), |d| <= u x_k
#   e_k = expf(t_k)                  documented at 1 ulp (HIP math API), a relative error <= EPS32
#   num = fma chain over 9 taps      9 roundings on the oldest term: relative <= 9 u = 4.5 EPS32 on every product
#   den = 8 additions                relative <= 8 u = 4 EPS32 on every term
#   out = num / den                  correctly rounded division: u = 0.5 EPS32
# so e_k = a_k (1 + eta_k) with |eta_k| <= EPS32 + (EPS32 / 2) x_k, and sum_k a_k |eta_k| <= EPS32 A +
# (EPS32 / 2) sum_k x_k exp(-x_k) <= (1 + 8 / (2 e)) EPS32 A = 2.4715 EPS32 A (x exp(-x) <= 1 / e for the eight taps that
# are not the maximum; A >= 1).  To first order
#   |num - N| / A <= (2.4715 + 4.5) EPS32 D,    |den - A| / A <= (2.4715 + 4) EPS32,    |N / A| <= D
#   |out - N / A| <= (6.9715 + 6.4715 + 0.5) EPS32 D = 13.943 EPS32 D
# The second-order terms are below 200 EPS32^2 D and the absolute error of a subnormal e_k (2^-149, against A >= 1) is
# smaller still; with the float64 reference's own error (1e-15 D) they fit the step to the next integer.
C_BOUND = 14

# (N, h, w, C): ragged shapes (odd sizes, a workgroup's 16 coarse pixels running over the end of a row, of a mask row and
# of the whole problem; every channel count's kernel) and one with more than one workgroup in each dimension
RAGGED_SHAPES = [(3, 5, 11, 1), (2, 3, 9, 2), (1, 1, 1, 4)]
MULTI_WORKGROUP_SHAPE = (2, 41, 73, 1)
ONE_HOT_SHAPE = (2, 4, 6, 1)
ROWS_CASE = dict(N=3, R=7, h=5, w=11, C=1, rows=[5, 0, 3])
SENTINEL = -12345.0


def make_inputs(N, h, w, C, mask_dtype=np.float16, seed=0, R=None, sigma=3.0):
    """-> (data [R,h,w,C] float32, mask [N,h,w,576] mask_dtype): logits ~ N(0, sigma) rounded to the mask's dtype (the
    reference is computed from these exact values), data ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    mask = rng.normal(0.0, sigma, (N, h, w, 576)).astype(mask_dtype)
    data = rng.normal(0.0, 1.0, (N if R is None else R, h, w, C)).astype(np.float32)
    return data, mask


def make_large_logits(N, h, w, C, lo, hi, seed=0):
    """float32 logits uniform in [lo, hi] (expf overflows at 88.7 without the maximum subtracted)"""
    rng = np.random.default_rng(seed)
    mask = rng.uniform(lo, hi, (N, h, w, 576)).astype(np.float32)
    data = rng.normal(0.0, 1.0, (N, h, w, C)).astype(np.float32)
    return data, mask


def make_one_hot(N, h, w, C, mask_dtype=np.float16, seed=0):
    """-> (data, mask, taps [N,h,w,8,8]): the chosen tap's logit is 0, the other eight -60000 (exact in fp16; exp of it
    underflows to an exact 0 in float32), the tap drawn per coarse pixel and sub-pixel"""
    rng = np.random.default_rng(seed)
    taps = rng.integers(0, 9, (N, h, w, 8, 8))
    mask = np.full((N, h, w, 9, 8, 8), -60000.0, dtype=np.float64)
    np.put_along_axis(mask, taps[:, :, :, None], 0.0, axis=3)
    data = rng.normal(0.0, 1.0, (N, h, w, C)).astype(np.float32)
    return data, mask.reshape(N, h, w, 576).astype(mask_dtype), taps


def one_hot_expected(data, taps):
    """the selected neighbour's value for every fine pixel, 0.0 where the tap falls outside the grid -> [N,8h,8w,C], in
    data's dtype (bit-exact expectation)"""
    N, h, w, C = data.shape
    pad = np.zeros((N, h + 2, w + 2, C), dtype=data.dtype)
    pad[:, 1:-1, 1:-1] = data
    n, y, x, dy, dx = np.meshgrid(*(np.arange(s) for s in taps.shape), indexing="ij")
    sel = pad[n, y + taps // 3, x + taps % 3]  # [N,h,w,8,8,C]: tap k = ky*3 + kx reads (y + ky - 1, x + kx - 1)
    return np.ascontiguousarray(sel.transpose(0, 1, 3, 2, 4, 5)).reshape(N, 8 * h, 8 * w, C)


def _padded(data):
    R, h, w, C = data.shape
    pad = np.zeros((R, h + 2, w + 2, C), dtype=np.float64)
    pad[:, 1:-1, 1:-1] = data
    return pad


def cvx_upsample_ref(data, mask, rows=None):
    """float64 -> [N,8h,8w,C]: the upsampled data[rows[s]] (data[s] without rows) for every mask row s"""
    data = np.asarray(data, dtype=np.float64)
    mask = np.asarray(mask).astype(np.float64)
    N, h, w, _ = mask.shape
    C = data.shape[3]
    pad = _padded(data if rows is None else data[np.asarray(rows, dtype=np.int64)])
    logits = mask.reshape(N, h, w, 9, 8, 8)  # channel = k*64 + dy*8 + dx
    e = np.exp(logits - logits.max(axis=3, keepdims=True))
    p = e / e.sum(axis=3, keepdims=True)
    out = np.zeros((N, h, 8, w, 8, C), dtype=np.float64)
    for ky in range(3):
        for kx in range(3):
            nb = pad[:N, ky:ky + h, kx:kx + w]  # data[y + ky - 1, x + kx - 1], zero outside
            for dy in range(8):
                for dx in range(8):
                    out[:, :, dy, :, dx, :] += p[:, :, :, ky * 3 + kx, dy, dx, None] * nb
    return out.reshape(N, 8 * h, 8 * w, C)


def neighbourhood_minmax(data, rows=None):
    """-> (lo, hi) [N,8h,8w,C] float64: min and max over the 3 x 3 coarse neighbourhood of every fine pixel, the zeros of
    the padding included"""
    data = np.asarray(data, dtype=np.float64)
    pad = _padded(data if rows is None else data[np.asarray(rows, dtype=np.int64)])
    N, h, w, C = pad.shape[0], pad.shape[1] - 2, pad.shape[2] - 2, pad.shape[3]
    st = np.stack([pad[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)])
    up = lambda a: np.repeat(np.repeat(a, 8, axis=1), 8, axis=2)  # noqa: E731
    return up(st.min(0)), up(st.max(0))


def cvx_bound(data, rows=None):
    """C_BOUND * EPS32 * max |data| over the 3 x 3 neighbourhood, per fine pixel and channel -> [N,8h,8w,C]"""
    lo, hi = neighbourhood_minmax(data, rows)
    return C_BOUND * EPS32 * np.maximum(np.abs(lo), np.abs(hi))


def torch_composition(data, mask_nhwc):
    """DROID-SLAM's cvx_upsample as torch operators (softmax + F.unfold + sum) in the tensors' dtype and on their
    device: data [N,h,w,C], mask [N,h,w,576] -> [N,8h,8w,C]"""
    import torch
    import torch.nn.functional as F
    N, h, w, C = data.shape
    m = mask_nhwc.permute(0, 3, 1, 2).to(data.dtype).reshape(N, 1, 9, 8, 8, h, w)
    m = torch.softmax(m, dim=2)
    up = F.unfold(data.permute(0, 3, 1, 2), [3, 3], padding=1).view(N, C, 9, 1, 1, h, w)
    up = torch.sum(m * up, dim=2)
    return up.permute(0, 4, 2, 5, 3, 1).reshape(N, 8 * h, 8 * w, C)
