"""The small kernels between the heavy ones of an update iteration, restated in plain numpy.

ORACLE (test infrastructure).  Byte-exact where the kernel only moves data (`vipe_rows_gather`,
`vipe_gather_nchw_to_nhwc_f16`, `vipe_update_finish`), float64 where it computes (`vipe_segment_mean_nhwc_f16`,
`vipe_glo_context`, `vipe_flow_score`) - with the bound each float32 kernel has to meet next to its reference, derived
from the roundings the operation needs and not from what a kernel returns.  Written from the contract in
include/vipe_amd.h and the reference lines cited there; tests/test_oracle_glue.py pins every function to hand-worked
numbers, tests/test_gpu_glue_kernels.py compares the kernels with them.
"""

import numpy as np

U32 = 2.0 ** -24  # unit roundoff of float32
U16 = 2.0 ** -11  # ... of float16


# ------------------------------------------------------------------------------------------------ vipe_rows_gather
def rows_job(n_rows, row_bytes, idx=None, dst_row0=0, seg=None, src_off=0, dst_off=0, src_row_pitch=None,
             dst_row_pitch=None):
    """One `vipe_rows_job` as a dict: `seg` = (seg_bytes, seg_pitch, n_seg) or None for whole rows of `row_bytes`;
    `src_off` / `dst_off`: where the job's src / dst pointers stand inside their allocations (bytes)."""
    seg_bytes, seg_pitch, n_seg = seg or (row_bytes, row_bytes, 1)
    return dict(n_rows=int(n_rows), idx=None if idx is None else np.asarray(idx, dtype=np.int64), dst_row0=int(dst_row0),
                seg_bytes=int(seg_bytes), seg_pitch=int(seg_pitch), n_seg=int(n_seg), src_off=int(src_off), dst_off=int(dst_off),
                src_row_pitch=int(src_row_pitch or row_bytes), dst_row_pitch=int(dst_row_pitch or row_bytes))


def rows_gather_ref(dst_bytes, src_bytes, job):
    """dst row (dst_row0 + r) = src row idx[r] (r itself without idx), r < n_rows; a row is n_seg segments of seg_bytes
    every seg_pitch bytes, rows every *_row_pitch bytes, counted from src_off / dst_off of the uint8 buffers.
    -> the whole destination buffer as it has to look afterwards (a copy; bytes outside the segments keep their value)"""
    assert dst_bytes.dtype == np.uint8 and src_bytes.dtype == np.uint8 and dst_bytes.ndim == src_bytes.ndim == 1
    out = dst_bytes.copy()
    for r in range(job["n_rows"]):
        sr = r if job["idx"] is None else int(job["idx"][r])
        for s in range(job["n_seg"]):
            a = job["src_off"] + sr * job["src_row_pitch"] + s * job["seg_pitch"]
            b = job["dst_off"] + (job["dst_row0"] + r) * job["dst_row_pitch"] + s * job["seg_pitch"]
            assert 0 <= a and a + job["seg_bytes"] <= src_bytes.size and 0 <= b and b + job["seg_bytes"] <= out.size
            out[b:b + job["seg_bytes"]] = src_bytes[a:a + job["seg_bytes"]]
    return out


def rows_unit(job):
    """the copy unit the header promises: the largest of 16 / 8 / 4 bytes that segment size, every pitch and both
    addresses (allocations 16-byte aligned, so src_off / dst_off) are multiples of; None when 4 does not divide them"""
    every = [job[k] for k in ("seg_bytes", "seg_pitch", "src_row_pitch", "dst_row_pitch", "src_off", "dst_off")]
    for unit in (16, 8, 4):
        if all(v % unit == 0 for v in every):
            return unit
    return None


def rows_units(job):
    """number of copy units of a job"""
    return job["n_rows"] * job["n_seg"] * (job["seg_bytes"] // rows_unit(job))


# ---------------------------------------------------------------------------------- vipe_gather_nchw_to_nhwc_f16
def nchw_to_nhwc_ref(dst, src, frame, C, P, dst_row0, dst_ctot, dst_coff, n_rows=None):
    """`nets[frame].permute(0, 2, 3, 1)` (factor_graph.py:160-166 of the reference) written into the channel slice
    [dst_coff, dst_coff + C) of the rows dst_row0.. of dst [rows, P, dst_ctot]; src [N, C, P]; frame [n_rows], or None:
    row r reads frame r, for the first `n_rows` frames (default: all of src).  -> the whole destination (a copy)"""
    assert src.shape[1:] == (C, P) and dst.shape[1:] == (P, dst_ctot)
    out = dst.copy()
    if frame is None:
        frame = np.arange(src.shape[0] if n_rows is None else n_rows)
    for r, f in enumerate(frame):
        out[dst_row0 + r, :, dst_coff:dst_coff + C] = src[int(f)].T
    return out


# ---------------------------------------------------------------------------------- vipe_segment_mean_nhwc_f16
def _segment_sums(src, ctot, coff, order, rowptr, C):
    src = np.asarray(src)
    assert src.dtype == np.float16 and src.shape[-1] == ctot
    n_out = len(rowptr) - 1
    x = src[..., coff:coff + C].astype(np.float64)
    s = np.zeros((n_out,) + x.shape[1:], dtype=np.float64)
    a = np.zeros_like(s)
    n = np.zeros(n_out, dtype=np.int64)
    for k in range(n_out):
        for q in range(int(rowptr[k]), int(rowptr[k + 1])):
            s[k] += x[int(order[q])]
            a[k] += np.abs(x[int(order[q])])
            n[k] += 1
    return s, a, n


def segment_mean_ref(src, ctot, coff, order, rowptr, C):
    """scatter_mean of GraphAgg (droid_net.py:420-421 of the reference) over a CSR of the edges: out[k] = mean over
    q in [rowptr[k], rowptr[k+1]) of src[order[q], :, coff:coff+C]; src [E, rows, ctot] fp16 -> [n_out, rows, C] float64,
    zeros for an empty segment"""
    s, _, n = _segment_sums(src, ctot, coff, order, rowptr, C)
    return s / np.maximum(n, 1).reshape((-1,) + (1,) * (s.ndim - 1))


def segment_mean_bound(src, ctot, coff, order, rowptr, C):
    """per element: 2^-11 |ref| (the result is rounded to half) + (n + 2) 2^-24 mean|inputs| (n - 1 float32 additions of
    partial sums none larger than sum|inputs|, the rounded reciprocal of n, its product) + 2^-25 (half the step of
    fp16's subnormals, which the first term does not cover)"""
    s, a, n = _segment_sums(src, ctot, coff, order, rowptr, C)
    nn = np.maximum(n, 1).reshape((-1,) + (1,) * (s.ndim - 1))
    cnt = n.reshape(nn.shape)
    return U16 * np.abs(s / nn) + (cnt + 2) * U32 * (a / nn) + 2.0 ** -25


# ------------------------------------------------------------------------------------------------ vipe_glo_context
def glo_context_ref(glo_sum, wT, bias, hw):
    """the ConvGRU's three *_glo 1x1 convolutions on the pooled vector (droid_net.py:392-399 of the reference):
    bias + (glo_sum / hw) @ wT in float64; glo_sum [E,128], wT [128,384], bias [384]"""
    g = np.asarray(glo_sum, dtype=np.float64) / float(hw)
    return np.asarray(bias, dtype=np.float64)[None] + g @ np.asarray(wT, dtype=np.float64)


def glo_context_bound(glo_sum, wT, bias, hw):
    """132 x 2^-24 (|bias| + sum_k |g_k w_k|): 128 fused multiply-adds, the rounded 1 / hw and its product with the sum"""
    g = np.abs(np.asarray(glo_sum, dtype=np.float64)) / float(hw)
    return 132 * U32 * (np.abs(np.asarray(bias, dtype=np.float64))[None] + g @ np.abs(np.asarray(wT, dtype=np.float64)))


# ------------------------------------------------------------------------------------------------ vipe_update_finish
def update_finish_ref(coords1, dw, mask, eta, du, damping):
    """factor_graph.py:272-278 of the reference: weight[masked source frame's pixels] = 0, target = coords1 + delta,
    damping[du] = eta.  coords1 [E,h,w,2], dw [E,h,w,4] = (delta | weight), mask [E,h,w] bool or None, eta [n_src,h,w] or
    None, du [n_src], damping [*,h,w]; all float32 -> (target, weight, damping) float32: one float32 operation at most per
    value, so exact"""
    coords1, dw = np.asarray(coords1, dtype=np.float32), np.asarray(dw, dtype=np.float32)
    target = (coords1 + dw[..., :2]).astype(np.float32)
    weight = dw[..., 2:].copy()
    if mask is not None:
        weight[np.asarray(mask, dtype=bool)] = np.float32(0.0)
    out = None if damping is None else np.asarray(damping, dtype=np.float32).copy()
    if eta is not None and len(du):
        out[np.asarray(du, dtype=np.int64)] = np.asarray(eta, dtype=np.float32)
    return target, weight, out


# ------------------------------------------------------------------------------------------------ vipe_flow_score
def flow_score_ref(dw, invalid, round_half=True):
    """motion_filter.py:103-108 of the reference: per view mean |delta| over the pixels, or with a mask
    mean(|delta| (1 - invalid)) / (mean(1 - invalid) + 1e-6).  dw [V,P,4] float32 (delta | weight; the weights are not
    read), invalid [V,P] bool or None.  delta is the operator's fp16 head output: rounded to half first
    (`round_half=False` skips that - what a kernel that forgot it would compute), then float64 -> [V] float64"""
    d = np.asarray(dw)[..., :2]
    d = d.astype(np.float16).astype(np.float64) if round_half else d.astype(np.float64)
    flow = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    if invalid is None:
        return flow.mean(-1)
    w = 1.0 - np.asarray(invalid, dtype=bool).astype(np.float64)
    return (flow * w).mean(-1) / (w.mean(-1) + 1e-6)


def flow_score_bound(ref, P):
    """relative (ceil(P / 256) + 16) 2^-23: the per-lane sequential float32 sum, nine reduction steps, the square, add and
    sqrtf of each term, the two divisions"""
    return ((P + 255) // 256 + 16) * 2.0 ** -23 * np.abs(ref)
