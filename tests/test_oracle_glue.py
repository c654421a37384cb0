"""The references of oracle/glue.py pinned to hand-worked numbers, and the inputs of oracle/glue_cases.py checked with
those references alone: every property tests/test_gpu_glue_kernels.py relies on to catch a wrong kernel (which copy unit
a gather job selects, which segment sizes occur, how much the fp16 rounding of the deltas moves the score, that `du` is
no identity) holds for the numbers the GPU test feeds the kernels - so that a pass on the GPU means something.
"""

import numpy as np
import pytest

from oracle import glue
from oracle import glue_cases as gc

# ------------------------------------------------------------------------------------------------ hand-worked values


def test_rows_gather_ref_by_hand():
    """two rows of two 2-byte segments every 3 bytes; source rows 4 apart behind 1 byte, destination rows 8 apart"""
    src = np.arange(16, dtype=np.uint8)
    dst = np.full(24, 99, dtype=np.uint8)
    job = glue.rows_job(2, 0, idx=[2, 0], dst_row0=1, seg=(2, 3, 2), src_off=1, src_row_pitch=4, dst_row_pitch=8)
    want = [99] * 8 + [9, 10, 99, 12, 13, 99, 99, 99] + [1, 2, 99, 4, 5, 99, 99, 99]
    assert glue.rows_gather_ref(dst, src, job).tolist() == want
    job = glue.rows_job(2, 0, idx=None, dst_row0=0, seg=(2, 3, 2), src_off=1, src_row_pitch=4, dst_row_pitch=8)
    want = [1, 2, 99, 4, 5, 99, 99, 99] + [5, 6, 99, 8, 9, 99, 99, 99] + [99] * 8
    assert glue.rows_gather_ref(dst, src, job).tolist() == want
    assert np.all(dst == 99)  # the input is left alone


def test_rows_unit_by_hand():
    assert glue.rows_unit(glue.rows_job(1, 32)) == 16
    assert glue.rows_unit(glue.rows_job(1, 24)) == 8
    assert glue.rows_unit(glue.rows_job(1, 20)) == 4
    assert glue.rows_unit(glue.rows_job(1, 32, src_off=4)) == 4 and glue.rows_unit(glue.rows_job(1, 32, dst_off=8)) == 8
    assert glue.rows_unit(glue.rows_job(1, 64, seg=(16, 24, 2))) == 8  # the segment pitch counts too
    assert glue.rows_unit(glue.rows_job(1, 6)) is None
    assert glue.rows_units(glue.rows_job(3, 64, seg=(16, 24, 2))) == 3 * 2 * 2


def test_nchw_to_nhwc_ref_by_hand():
    src = np.arange(12, dtype=np.float16).reshape(2, 2, 3)  # [N=2, C=2, P=3]: frame 1 channel 0 = 6 7 8, channel 1 = 9 10 11
    dst = np.full((3, 3, 4), -1, dtype=np.float16)
    out = glue.nchw_to_nhwc_ref(dst, src, [1, 0], 2, 3, 1, 4, 1)
    assert np.all(out[0] == -1)
    assert out[1].tolist() == [[-1, 6, 9, -1], [-1, 7, 10, -1], [-1, 8, 11, -1]]
    assert out[2].tolist() == [[-1, 0, 3, -1], [-1, 1, 4, -1], [-1, 2, 5, -1]]
    out = glue.nchw_to_nhwc_ref(dst, src, None, 2, 3, 0, 4, 2, n_rows=1)
    assert out[0].tolist() == [[-1, -1, 0, 3], [-1, -1, 1, 4], [-1, -1, 2, 5]] and np.all(out[1:] == -1)


def test_segment_mean_ref_by_hand():
    """three edges of one row and four channels, the middle two channels are the slice; segments {2, 0}, {}, {1}"""
    src = np.array([[[9, 1, 2, 9]], [[9, 10, 20, 9]], [[9, 4, -8, 9]]], dtype=np.float16)
    order, rowptr = [2, 0, 1], [0, 2, 2, 3]
    ref = glue.segment_mean_ref(src, 4, 1, order, rowptr, 2)
    assert ref.dtype == np.float64 and ref.tolist() == [[[2.5, -3.0]], [[0.0, 0.0]], [[10.0, 20.0]]]
    b = glue.segment_mean_bound(src, 4, 1, order, rowptr, 2)
    # segment 0, channel 1: |ref| 3, n 2, mean|x| 5;  the empty segment: the subnormal half-step alone
    assert b[0, 0, 1] == 2.0 ** -11 * 3 + 4 * 2.0 ** -24 * 5 + 2.0 ** -25
    assert np.all(b[1] == 2.0 ** -25)


def test_glo_context_ref_by_hand():
    glo = np.zeros((2, 128), dtype=np.float32)
    glo[0, 0], glo[0, 127], glo[1, 5] = 6.0, -3.0, 9.0
    wT = np.zeros((128, 384), dtype=np.float32)
    wT[0, 1], wT[127, 1], wT[127, 383], wT[5, 200] = 2.0, 4.0, 0.5, -1.0
    bias = np.zeros(384, dtype=np.float32)
    bias[1], bias[2] = 0.25, 7.0
    ref = glue.glo_context_ref(glo, wT, bias, 3)
    want = np.zeros((2, 384))
    want[:, 1], want[:, 2] = 0.25, 7.0
    want[0, 1] += 2.0 * 2.0 + -1.0 * 4.0  # (6/3) 2 + (-3/3) 4
    want[0, 383] = -0.5
    want[1, 200] = -3.0
    assert ref.dtype == np.float64 and np.array_equal(ref, want)
    assert glue.glo_context_bound(glo, wT, bias, 3)[0, 1] == 132 * 2.0 ** -24 * (0.25 + 4.0 + 4.0)


def test_update_finish_ref_by_hand():
    coords1 = np.array([[[[1.0, 2.0], [3.0, 4.0]]], [[[5.0, 6.0], [7.0, 8.0]]]], dtype=np.float32)  # [E=2, 1, 2, 2]
    dw = np.array([[[[0.5, -0.5, 0.1, 0.2], [1.0, 1.0, 0.3, 0.4]]], [[[-1.0, 0.0, 0.5, 0.6], [0.25, 0.75, 0.7, 0.8]]]], dtype=np.float32)
    mask = np.array([[[False, True]], [[False, False]]])
    eta = np.array([[[10.0, 11.0]]], dtype=np.float32)
    damping = np.array([[[1.0, 2.0]], [[3.0, 4.0]], [[5.0, 6.0]]], dtype=np.float32)
    t, w, d = glue.update_finish_ref(coords1, dw, mask, eta, [2], damping)
    assert t.dtype == w.dtype == d.dtype == np.float32
    assert t.tolist() == [[[[1.5, 1.5], [4.0, 5.0]]], [[[4.0, 6.0], [7.25, 8.75]]]]
    assert np.array_equal(w, np.array([[[[0.1, 0.2], [0.0, 0.0]]], [[[0.5, 0.6], [0.7, 0.8]]]], dtype=np.float32))
    assert not np.signbit(w[0, 0, 1]).any()
    assert d.tolist() == [[[1.0, 2.0]], [[3.0, 4.0]], [[10.0, 11.0]]] and damping[2, 0, 0] == 5.0
    t, w, d = glue.update_finish_ref(coords1, dw, None, None, None, damping)
    assert np.array_equal(w, dw[..., 2:]) and np.array_equal(d, damping)


def test_flow_score_ref_by_hand():
    """view 0: deltas (3, 4) and (2049, 0) -> fp16 (3, 4), (2048, 0): norms 5 and 2048;  view 1: (0.6, 0.8) twice in fp16"""
    dw = np.zeros((2, 2, 4), dtype=np.float32)
    dw[0, 0, :2], dw[0, 1, :2] = (3, 4), (2049, 0)
    dw[1, :, :2] = (0.6, 0.8)
    dw[..., 2:] = np.nan
    ref = glue.flow_score_ref(dw, None)
    h6, h8 = float(np.float16(0.6)), float(np.float16(0.8))
    assert ref.dtype == np.float64 and ref[0] == (5 + 2048) / 2 and ref[1] == np.sqrt(h6 * h6 + h8 * h8)
    assert glue.flow_score_ref(dw, None, round_half=False)[0] == (5 + 2049) / 2
    invalid = np.array([[False, True], [True, True]])
    ref = glue.flow_score_ref(dw, invalid)
    assert ref[0] == (5 / 2) / (0.5 + 1e-6) and ref[1] == 0.0
    assert glue.flow_score_bound(np.array([2.0]), 257)[0] == 18 * 2.0 ** -23 * 2.0


# ------------------------------------------------------------------------------------------------ the case conditions


@pytest.mark.parametrize("V,P", gc.FLOW_SIZES)
@pytest.mark.parametrize("mask", gc.FLOW_MASKS)
def test_flow_score_cases(V, P, mask):
    """large deltas: a kernel without the fp16 rounding is off by >= 100 x the GPU bound; a wholly invalid view scores
    exactly 0; NaN weights do not reach the score"""
    c = gc.flow_case(V, P, "large", mask)
    ref = glue.flow_score_ref(c.dw, c.invalid)
    raw = glue.flow_score_ref(c.dw, c.invalid, round_half=False)
    live = ref != 0
    assert live.any() or (mask == "first_invalid" and V == 1)
    assert np.all(np.abs(raw - ref)[live] >= 100 * glue.flow_score_bound(ref, P)[live]), (raw, ref)
    if live.any():
        assert 3000 < ref[live].mean() < 4000
    for magnitude in gc.FLOW_MAGNITUDES:
        c = gc.flow_case(V, P, magnitude, mask)
        ref = glue.flow_score_ref(c.dw, c.invalid)
        if mask == "first_invalid":
            assert c.invalid[0].all() and ref[0] == 0.0
        if mask == "last_valid":
            assert not c.invalid[-1].any() and ref[-1] > 0
        if mask in ("random", "first_invalid", "last_valid") and V > 1:
            assert 0 < c.invalid.mean() < 1
        n = gc.flow_case(V, P, magnitude, mask, nan_weights=True)
        assert np.isnan(n.dw[..., 2:]).all() and np.array_equal(n.dw[..., :2], c.dw[..., :2])
        got = glue.flow_score_ref(n.dw, n.invalid)
        assert np.isfinite(got).all() and np.array_equal(got, ref)


def test_segment_mean_cases():
    """an empty segment, segments of 1, 2, 3 and >= 32 edges, an order that is not sorted by edge; reading edge q in place
    of order[q] moves some segment by more than 10 x the GPU bound (in every case, the second-trip one included)"""
    sizes = set()
    for name in list(gc.SEG_LAYOUTS) + ["stride"]:
        c = gc.segment_case(name)
        n = np.diff(c.rowptr)
        sizes |= set(n.tolist())
        assert c.src.shape == (int(c.rowptr[-1]), c.rows, c.ctot) and sorted(c.order.tolist()) == list(range(len(c.order)))
        assert not np.array_equal(c.order, np.sort(c.order))
        assert any(np.any(np.diff(c.order[a:b]) < 0) for a, b in zip(c.rowptr[:-1], c.rowptr[1:])) or name == "stride"
        ref = glue.segment_mean_ref(c.src, c.ctot, c.coff, c.order, c.rowptr, c.C)
        bound = glue.segment_mean_bound(c.src, c.ctot, c.coff, c.order, c.rowptr, c.C)
        wrong = glue.segment_mean_ref(c.src, c.ctot, c.coff, np.arange(len(c.order)), c.rowptr, c.C)
        assert np.any(np.abs(wrong - ref) > 10 * bound), name
        assert np.abs(ref).max() < 10  # no +-1000 from the channels outside the slice
        for k in np.nonzero(n == 0)[0]:
            assert np.all(ref[k] == 0)
        if name != "stride":
            assert (np.abs(ref[-1]) < 2.0 ** -14).mean() > 0.9 and np.abs(ref[-1]).max() > 2.0 ** -17  # results in fp16's subnormal range
    assert {0, 1, 2, 3} <= sizes and max(sizes) >= 32
    s = gc.segment_case("stride")
    assert s.rows * (s.C // 8) > 1024 * 256
    assert gc.SEG_LAYOUTS["operator"] == (45, 384, 256, 128)


def test_rows_gather_cases():
    """which copy unit each job selects under the header's alignment rule; all three occur, the 4-byte one once from a
    size and once from an address; the big job needs a second grid-stride trip"""
    units = {name: [None if s.job is None else glue.rows_unit(s.job) for s in gc.rows_launch(name)] for name in gc.ROWS_LAUNCHES}
    assert units == {"units": [16, 8, 4, 4, 8], "segments": [16, 8], "indices": [8, 8], "big": [None, 16, 4, None, 4, 8, 4, 8]}
    u = [s.job for s in gc.rows_launch("units")]
    assert [j["seg_bytes"] for j in u] == [4608, 360, 36, 4608, 4608]
    assert u[2]["seg_bytes"] % 8 == 4 and u[2]["src_off"] == u[2]["dst_off"] == 0           # 4 from the size
    assert u[3]["seg_bytes"] % 16 == 0 and u[3]["src_off"] == u[3]["dst_off"] == 4          # 4 from the address
    assert u[4]["src_off"] == u[4]["dst_off"] == 8
    big = gc.rows_launch("big")
    assert len(big) == 8 and big[0].job is None and big[3].job is None
    assert glue.rows_units(big[2].job) > 4096 * 256 and big[2].job["seg_bytes"] == 4004 and big[2].job["n_rows"] == 1100
    assert big[4].job["n_rows"] == 1 and big[4].job["seg_bytes"] == 4
    seg = [s.job for s in gc.rows_launch("segments")]
    assert (seg[0]["seg_bytes"], seg[0]["seg_pitch"], seg[0]["n_seg"]) == (256, 640, 45)
    assert (seg[1]["seg_bytes"], seg[1]["seg_pitch"]) == (8, 24)
    ind = [s.job for s in gc.rows_launch("indices")]
    assert ind[0]["idx"] is None and ind[0]["dst_row0"] == 3
    d = np.diff(ind[1]["idx"])
    assert np.all(d <= 0) and np.any(d == 0) and np.any(d < 0)
    for name in gc.ROWS_LAUNCHES:
        for s in gc.rows_launch(name):
            if s.job is None:
                continue
            want = glue.rows_gather_ref(s.dst, s.src, s.job)  # also asserts that every access lies inside the buffers
            assert np.any(want != s.dst) and np.any(want == gc.SENTINEL_BYTE)
            # the same job without its dst_row0 stays inside the buffers and gives another result (what the test must catch)
            if s.job["dst_row0"]:
                assert not np.array_equal(glue.rows_gather_ref(s.dst, s.src, dict(s.job, dst_row0=0)), want)


def test_update_finish_cases():
    """du is no identity, damping has rows outside du, and n_src == 0, < E, == E and > E all occur"""
    kinds = set()
    cases = [gc.finish_case(E, h, w, None if du is None else tuple(du), masked)
             for (E, h, w) in gc.UF_GRIDS for du in gc.UF_DU[E].values() for masked in (False, True)]
    (E1, h1, w1), du1 = gc.UF_MORE
    cases.append(gc.finish_case(E1, h1, w1, tuple(du1), True))
    for c in cases:
        n_src = 0 if c.du is None else len(c.du)
        kinds.add("zero" if n_src == 0 else "fewer" if n_src < c.E else "equal" if n_src == c.E else "more")
        assert c.damping.shape[0] == gc.UF_DAMPING_ROWS
        if n_src:
            assert not np.array_equal(c.du, np.arange(n_src)) and len(set(c.du.tolist())) == n_src
            assert c.du.max() < c.damping.shape[0] and n_src < c.damping.shape[0]  # rows outside du exist
            _, _, d = glue.update_finish_ref(c.coords1, c.dw, c.mask, c.eta, c.du, c.damping)
            outside = np.setdiff1d(np.arange(c.damping.shape[0]), c.du)
            assert np.array_equal(d[outside], c.damping[outside]) and np.array_equal(d[c.du], c.eta)
            # scattering to rows 0 .. n_src - 1 instead stays inside damping and gives another result
            assert not np.array_equal(glue.update_finish_ref(c.coords1, c.dw, c.mask, c.eta, np.arange(n_src), c.damping)[2], d)
        if c.mask is not None:
            assert 0 < c.mask.mean() < 1 and (c.E == 1 or (not c.mask[0].any() and c.mask[1:].any()))
    assert kinds == {"zero", "fewer", "equal", "more"}
    assert [g[1] * g[2] * g[0] for g in gc.UF_GRIDS] == [225, 777]
    assert gc.UF_DU[5]["fewer"] == [7, 2, 4] and sorted(gc.UF_DU[5]["equal"]) == list(range(5))


def test_nhwc_cases():
    """the (C, P) pairs of the issue, a frame list with repeats and out of order, every job with a destination offset"""
    assert [(C, P) for C, P, _, _ in gc.NHWC_SINGLE] == [(128, 45), (128, 64), (128, 65), (96, 130), (64, 200), (8, 1), (3, 200)]
    assert (64, 200, 320, 128) in gc.NHWC_SINGLE and gc.NHWC_ROW0 > 0
    f = gc.NHWC_FRAMES
    assert len(set(f.tolist())) < len(f) and not np.array_equal(f, np.sort(f)) and f.max() < gc.NHWC_N
    assert len(gc.NHWC_MULTI) == 8 and len({(ct, co) for ct, co, _, _ in gc.NHWC_MULTI}) == 8
    assert all(co + gc.NHWC_MULTI_CP[0] <= ct for ct, co, _, _ in gc.NHWC_MULTI)
