"""The small kernels between the heavy ones of every update iteration and every keyframe, each against its own reference.

`vipe_rows_gather`, `vipe_gather_nchw_to_nhwc_f16` (edge_state.hip) and `vipe_update_finish` (update_op.hip) move data:
byte for byte against oracle/glue.py.  `vipe_segment_mean_nhwc_f16`, `vipe_flow_score` (aux_ops.hip) and
`vipe_glo_context` (update_op.hip) compute in float32: against float64 with the bound derived next to each reference in
oracle/glue.py from the roundings the operation needs (never from what the kernel returns).  Every output buffer is
prefilled with a sentinel, carries spare room behind the region the kernel may write, and is compared WHOLE.

The inputs come from oracle/glue_cases.py; tests/test_oracle_glue.py shows, without a GPU, that they have the properties
that make these comparisons bite (all three copy units, every segment size, deltas whose fp16 rounding matters, ...).
Each test prints its largest error as a fraction of the bound.
"""

import ctypes

import numpy as np
import pytest
import torch

from oracle import glue
from oracle import glue_cases as gc

pytestmark = pytest.mark.gpu

OK, EINVAL, EUNSUPPORTED = 0, -1, -3


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def bits(t, dtype=torch.uint8):
    """device tensor -> host tensor of its raw bytes / words"""
    return t.detach().cpu().contiguous().view(-1).view(dtype)


def same_bits(t, want):
    return torch.equal(bits(t), torch.from_numpy(np.ascontiguousarray(want)).view(-1).view(torch.uint8))


def abi():
    from vipe_amd._lib import lib, ptr, stream_ptr
    return lib(), ptr, stream_ptr


# ------------------------------------------------------------------------------------------------ vipe_rows_gather


def _rows_struct(slots):
    """the vipe_rows_job array of a launch, filled field by field (the Python helper of the factor graph demands an
    index and equal pitches) -> (array, [(dst tensor, expected bytes)], tensors to keep alive)"""
    from vipe_amd.slam.factor_graph import RowsJob
    arr = (RowsJob * len(slots))()
    outs, keep = [], []
    for j, s in zip(arr, slots):
        j.n_seg, j.seg_bytes, j.seg_pitch = 1, 4, 4
        if s.job is None:  # an empty job: no rows, null pointers
            continue
        src, dst, idx = T(s.src), T(s.dst), T(s.job["idx"])
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0  # what oracle.glue.rows_unit assumes
        j.src, j.dst = src.data_ptr() + s.job["src_off"], dst.data_ptr() + s.job["dst_off"]
        j.idx = None if idx is None else idx.data_ptr()
        for f in ("src_row_pitch", "dst_row_pitch", "seg_bytes", "seg_pitch", "n_seg", "n_rows", "dst_row0"):
            setattr(j, f, s.job[f])
        outs.append((dst, glue.rows_gather_ref(s.dst, s.src, s.job)))
        keep += [src, idx]
    return arr, outs, keep


@pytest.mark.parametrize("name", list(gc.ROWS_LAUNCHES))
def test_rows_gather_byte_exact(name):
    """units: one launch whose jobs select the 16-, 8- and 4-byte unit (the last once from a row size, once from the
    addresses).  segments: the per-pixel slice of the operator input's compaction and an 8-of-24-byte one; the bytes
    between the segments keep their sentinel.  indices: no index with dst_row0 = 3; a descending index with repeats.
    big: eight jobs, two of them empty with null pointers, one of a single 4-byte row, one of 1100 x 4004 bytes - more
    four-byte units than 4096 workgroups hold, so the grid-stride loop takes a second trip."""
    L, _, stream_ptr = abi()
    slots = gc.rows_launch(name)
    arr, outs, keep = _rows_struct(slots)
    assert L.vipe_rows_gather(ctypes.addressof(arr), len(slots), stream_ptr(outs[0][0])) == OK
    torch.cuda.synchronize()
    for k, (dst, want) in enumerate(outs):
        got = bits(dst).numpy()
        wrong = int((got != want).sum())
        print(f"rows_gather {name} live job {k}: {want.size} bytes, {wrong} differ")
        assert wrong == 0, (name, k, np.nonzero(got != want)[0][:8])


def test_rows_gather_argument_checks():
    """nine jobs, a size that is no multiple of 4 and src == dst are VIPE_EINVAL, and nothing is written"""
    L, _, stream_ptr = abi()
    good = gc.rows_launch("indices")
    for case in ("n_jobs", "size", "alias"):
        slots = (good * 5)[:9] if case == "n_jobs" else good
        arr, outs, keep = _rows_struct(slots)
        if case == "size":
            arr[1].seg_bytes = arr[1].seg_pitch = 6
        if case == "alias":
            arr[1].src = arr[1].dst
        assert L.vipe_rows_gather(ctypes.addressof(arr), len(slots), stream_ptr(outs[0][0])) == EINVAL, case
        torch.cuda.synchronize()
        for (dst, _), s in zip(outs, [s for s in slots if s.job is not None]):
            assert same_bits(dst, s.dst), case


# ---------------------------------------------------------------------------------- vipe_gather_nchw_to_nhwc_f16


def _nhwc_launch(jobs, n_rows, C, P):
    """jobs: [(src np [N,C,P], frame np or None, dst np [rows,P,ctot], ctot, coff, row0)] -> (return code, [dst tensors])"""
    from vipe_amd.slam.factor_graph import NhwcJob
    L, _, stream_ptr = abi()
    arr = (NhwcJob * len(jobs))()
    dsts, keep = [], []
    for j, (src, frame, dst, ctot, coff, row0) in zip(arr, jobs):
        s, f, d = T(src), T(frame), T(dst)
        j.src, j.frame, j.dst = s.data_ptr(), None if f is None else f.data_ptr(), d.data_ptr()
        j.dst_row_pitch, j.dst_ctot, j.dst_coff, j.dst_row0 = P * ctot, ctot, coff, row0
        dsts.append(d)
        keep += [s, f]
    rc = L.vipe_gather_nchw_to_nhwc_f16(ctypes.addressof(arr), len(jobs), n_rows, C, P, stream_ptr(dsts[0]))
    torch.cuda.synchronize()
    return rc, dsts


@pytest.mark.parametrize("C,P,ctot,coff", gc.NHWC_SINGLE)
def test_gather_nchw_to_nhwc_bit_exact(C, P, ctot, coff):
    """`nets[frame].permute(0, 2, 3, 1)` into a channel slice, for pixel counts on every side of the 64-pixel tile and
    channel counts that do and do not divide the workgroup; frames out of order with a repeat, rows behind dst_row0 > 0;
    the rows before and after and the channels outside the slice keep their sentinel"""
    src = gc.nhwc_src(C, P)
    dst = gc.nhwc_dst(gc.NHWC_ROW0 + len(gc.NHWC_FRAMES) + 1, P, ctot)
    rc, (out,) = _nhwc_launch([(src, gc.NHWC_FRAMES, dst, ctot, coff, gc.NHWC_ROW0)], len(gc.NHWC_FRAMES), C, P)
    assert rc == OK
    want = glue.nchw_to_nhwc_ref(dst, src, gc.NHWC_FRAMES, C, P, gc.NHWC_ROW0, ctot, coff)
    assert (want != dst).any() and same_bits(out, want)


def test_gather_nchw_to_nhwc_eight_jobs_and_null_frame():
    """one launch with eight jobs of different destination widths, offsets, first rows and frame lists; one launch without
    a frame list (row r reads frame r)"""
    C, P = gc.NHWC_MULTI_CP
    jobs = []
    for k, (ctot, coff, row0, frames) in enumerate(gc.NHWC_MULTI):
        jobs.append((gc.nhwc_src(C, P, seed=k % 2), np.array(frames, dtype=np.int64), gc.nhwc_dst(row0 + 4, P, ctot), ctot, coff, row0))
    rc, outs = _nhwc_launch(jobs, 3, C, P)
    assert rc == OK
    for out, (src, frames, dst, ctot, coff, row0) in zip(outs, jobs):
        assert same_bits(out, glue.nchw_to_nhwc_ref(dst, src, frames, C, P, row0, ctot, coff)), (ctot, coff)
    C, P, ctot, coff, row0, n_rows = gc.NHWC_NULL_FRAME
    src, dst = gc.nhwc_src(C, P), gc.nhwc_dst(row0 + n_rows + 1, P, ctot)
    rc, (out,) = _nhwc_launch([(src, None, dst, ctot, coff, row0)], n_rows, C, P)
    assert rc == OK and same_bits(out, glue.nchw_to_nhwc_ref(dst, src, None, C, P, row0, ctot, coff, n_rows=n_rows))


def test_gather_nchw_to_nhwc_limits():
    """C = 129 is VIPE_EUNSUPPORTED, no rows is VIPE_OK; neither writes"""
    P = 10
    src = np.zeros((gc.NHWC_N, 129, P), dtype=np.float16)
    dst = gc.nhwc_dst(4, P, 136)
    rc, (out,) = _nhwc_launch([(src, gc.NHWC_FRAMES, dst, 136, 0, 0)], len(gc.NHWC_FRAMES), 129, P)
    assert rc == EUNSUPPORTED and same_bits(out, dst)
    rc, (out,) = _nhwc_launch([(src, gc.NHWC_FRAMES, dst, 136, 0, 0)], 0, 128, P)
    assert rc == OK and same_bits(out, dst)


# ---------------------------------------------------------------------------------- vipe_segment_mean_nhwc_f16


@pytest.mark.parametrize("name", list(gc.SEG_LAYOUTS) + ["stride"])
def test_segment_mean_against_float64(name):
    """operator: the GraphAgg slice of the heads buffer (channels [256, 384) of 384, the others +-1000).  narrow: one
    eight-channel unit per row.  middle: 24 channels inside 40.  All three with segments of 2, 0, 37, 1 and 3 edges
    interleaved by `order`, the last with results in fp16's subnormal range.  stride: 262 400 units, more than 1024
    workgroups hold.  Per element |out - ref| <= 2^-11 |ref| + (n + 2) 2^-24 mean|inputs| + 2^-25 (oracle.glue.
    segment_mean_bound says where the terms come from); an empty segment is exactly zero; the row behind the output
    keeps its sentinel."""
    L, ptr, stream_ptr = abi()
    c = gc.segment_case(name)
    n_out = len(c.rowptr) - 1
    src, order, rowptr = T(c.src), T(c.order), T(c.rowptr)
    out = torch.full((n_out + 1, c.rows, c.C), float(gc.SENTINEL_F16), dtype=torch.float16, device=dev())
    assert L.vipe_segment_mean_nhwc_f16(ptr(src), c.ctot, c.coff, ptr(order), ptr(rowptr), ptr(out), n_out, c.rows, c.C,
                                        stream_ptr(src)) == OK
    got = out.cpu().numpy()
    assert np.all(got[n_out] == gc.SENTINEL_F16)
    ref = glue.segment_mean_ref(c.src, c.ctot, c.coff, c.order, c.rowptr, c.C)
    bound = glue.segment_mean_bound(c.src, c.ctot, c.coff, c.order, c.rowptr, c.C)
    err = np.abs(got[:n_out].astype(np.float64) - ref)
    print(f"segment_mean {name}: max err / bound = {(err / bound).max():.3f}, max |err| = {err.max():.3e}")
    assert np.all(err <= bound), (name, (err / bound).max())
    for k in np.nonzero(np.diff(c.rowptr) == 0)[0]:
        assert np.all(got[k].view(np.uint16) == 0)


def test_segment_mean_no_outputs():
    L, ptr, stream_ptr = abi()
    c = gc.segment_case("narrow")
    src, order, rowptr = T(c.src), T(c.order), T(c.rowptr)
    out = torch.full((2, c.rows, c.C), float(gc.SENTINEL_F16), dtype=torch.float16, device=dev())
    assert L.vipe_segment_mean_nhwc_f16(ptr(src), c.ctot, c.coff, ptr(order), ptr(rowptr), ptr(out), 0, c.rows, c.C,
                                        stream_ptr(src)) == OK
    torch.cuda.synchronize()
    assert bool((out == float(gc.SENTINEL_F16)).all())


# ------------------------------------------------------------------------------------------------ vipe_glo_context


def _glo(glo_sum, wT, bias, hw):
    """-> extra [E, 384] as numpy; the row behind it must keep its sentinel"""
    L, ptr, stream_ptr = abi()
    E = glo_sum.shape[0]
    extra = torch.full((E + 1, 384), float(gc.SENTINEL_F32), device=dev())
    assert L.vipe_glo_context(ptr(glo_sum), ptr(wT), ptr(bias), ptr(extra), E, hw, stream_ptr(extra)) == OK
    got = extra.cpu().numpy()
    assert np.all(got[E] == gc.SENTINEL_F32)
    return got[:E].astype(np.float64)


@pytest.mark.parametrize("E", gc.GLO_E)
def test_glo_context_against_float64(E):
    """bias + (glo_sum / hw) @ wT for hw = 1, 3, 45 and 3072 within 132 x 2^-24 (|bias| + sum_k |g_k w_k|) per output: 128
    fused multiply-adds, the rounded 1 / hw and its product"""
    for hw in gc.GLO_HW:
        c = gc.glo_case(E, hw)
        got = _glo(T(c.glo_sum), T(c.wT), T(c.bias), hw)
        err = np.abs(got - glue.glo_context_ref(c.glo_sum, c.wT, c.bias, hw))
        bound = glue.glo_context_bound(c.glo_sum, c.wT, c.bias, hw)
        print(f"glo_context E={E} hw={hw}: max err / bound = {(err / bound).max():.3f}")
        assert np.all(err <= bound), (E, hw, (err / bound).max())


def test_glo_context_weight_packing_is_z_r_q():
    """`UpdateEngine.glo_w` / `glo_b` of a seeded update module through the entry point, against the module's three *_glo
    1x1 convolutions evaluated in float64 on the pooled vector: columns [0,128) are z, [128,256) r, [256,384) q.  The
    gates' weights and biases differ, and their outputs differ by far more than the bound, so no other order passes."""
    from vipe_amd.slam.networks import UpdateModule
    from vipe_amd.slam.update_engine import UpdateEngine
    torch.manual_seed(0)
    um = UpdateModule().eval()
    eng = UpdateEngine(um, dev())
    assert tuple(eng.glo_w.shape) == (128, 384) and eng.glo_w.is_contiguous() and tuple(eng.glo_b.shape) == (384,)
    hw = 45
    glo_sum = gc.glo_case(5, hw).glo_sum
    got = _glo(T(glo_sum), eng.glo_w, eng.glo_b, hw)
    g = glo_sum.astype(np.float64) / hw
    gates = [um.gru.convz_glo, um.gru.convr_glo, um.gru.convq_glo]
    refs, bounds = [], []
    for conv in gates:
        W = conv.weight.detach().double().numpy().reshape(128, 128)  # [out, in]
        b = conv.bias.detach().double().numpy()
        refs.append(b[None] + g @ W.T)
        bounds.append(132 * 2.0 ** -24 * (np.abs(b)[None] + np.abs(g) @ np.abs(W.T)))
    for a in range(3):
        for b_ in range(a + 1, 3):
            assert not torch.equal(gates[a].weight, gates[b_].weight) and not torch.equal(gates[a].bias, gates[b_].bias)
            assert np.abs(refs[a] - refs[b_]).max() > 1000 * bounds[a].max()
    for k, name in enumerate("zrq"):
        err = np.abs(got[:, 128 * k:128 * (k + 1)] - refs[k])
        print(f"glo_context packing gate {name}: max err / bound = {(err / bounds[k]).max():.3f}")
        assert np.all(err <= bounds[k]), name


# ------------------------------------------------------------------------------------------------ vipe_update_finish


def _finish_buffers(c):
    """sentinel-filled target / weight with one spare edge behind them -> (whole buffers, the [1,E,h,w,2] views)"""
    n = c.E * c.h * c.w * 2
    whole = [torch.full((n + c.h * c.w * 2,), float(gc.SENTINEL_F32), device=dev()) for _ in range(2)]
    return whole, [b[:n].view(1, c.E, c.h, c.w, 2) for b in whole]


def _finish_check(c, whole, damping):
    t, w, d = glue.update_finish_ref(c.coords1, c.dw, c.mask, c.eta, c.du, c.damping)
    tail = np.full(c.h * c.w * 2, gc.SENTINEL_F32, dtype=np.float32)
    assert same_bits(whole[0], np.concatenate([t.reshape(-1), tail])), "target"
    assert same_bits(whole[1], np.concatenate([w.reshape(-1), tail])), "weight"
    assert same_bits(damping, d), "damping"
    if c.mask is not None:
        wm = bits(whole[1], torch.int32)[:c.E * c.h * c.w * 2].view(c.E, c.h, c.w, 2)[torch.from_numpy(c.mask)]
        assert wm.numel() > 0 and bool((wm == 0).all())  # exactly +0
    if c.du is not None:
        outside = np.setdiff1d(np.arange(c.damping.shape[0]), c.du)
        assert same_bits(damping[torch.from_numpy(outside).to(damping.device)], c.damping[outside])


@pytest.mark.parametrize("E,h,w", gc.UF_GRIDS)
@pytest.mark.parametrize("sources", ["none", "fewer", "equal"])
@pytest.mark.parametrize("masked", [False, True])
def test_update_finish_bit_exact(E, h, w, sources, masked):
    """`slam_ext.update_finish` bit for bit: target = coords1 + delta, weight = w with the masked pixels exactly +0,
    damping[du] = eta with du no identity and the other damping rows as they were; without eta maps, with fewer than and
    as many as edges; 225 pixels (under one workgroup) and 777 (a partial last one)"""
    from vipe_amd.ext import slam_ext
    du = gc.UF_DU[E][sources]
    c = gc.finish_case(E, h, w, None if du is None else tuple(du), masked)
    whole, (target, weight) = _finish_buffers(c)
    damping = T(c.damping)
    slam_ext.update_finish(T(c.coords1), T(c.dw), T(c.mask), target, weight, T(c.eta), T(c.du), damping)
    _finish_check(c, whole, damping)


def test_update_finish_more_sources_than_edges_and_no_edges():
    """through the ABI: E = 1 with three eta maps (the launch is sized by them) - the edge's target / weight and all three
    damping rows; E = 0 is VIPE_OK and touches nothing"""
    L, ptr, stream_ptr = abi()
    (E, h, w), du = gc.UF_MORE
    c = gc.finish_case(E, h, w, tuple(du), True)
    whole, _ = _finish_buffers(c)
    damping = T(c.damping)
    args = [T(c.coords1), T(c.dw), T(c.mask), whole[0], whole[1], T(c.eta), T(c.du), damping]
    assert L.vipe_update_finish(*[ptr(a) for a in args], 0, len(du), h, w, stream_ptr(damping)) == OK
    torch.cuda.synchronize()
    assert bool((whole[0] == float(gc.SENTINEL_F32)).all()) and bool((whole[1] == float(gc.SENTINEL_F32)).all())
    assert same_bits(damping, c.damping)
    assert L.vipe_update_finish(*[ptr(a) for a in args], E, len(du), h, w, stream_ptr(damping)) == OK
    _finish_check(c, whole, damping)


# ------------------------------------------------------------------------------------------------ vipe_flow_score


@pytest.mark.parametrize("V,P", gc.FLOW_SIZES)
@pytest.mark.parametrize("magnitude", gc.FLOW_MAGNITUDES)
def test_flow_score_against_float64(V, P, magnitude):
    """per view within (ceil(P / 256) + 16) 2^-23 of the float64 score of the fp16-rounded deltas (the per-lane
    sequential sum, nine reduction steps, square / add / sqrtf per term, two divisions).  `large` deltas lose 0.9 - 1 per
    component to that rounding, > 100 bounds (tests/test_oracle_glue.py).  Without a mask, with a random one, with view 0
    wholly invalid (exactly 0) and with the last view wholly valid under a mask (divisor 1 + 1e-6); once more with NaN
    in the weight channels, which must not be read."""
    L, ptr, stream_ptr = abi()
    for mask in gc.FLOW_MASKS:
        for nan_weights in (False, True):
            c = gc.flow_case(V, P, magnitude, mask, nan_weights)
            dw, invalid = T(c.dw), T(c.invalid)
            score = torch.full((V + 1,), float(gc.SENTINEL_F32), device=dev())
            assert L.vipe_flow_score(ptr(dw), ptr(invalid), ptr(score), V, P, stream_ptr(dw)) == OK
            got = score.cpu().numpy()
            assert got[V] == gc.SENTINEL_F32
            ref = glue.flow_score_ref(c.dw, c.invalid)
            bound = glue.flow_score_bound(ref, P)
            err = np.abs(got[:V].astype(np.float64) - ref)
            ratio = (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0
            print(f"flow_score V={V} P={P} {magnitude} {mask} nan={nan_weights}: max err / bound = {ratio:.3f}")
            assert np.isfinite(got[:V]).all() and np.all(err <= bound), (mask, nan_weights, got[:V], ref)
            if mask == "first_invalid":
                assert got[0] == 0.0 and not np.signbit(got[0])
