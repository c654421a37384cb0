"""The tile convolutions' fused epilogues (conv_halo32_kernel, conv_halo32_narrow_kernel, conv1x1_glo_kernel of
csrc/conv_mfma.hip) against the float64 restatement in oracle/conv_epilogues.py.

Every case is ONE `vipe_conv2d_fused` launch exactly as csrc/update_op.hip issues it - the operator's buffers with their
channel pitches and offsets (oracle/conv_epilogue_cases.py::LAUNCHES) - on the smallest grids at which each tiling can go
wrong: two aligned ones (4 x 64 tiles) and four of the flat tiling.  Every output tensor has one guard image before and
after and is filled with a canary: nothing but the named channels of the named pixels may change (on the flat grids a
stored pad position would land on the next pixel or in the guard).  The bounds are those stated next to the reference
functions; tests/test_oracle_conv_epilogues.py shows on these very inputs what they tell apart.

Measured on the MI355X when these tests were written (every case prints its figures, `pytest -s`): every fp16 output of
every launch and grid at most ONE fp16 step from the rounded float64 value (4.9e-4 below 1, 9.8e-4 for the relu outputs
in [2, 4)) with no element beyond the two-step bound; PARTIAL at 0.2 % of its bound (2.3e-6); the global-context sums at
0.2 - 2 % of the loose bound and 0.02 - 1.1 % of the exact one; eta above the softplus threshold at half an fp16 step of
[16, 32) (7.8e-3, 0.8 of its bound).
"""

import copy

import numpy as np
import pytest
import torch

from oracle import conv_epilogue_cases as cases
from oracle import conv_epilogues as oce

pytestmark = pytest.mark.gpu

ACT = {"none": 0, "relu": 1, "sigmoid": 2, "tanh": 3}
ACCINIT_F32 = 0x100
CANARY16, CANARY32 = 7.0, -12345.5
SMALLEST = [(1, 4, 128), (3, 5, 7)]  # the smallest grid of each tiling


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def gid(grid):
    return "%dx%dx%d" % grid


def run(grid, L, bufs=None, wb=None, bias=None, raw=False):
    """One launch `L` (a record of cases.LAUNCHES) on `grid` -> the outputs as CPU tensors in the order of
    cases.reference (GLO: fout AFTER the launch, prefill included).  `bias`: a device tensor to pass instead of the packed
    one.  Checks the guard images and the spare channels of every output.  raw: the whole output tensors, guards and all."""
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    from vipe_amd.slam.update_engine import _Packed
    B, H, W = grid
    bufs = cases.buffers(grid) if bufs is None else bufs
    w, b = cases.weights(_name(L)) if wb is None else wb
    pk = _Packed(w, b, dev())

    on_dev = {}

    def up(name):  # one device copy per buffer: the global-context kernel is taken when `net` IS the input tensor
        if name is not None and name not in on_dev:
            on_dev[name] = bufs[name].to(dev())
        return on_dev.get(name)

    def pitch(t):
        return 0 if t is None else t.shape[-1]

    x0, x1 = up(L.x0[0]), up(L.x1[0] if L.x1 else None)
    extra = up("extra" if L.extra_off is not None else None)
    init, net, z = up(L.init[0] if L.init else None), up(L.net), up(L.z)
    y = y2 = fout = None
    if L.mode in ("plain", "zr", "q"):
        y = torch.full((B + 2, H, W, L.y[0]), CANARY16, dtype=torch.float16, device=dev())
    if L.mode == "zr":
        y2 = torch.full((B + 2, H, W, L.y2[0]), CANARY16, dtype=torch.float16, device=dev())
    if L.mode == "glo":
        fout = bufs["glo_prefill"].to(dev())
    elif L.mode in ("heads", "eta", "partial"):
        shape = {"heads": (B + 2, H, W, 4), "eta": (B + 2, H, W), "partial": (B + 2, H, W, L.y[0] if L.y else 0)}[L.mode]
        fout = torch.full(shape, CANARY32, dtype=torch.float32, device=dev())
    mode = cases.MODE[L.mode] | (ACCINIT_F32 if init is not None and init.dtype == torch.float32 else 0)
    inner = [None if t is None else t[1:] for t in (y, y2, fout)]
    check(lib().vipe_conv2d_fused(
        ptr(x0), pitch(x0), L.x0[1], ptr(x1), pitch(x1), L.x1[1] if L.x1 else 0, L.split,
        ptr(pk.packed), ptr(pk.bias if bias is None else bias), ptr(extra), pitch(extra), L.extra_off or 0,
        ptr(inner[0]), L.y[0] if L.y else 0, L.y[1] if L.y else 0, ptr(inner[1]), L.y2[0] if L.y2 else 0, L.y2[1] if L.y2 else 0,
        ptr(net), pitch(net), 0, ptr(z), ptr(inner[2]), ptr(init), pitch(init), L.init[1] if L.init else 0,
        B, H, W, L.cin, L.cout, L.k, L.k, ACT[L.act], mode, stream_ptr(x0)), "conv2d_fused %s" % L.mode)
    torch.cuda.synchronize()
    y, y2, fout = [None if t is None else t.cpu() for t in (y, y2, fout)]
    if raw:
        return [t for t in (y, y2, fout) if t is not None]
    outs = []
    for t, spec in ((y, L.y), (y2, L.y2)):
        if t is None:
            continue
        n, off = (L.cout if L.mode == "plain" else 128), spec[1]
        assert bool((t[0] == CANARY16).all()) and bool((t[-1] == CANARY16).all()), "guard image written"
        assert bool((t[..., :off] == CANARY16).all()) and bool((t[..., off + n:] == CANARY16).all()), "spare channels written"
        outs.append(t[1:-1, ..., off:off + n])
    if fout is not None:
        guard = bufs["glo_prefill"] if L.mode == "glo" else torch.full_like(fout, CANARY32)
        assert torch.equal(fout[0], guard[0]) and torch.equal(fout[-1], guard[-1]), "guard image written"
        outs.append(fout[1:-1])
    return outs


def _name(L):
    return next(k for k, v in cases.LAUNCHES.items() if v is L or v is getattr(L, "base", None))


def variant(name, **kw):
    """a launch of the table with something replaced (its seeded weights stay those of `name`)"""
    L = copy.copy(cases.LAUNCHES[name])
    L.base = cases.LAUNCHES[name]
    for k, v in kw.items():
        setattr(L, k, v)
    return L


def fig(tag, grid, kernel, output, err, against):
    """one figure line per output, printed before anything is asserted (`pytest -s` shows them)"""
    print("FIG | %s | %s | %s | %s | max err %.3e | %s" % (tag, gid(grid), kernel, output, err, against))


def check_outputs(tag, L, o, outs, grid, raw=None):
    """the bounds of oracle/conv_epilogues.py; prints one figure line per output before it asserts"""
    B, H, W = grid
    kern = cases.expected_kernel(_name(L), grid)
    if L.mode == "partial":
        ref = cases.reference(o, rounded=False, raw=raw)[0]
        ratio = float(((outs[0].double() - ref).abs() / oce.partial_bound(o.x, o.w, o.init, o.init_off)).max())
        fig(tag, grid, kern, "fout", float((outs[0].double() - ref).abs().max()), "%.4f of the bound" % ratio)
        assert ratio <= 1.0, (tag, grid, ratio)
        return
    if L.mode == "glo":
        pre = cases.buffers(grid)["glo_prefill"][1:-1]
        ref = pre.double() + cases.reference(o, raw=raw)[0]
        err = (outs[0].double() - ref).abs()
        ratio = float((err / oce.glo_bound(oce.glo_terms(o.x, o.w, o.b, o.net, raw=raw), H * W, pre)).max())
        fig(tag, grid, kern, "fout", float(err.max()), "%.4f of the bound" % ratio)
        assert ratio <= 1.0, (tag, grid, ratio)
        return
    scale = 0.01 if L.mode == "eta" else 1.0
    fails = []
    for what, got, ref in zip(("y", "y2"), outs, cases.reference(o, raw=raw)):
        assert bool(torch.isfinite(got).all()), (tag, grid, what)
        err, share = oce.fp16_errors(got.double() / scale, ref / scale)
        fig(tag, grid, kern, what, err, "share over two steps %.2e" % share)
        if not (err <= oce.FP16_CAP and share <= oce.FP16_SHARE):
            fails.append((what, err, share))
    assert not fails, (tag, grid, fails)


LAUNCH_CASES = [(name, grid) for name in cases.LAUNCHES for grid in cases.launch_grids(name)]


@pytest.mark.parametrize("name,grid", LAUNCH_CASES, ids=["%s-%s" % (n, gid(g)) for n, g in LAUNCH_CASES])
def test_operator_launch_against_float64_reference(name, grid):
    """Every launch of the table on every grid: fp16 outputs within 4e-3 and at most 0.1 % of an output beyond two fp16
    steps; PARTIAL within (K + 1) 2^-24 (|init| + sum |x w|); GLO within 2^-10 sum |sigmoid net| (+ the prefilled fout)."""
    L = cases.LAUNCHES[name]
    check_outputs(name, L, cases.operands(grid, name), run(grid, L), grid, raw=cases.conv_sum(grid, name))


@pytest.mark.parametrize("grid", cases.GRIDS, ids=gid)
@pytest.mark.parametrize("name", ["glo_net", "glo_x"])
def test_global_context_sum_with_zero_weights_counts_every_pixel_once(name, grid):
    """Zero weights and zero bias: every term is exactly 0.5 net, the sum is bounded by its float32 order alone -
    (n + 1) 2^-24 (|prefill| + sum |0.5 net|).  A dropped short last tile, a pixel counted twice, or a `=` for the `+=`
    into the prefilled fout is tens of bounds away."""
    L = cases.LAUNCHES[name]
    o = cases.operands(grid, name)
    wb = (torch.zeros_like(o.w), torch.zeros_like(o.b))
    pre = cases.buffers(grid)["glo_prefill"][1:-1]
    got = run(grid, L, wb=wb)[0]
    err = (got.double() - (pre.double() + 0.5 * o.net.double().sum((1, 2)))).abs()
    ratio = float((err / oce.glo_exact_bound(o.net, pre)).max())
    fig(name + " exact", grid, cases.expected_kernel(name, grid), "fout", float(err.max()), "%.4f of the bound" % ratio)
    assert ratio <= 1.0, (name, grid, ratio)


@pytest.mark.parametrize("grid", SMALLEST, ids=gid)
def test_saturated_update_and_reset_gates_are_exactly_0_or_1(grid):
    """`extra` = +-40 on some channels of z and of r: the sigmoid is exactly 1 or 0 there, so z is and r * net is bit-equal
    to net or zero; every other channel still meets the reference built from the same `extra`."""
    bufs = dict(cases.buffers(grid))
    extra = bufs["extra"].clone()
    extra[:, 0:16], extra[:, 16:32], extra[:, 128:144], extra[:, 144:160] = 40.0, -40.0, 40.0, -40.0
    bufs["extra"] = extra
    L = cases.LAUNCHES["zr_ctx"]
    z, rnet = run(grid, L, bufs=bufs)
    net = bufs["net"]
    assert bool((z[..., 0:16] == 1.0).all()) and bool((z[..., 16:32] == 0.0).all())
    assert torch.equal(rnet[..., 0:16].view(torch.int16), net[..., 0:16].view(torch.int16))
    assert bool((rnet[..., 16:32] == 0.0).all())
    check_outputs("zr_ctx saturated", L, cases.operands(grid, "zr_ctx", bufs=bufs), [z, rnet], grid,
                  raw=cases.conv_sum(grid, "zr_ctx"))


@pytest.mark.parametrize("grid", SMALLEST, ids=gid)
def test_saturated_blend_copies_the_hidden_state_or_the_candidate(grid):
    """z exactly 0: the new hidden state is bit-equal to `net`; z exactly 1: bit-equal to h16(tanh(.)) - read off the same
    convolution launched with the plain tanh epilogue, and exactly +-1 where `extra` = +-40 saturates the tanh."""
    bufs = dict(cases.buffers(grid))
    z = bufs["z"].clone()
    z[..., 0:16], z[..., 16:48] = 0.0, 1.0
    extra = bufs["extra"].clone()
    extra[:, 256 + 32:256 + 40], extra[:, 256 + 40:256 + 48] = 40.0, -40.0
    bufs["z"], bufs["extra"] = z, extra
    L = cases.LAUNCHES["q_ctx"]
    h = run(grid, L, bufs=bufs)[0]
    cand = run(grid, variant("q_ctx", mode="plain", act="tanh", net=None, z=None), bufs=bufs)[0]
    net = bufs["net"]
    assert torch.equal(h[..., 0:16].view(torch.int16), net[..., 0:16].view(torch.int16))
    assert torch.equal(h[..., 16:48].view(torch.int16), cand[..., 16:48].view(torch.int16))
    assert bool((h[..., 32:40] == 1.0).all()) and bool((h[..., 40:48] == -1.0).all())
    o = cases.operands(grid, "q_ctx", bufs=bufs)
    check_outputs("q_ctx saturated", L, o, [h], grid, raw=cases.conv_sum(grid, "q_ctx"))
    oc = copy.copy(o)
    oc.mode, oc.act = "plain", "tanh"
    check_outputs("q_ctx candidate", variant("q_ctx", mode="plain"), oc, [cand], grid, raw=cases.conv_sum(grid, "q_ctx"))


@pytest.mark.parametrize("grid", SMALLEST, ids=gid)
def test_eta_above_the_softplus_threshold(grid):
    """bias 25: every pre-activation v lies above 20, where the kernel returns v itself.  The output is 0.01f * h for an
    fp16 value h (bit for bit), and h is the rounding of v: |h - v| <= 2^-7 (half an fp16 step in [16, 32)) +
    (K + 2) 2^-24 (25 + sum |x w|) for the float32 sum.  (The 4e-3 cap of the other cases does not apply at this
    magnitude: half a step alone is 7.8e-3.)"""
    L = cases.LAUNCHES["eta"]
    w, _ = cases.weights("eta")
    wb = (w, torch.tensor([25.0]))
    got = run(grid, L, wb=wb)[0]
    o = cases.operands(grid, "eta", wb=wb)
    v = oce.preactivation(o.x, o.w, o.b, raw=cases.conv_sum(grid, "eta"))[..., 0]
    assert float(v.min()) > 20.0 and float(v.max()) < 32.0
    h = (got.double() / 0.01).numpy().astype(np.float16)
    assert np.array_equal(got.numpy(), np.float32(0.01) * h.astype(np.float32)), "not 0.01f * (an fp16 value)"
    err = (torch.from_numpy(h.astype(np.float64)) - v).abs()
    bound = 2.0 ** -7 + oce.partial_bound(o.x, o.w)[..., 0] + (o.w[0].numel() + 2) * oce.U32 * 25.0
    fig("eta bias 25", grid, cases.expected_kernel("eta", grid), "fout", float(err.max()),
        "%.4f of the bound" % float((err / bound).max()))
    assert bool((err <= bound).all()), (grid, float(err.max()))
    assert oce.fp16_errors(got.double() / 0.01, cases.reference(o, raw=cases.conv_sum(grid, "eta"))[0] / 0.01)[1] == 0.0


@pytest.mark.parametrize("grid", SMALLEST, ids=gid)
@pytest.mark.parametrize("name", ["heads", "eta", "plain_upmask"])
def test_bias_values_behind_cout_are_ignored(name, grid):
    """The tile kernels load the bias up to the padded output-channel count (16 floats for the 4 of HEADS and the 1 of ETA,
    640 for the 576 of the upsampling mask): include/vipe_amd.h asks for a buffer readable that far and promises that the
    values behind Cout are ignored.  The bias is a view into the middle of a larger tensor whose floats from Cout to the
    padded count are NaN: the outputs are bit-equal to the run with the zero tail of `_Packed`."""
    from vipe_amd.slam.update_engine import _Packed
    L = cases.LAUNCHES[name]
    w, b = cases.weights(name)
    pad = _Packed(w, b, dev()).bias.numel()
    assert pad > L.cout and pad == {4: 32, 1: 32, 576: 640}[L.cout]
    big = torch.zeros(64 + pad + 64, dtype=torch.float32, device=dev())
    big[64:64 + L.cout] = b.to(dev())
    big[64 + L.cout:64 + pad] = float("nan")
    want = run(grid, L, raw=True)
    got = run(grid, L, bias=big[64:], raw=True)
    assert len(want) == len(got) == 1 and bool(torch.isfinite(got[0].float()).all())
    assert torch.equal(got[0], want[0])


def test_packed_bias_is_padded_with_zeros():
    """`_Packed` hands every convolution entry point a bias buffer of the padded output-channel count"""
    import ctypes
    from vipe_amd._lib import check, lib
    from vipe_amd.slam.update_engine import _Packed
    for cout, cin, k in ((4, 256, 3), (1, 128, 3), (576, 128, 1), (128, 200, 1), (64, 128, 3), (384, 128, 3)):
        cp = ctypes.c_int()
        check(lib().vipe_conv_packed_dims(cout, cin, k, k, ctypes.addressof(cp), None, None), "conv_packed_dims")
        b = torch.arange(1, cout + 1, dtype=torch.float32)
        pk = _Packed(torch.zeros(cout, cin, k, k).half(), b, dev())
        assert pk.bias.numel() == cp.value and torch.equal(pk.bias[:cout].cpu(), b) and not bool(pk.bias[cout:].any())
