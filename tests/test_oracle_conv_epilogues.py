"""oracle/conv_epilogues.py checked on the CPU: (i) its unrounded functions chained in operator order ARE
oracle/update_module.py::update_forward (pinned to the reference class by tests/test_oracle_golden.py), in the unsplit
form and in the gate-split forms; (ii) on the very inputs tests/test_gpu_conv_epilogues.py feeds the tile kernels, every
mistake an epilogue can make moves an output by at least ten times the bound the kernel is held to; (iii) a float32
evaluation of the same restatement stays inside those bounds, so the reference alone does not use them up."""

import copy

import pytest
import torch

from oracle import conv_epilogue_cases as cases
from oracle import conv_epilogues as oce
from oracle import update_module as oum


# ------------------------------------------------------------------------------------------------ helpers
def test_rounding_helpers_on_hand_worked_numbers():
    # 1 + 2^-11 + 2^-30 lies above the tie between 1 and 1 + 2^-10: a conversion through float32 would round it to the tie
    # first and then to even (1.0)
    t = torch.tensor([1.0 + 2.0 ** -11 + 2.0 ** -30, 0.1, -3.0004], dtype=torch.float64)
    assert oce.h16(t).tolist() == [1.0 + 2.0 ** -10, float(torch.tensor(0.1).half()), -3.0]
    ref = torch.tensor([0.0, 0.3, 1.0, 1.5, 2.0, 3.0, -5.0])
    assert oce.two_step(ref).tolist() == [2.0 ** -10 * s for s in (1, 1, 1, 2, 2, 4, 8)]
    got = ref + torch.tensor([0.0, 2.0 ** -10, 2.0 ** -9, 0.0, 0.0, 0.0, 0.0])
    err, share = oce.fp16_errors(got, ref)
    assert err == 2.0 ** -9 and share == 1.0 / 7.0 and not oce.fp16_ok(got, ref)
    v = torch.tensor([-30.0, 0.0, 19.0, 25.0], dtype=torch.float64)
    assert torch.allclose(oce.softplus(v), torch.nn.functional.softplus(v), rtol=0, atol=3e-9)


# ------------------------------------------------------------------------------------------------ (i) chaining
def _nhwc(t):
    return t[0].permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("form", ["unsplit", "context", "staged"])
def test_unrounded_functions_chain_into_update_forward(form):
    """GLO -> mean -> the three *_glo 1x1s -> ZR -> Q -> heads0 -> HEADS, and agg2 -> ETA, with the weights of a seeded
    UpdateModule assembled as vipe_amd/slam/update_engine.py assembles them, on a 6 x 9 grid with E = 2.  `context`: the
    gate convolutions start from pgate = conv(inp) (gate-context hoisting); `staged`: additionally PARTIAL -> ZR with the
    float32-typed initial accumulators.  Bound: float64 round-off - sums of at most 4032 products of magnitude <= 1 are
    good to ~4032 x 2^-53 ~ 5e-13 per layer, eight layers, slopes <= 1: 1e-11."""
    from vipe_amd.slam.networks import UpdateModule
    torch.manual_seed(0)
    sd = {k: v.double() for k, v in UpdateModule().eval().state_dict().items()}
    E, H, W = 2, 6, 9
    g = torch.Generator().manual_seed(7)
    net = torch.randn(1, E, 128, H, W, generator=g).tanh().double()
    inp = torch.randn(1, E, 128, H, W, generator=g).relu().double()
    corr = (torch.randn(1, E, 196, H, W, generator=g) * 0.5).double()
    flow = (torch.randn(1, E, 4, H, W, generator=g) * 2).double()
    ix = torch.tensor([0, 0])
    with torch.no_grad():
        net_r, delta_r, weight_r, eta_r, _ = oum.update_forward(sd, net, inp, corr, flow, ix)

    def wb(name):
        return sd[name + ".weight"], sd[name + ".bias"]

    kw = dict(rounded=False)
    n = _nhwc(net)
    c = oce.plain(oce.plain(_nhwc(corr), *wb("corr_encoder.0"), "relu", **kw), *wb("corr_encoder.2"), "relu", **kw)
    f = oce.plain(oce.plain(_nhwc(flow), *wb("flow_encoder.0"), "relu", **kw), *wb("flow_encoder.2"), "relu", **kw)
    xbuf = torch.cat([_nhwc(inp), c, f], -1)
    pooled = oce.glo(n, *wb("gru.w"), n, **kw) / (H * W)
    glo_w = torch.cat([sd["gru.conv%s_glo.weight" % s].reshape(128, 128) for s in "zrq"], 0)
    extra = torch.cat([sd["gru.conv%s_glo.bias" % s] for s in "zrq"], 0)[None] + pooled @ glo_w.t()
    (wz, bz), (wr, br), (wq, bq) = wb("gru.convz"), wb("gru.convr"), wb("gru.convq")
    wzr, bzr = torch.cat([wz, wr], 0), torch.cat([bz, br], 0)
    rest = list(range(0, 128)) + list(range(256, 448))
    if form == "unsplit":
        z, rnet = oce.zr((n, xbuf, 128), wzr, bzr, n, extra, 0, **kw)
        h = oce.q((rnet, xbuf, 128), wq, bq, n, z, extra, 256, **kw)
    else:
        pgate = oce.plain(xbuf[..., :128], torch.cat([wz, wr, wq], 0)[:, 128:256], torch.zeros(384), **kw)
        if form == "context":
            z, rnet = oce.zr((n, xbuf[..., 128:], 128), wzr[:, rest], bzr, n, extra, 0, init=pgate, init_off=0, **kw)
        else:
            pzr = oce.partial(n, wzr[:, :128], init=pgate, init_off=0, **kw)
            z, rnet = oce.zr(xbuf[..., 128:], wzr[:, 256:], bzr, n, extra, 0, init=pzr, init_off=0, **kw)
        h = oce.q((rnet, xbuf[..., 128:], 128), wq[:, rest], bq, n, z, extra, 256, init=pgate, init_off=256, **kw)
    w0 = torch.cat([sd["delta.0.weight"], sd["weight.0.weight"], sd["agg.conv1.weight"]], 0)
    b0 = torch.cat([sd["delta.0.bias"], sd["weight.0.bias"], sd["agg.conv1.bias"]], 0)
    hbuf = oce.plain(h, w0, b0, "relu", **kw)
    w2 = torch.zeros(4, 256, 3, 3, dtype=torch.float64)
    w2[0:2, 0:128] = sd["delta.2.weight"][:2]
    w2[2:4, 128:256] = sd["weight.2.weight"][:2]
    dw = oce.heads(hbuf[..., :256], w2, torch.cat([sd["delta.2.bias"][:2], sd["weight.2.bias"][:2]], 0), **kw)
    agg = oum.scatter_mean(hbuf[None, ..., 256:], ix)[0]
    et = oce.eta(oce.plain(agg, *wb("agg.conv2"), "relu", **kw), *wb("agg.eta.0"), **kw)
    bound = 1e-11
    assert float((h - _nhwc(net_r)).abs().max()) < bound
    assert float((dw[..., :2] - delta_r[0]).abs().max()) < bound
    assert float((dw[..., 2:] - weight_r[0]).abs().max()) < bound
    assert float((et - eta_r[0]).abs().max()) < bound


# ------------------------------------------------------------------------------------------------ (ii) discrimination
def _mut(o, **kw):
    m = copy.copy(o)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _shifted(t, halves):
    """what a kernel reads through a channel offset that is `halves` too large"""
    return torch.roll(t.flatten(), -halves).view_as(t)


def _pad_leak(o):
    """the contribution of the pad column if it held the next row's first pixel (as its left neighbour's right border)
    and the previous row's last pixel (as its right neighbour's left border) instead of zeros: the flat tiling without
    its pad position.  Convolution of an image that is zero but for those two columns -> an additive pre-activation term"""
    x = oce._input(o.x, o.w.shape[1]).double()
    B, H, W, C = x.shape
    wide = torch.zeros(B, H, W + 2, C, dtype=torch.float64)
    wide[:, :-1, W + 1] = x[:, 1:, 0]    # right border of row y: first pixel of row y + 1
    wide[:, 1:, 0] = x[:, :-1, W - 1]    # left border of row y: last pixel of row y - 1
    return oce.conv_sum(wide, o.w)[:, :, 1:W + 1]


def _margin(o, ref, mut, bound=None):
    """largest movement of an output in units of the bound its kernel is held to (fp16 outputs: the 4e-3 cap)"""
    best = 0.0
    for r, m in zip(ref, mut):
        d = (m.double() - r.double()).abs()
        if o.mode == "eta":
            d = d / 0.01
        best = max(best, float((d / (oce.FP16_CAP if bound is None else bound)).max()))
    return best


@pytest.mark.parametrize("grid", cases.GRIDS)
def test_reference_tells_epilogue_mistakes_apart(grid):
    """Each mutation of the reference moves at least one output by >= 10 x the bound of its kernel."""
    B, H, W = grid
    flat = grid in cases.GRIDS_FLAT
    margins = {}

    def note(name, what, o, mut, bound=None, ref=None):
        ref = cases.reference(o, raw=cases.conv_sum(grid, name)) if ref is None else ref
        margins[(name, what)] = _margin(o, ref, mut, bound)

    def ref_of(name, o):
        return cases.reference(o, raw=cases.conv_sum(grid, name))

    for name in ("zr", "zr_ctx", "zr_staged", "q", "q_ctx"):
        o = cases.operands(grid, name)
        note(name, "extra dropped", o, ref_of(name, _mut(o, extra=None)))
        note(name, "extra_off shifted by 128", o, ref_of(name, _mut(o, extra_off=128)))
        if B > 1:
            note(name, "extra rows rolled by one image", o, ref_of(name, _mut(o, extra=torch.roll(o.extra, 1, 0))))
        note(name, "net read 8 channels off", o, ref_of(name, _mut(o, net=_shifted(o.net, 8))))
    for name in ("zr_ctx", "q_ctx"):
        o = cases.operands(grid, name)
        note(name, "initial accumulator at channel offset 128", o, ref_of(name, _mut(o, init_off=128)))
    for name in ("zr", "zr_ctx", "zr_staged"):
        o = cases.operands(grid, name)
        z, rn = ref_of(name, o)
        s = oce.h16(torch.sigmoid(oce.preactivation(o.x, o.w, o.b, o.extra, o.extra_off, o.init, o.init_off,
                                                     raw=cases.conv_sum(grid, name))))
        note(name, "halves swapped", o, (s[..., 128:], oce.h16(s[..., :128] * o.net.double())), ref=(z, rn))
    for name in ("q", "q_ctx"):
        o = cases.operands(grid, name)
        note(name, "z and 1 - z swapped", o, ref_of(name, _mut(o, z=(1.0 - o.z.double()))))
    # PARTIAL: the bound is per element
    o = cases.operands(grid, "partial")
    raw = cases.conv_sum(grid, "partial")
    pb = oce.partial_bound(o.x, o.w, o.init, o.init_off)
    pref = cases.reference(o, rounded=False, raw=raw)
    note("partial", "bias added", o, (pref[0] + o.b.double(),), pb, pref)
    note("partial", "initial accumulator at channel offset 128", o, cases.reference(_mut(o, init_off=128), rounded=False, raw=raw),
         pb, pref)
    # GLO with another input than net: the hidden state of the product read 8 channels off
    o = cases.operands(grid, "glo_x")
    raw = cases.conv_sum(grid, "glo_x")
    gb = oce.glo_bound(oce.glo_terms(o.x, o.w, o.b, o.net, raw=raw), H * W)
    note("glo_x", "net read 8 channels off", o, cases.reference(_mut(o, net=_shifted(o.net, 8)), raw=raw), gb)
    if flat:
        for name in ("zr_staged", "q_ctx", "heads", "eta", "partial"):
            o = cases.operands(grid, name)
            raw = cases.conv_sum(grid, name)
            leak = raw + _pad_leak(o)
            if name == "partial":
                note(name, "pad column = neighbouring row's pixel", o, cases.reference(o, rounded=False, raw=leak), pb, pref)
            else:
                note(name, "pad column = neighbouring row's pixel", o, cases.reference(o, raw=leak))
    for key, m in sorted(margins.items()):
        print("%-10s %-45s %8.1f x bound" % (key + (m,)))
    weak = {k: round(m, 2) for k, m in margins.items() if m < 10.0}
    assert not weak, (grid, weak)


# ------------------------------------------------------------------------------------------------ (iii) float32 evaluation
@pytest.mark.parametrize("grid", cases.GRIDS)
def test_float32_evaluation_stays_inside_the_bounds(grid):
    """fp32 convolution, the same rounding points: against the float64 evaluation inside the bounds the kernels are held
    to, and for the fp16 outputs at most one fp16 step apart with no element beyond the two-step bound."""
    B, H, W = grid
    for name, L in cases.LAUNCHES.items():
        if grid not in cases.launch_grids(name):
            continue
        o = cases.operands(grid, name)
        raw = cases.conv_sum(grid, name)
        lo = cases.reference(o, dtype=torch.float32)
        if L.mode == "partial":
            err = (lo[0].double() - cases.reference(o, rounded=False, raw=raw)[0]).abs()
            assert bool((err <= oce.partial_bound(o.x, o.w, o.init, o.init_off)).all()), (grid, name)
        elif L.mode == "glo":
            err = (lo[0].double() - cases.reference(o, raw=raw)[0]).abs()
            assert bool((err <= oce.glo_bound(oce.glo_terms(o.x, o.w, o.b, o.net, raw=raw), H * W)).all()), (grid, name)
            zero = (torch.zeros_like(o.w), torch.zeros_like(o.b))
            z64, z32 = (oce.glo(o.x, *zero, o.net, dtype=dt) for dt in (torch.float64, torch.float32))
            assert bool(((z32.double() - z64).abs() <= oce.glo_exact_bound(o.net)).all()), (grid, name, "exact form")
        else:
            for a, b in zip(lo, cases.reference(o, raw=raw)):
                scale = 0.01 if L.mode == "eta" else 1.0
                err, share = oce.fp16_errors(a.double() / scale, b / scale)
                print("%-12s max %.2e share %.1e" % (name, err, share))
                # (eta: the float32 product with 0.01f and its undoing here move a value by 2^-23 relative)
                one_step = bool(((a.double() - b).abs() / scale <= oce.two_step(b / scale) / 2 + 2.0 ** -22 * b.abs() / scale).all())
                assert share == 0.0 and one_step, (grid, name, err, share)
                assert oce.fp16_ok(a.double() / scale, b / scale)
