"""The frame encoders' layer kernels (enc_conv_kernel<KS,S>, enc_stem_kernel, enc_finish_kernel, enc_prep_kernel of
csrc/encoder.hip, through the C ABI `vipe_enc_*`) against the float64 restatement in oracle/encoder_layers.py, and the
whole fnet / cnet as vipe_amd/slam/encoders.py sequences them against its `emulate`.

Every layer case is ONE launch of oracle/encoder_cases.py, at an edge of the 4 x 32 x 32 tile: outputs of 3 x 5, 4 x 32,
5 x 33 and 9 x 70 pixels, stride 2 from odd and from even inputs, Cin 32 / 64 / 96 / 128.  Every output ELEMENT has to lie
in its interval [E(ref - acc), E(ref + acc)] (oracle/encoder_layers.py derives acc and the chain E), the statistics
within (n - 1) 2^-24 sum |term| of the float64 sums of the kernel's own pre-activation output, and every output and
statistics buffer has a guard image before and after the launch's own, filled with a canary that has to come back.
tests/test_oracle_encoder_layers.py shows on these very inputs that a float32 evaluation stays inside and what leaves.

The whole network is held to the spread of two CPU evaluations that round where the kernels round (float64 and float32
between the roundings): max |got - e64| <= 4 s_max and rms(got - e64) <= 2 s_rms.  The kernel's summation order is a
third realisation of the same rounding noise; the maximum over ten thousand outputs of such noise varies by about two
between realisations, the RMS barely.  Batched and single-image calls are each held to the gates, not to each other:
the statistics are float atomics.

Every case prints its figures before it asserts (`pytest -s`); DESIGN.md section 2 has those of the MI355X.
"""

from types import SimpleNamespace

import pytest
import torch

from oracle import encoder_cases as cases
from oracle import encoder_layers as oel

pytestmark = pytest.mark.gpu

CANARY16, CANARY32 = 7.0, -12345.5
EINVAL, EUNSUPPORTED = -1, -3


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _guarded(shape, canary, dtype):
    """[B + 2, ...] filled with the canary; the launch gets images 1 .. B"""
    return torch.full((shape[0] + 2,) + tuple(shape[1:]), canary, dtype=dtype, device=dev())


def _inner(t, what):
    """the launch's own images of a guarded buffer, as a CPU tensor, after checking both guards"""
    t = t.cpu()
    canary = CANARY16 if t.dtype == torch.float16 else CANARY32
    assert bool((t[0] == canary).all()) and bool((t[-1] == canary).all()), "%s: guard image written" % what
    return t[1:-1]


def _launch(o, relu, tanh_split, res, nchw, want_stats):
    """one vipe_enc_conv / vipe_enc_stem launch of operands `o` -> (y as NHWC CPU tensor, stats CPU tensor or None)"""
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    from vipe_amd.slam.encoders import _pack_conv, _pack_stem
    c = o.case
    conv = SimpleNamespace(weight=o.w.to(dev()), bias=o.bias.to(dev()))
    y = _guarded((c.B, c.cout, c.Ho, c.Wo) if nchw else (c.B, c.Ho, c.Wo, c.cout), CANARY16, torch.float16)
    stats = None
    if want_stats:
        stats = _guarded((c.B, c.cout, 2), CANARY32, torch.float32)
        stats[1:-1] = 0.0 if o.prefill is None else o.prefill.to(dev())
    if c.kind == "stem":
        x = torch.zeros(c.B, c.H, c.W, 4, dtype=torch.float16, device=dev())
        x[..., :3] = o.x.to(dev())
        wb = _pack_stem(conv)
        check(lib().vipe_enc_stem(ptr(x), ptr(wb[0]), ptr(wb[1]), ptr(y[1:]), ptr(stats[1:]) if want_stats else None, c.B,
                                  c.H, c.W, relu, stream_ptr(x)), "vipe_enc_stem")
    else:
        x = o.x.to(dev())
        wb = _pack_conv(conv)
        in_stats = None if o.in_stats is None else o.in_stats.to(dev())
        r = None if res is None else res.to(dev())
        check(lib().vipe_enc_conv(ptr(x), ptr(in_stats), ptr(wb[0]), ptr(wb[1]), ptr(r), ptr(y[1:]),
                                  ptr(stats[1:]) if want_stats else None, c.B, c.H, c.W, c.cin, c.cout, c.k, c.stride,
                                  relu, nchw, tanh_split, stream_ptr(x)), "vipe_enc_conv")
    torch.cuda.synchronize()
    y = _inner(y, c.id + " y")
    return (y.permute(0, 2, 3, 1) if nchw else y), (None if stats is None else _inner(stats, c.id + " stats"))


@pytest.mark.parametrize("cid", [c.id for c in cases.conv_cases() + cases.stem_cases()])
def test_layer_launch_lies_in_its_interval(cid):
    o, ref = cases.operands(cid), cases.reference(cid)
    c = o.case
    y, stats = _launch(o, c.relu, c.tanh_split, o.res, c.nchw, c.stats)
    mid = oel.epilogue(ref.ref, c.relu, c.tanh_split, o.res)
    out = oel.outside(y, ref.lo, ref.hi)
    print("FIG | %s | %d of %d outside | %.2f %% not the rounded float64 value, max |got - it| %.3e | interval open for %.2f %%" % (
        cid, out, y.numel(), 100 * float((y.double() != mid).double().mean()), float((y.double() - mid).abs().max()),
        100 * float((ref.lo != ref.hi).double().mean())))
    assert tuple(y.shape) == tuple(ref.lo.shape) and out == 0
    if c.stats:
        # the statistics are those of the fp16 value before ReLU, tanh or residual: the y of the bare launch
        y0 = y if (c.mode in ("plain", "norm") and c.tanh_split < 0) else _launch(o, 0, -1, None, 0, False)[0]
        want = oel.stats_sums(y0) + (0 if o.prefill is None else o.prefill.double())
        bound = oel.stats_bound(y0, o.prefill)
        err = (stats.double() - want).abs()
        print("FIG | %s | statistics: largest error / bound %.3f" % (cid, float((err / bound.clamp(min=1e-300)).max())))
        assert bool((err <= bound).all())


@pytest.mark.parametrize("cid", [c.id for c in cases.finish_cases()])
def test_finish_lies_in_its_interval(cid):
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    o = cases.finish_operands(cid)
    c = o.case
    lo, hi = cases.finish_reference(cid)
    raw, rs = o.raw.to(dev()), o.raw_stats.to(dev())
    res = None if o.res is None else o.res.to(dev())
    xs = None if o.res_stats is None else o.res_stats.to(dev())
    out = _guarded((c.B, c.H, c.W, c.C), CANARY16, torch.float16)
    check(lib().vipe_enc_finish(ptr(raw), ptr(rs), ptr(res), ptr(xs), ptr(out[1:]), c.B, c.H * c.W, c.C, stream_ptr(raw)),
          "vipe_enc_finish")
    torch.cuda.synchronize()
    got = _inner(out, cid)
    n = oel.outside(got, lo, hi)
    print("FIG | %s | %d of %d outside | interval open for %.2f %%" % (cid, n, got.numel(),
                                                                      100 * float((lo != hi).double().mean())))
    assert n == 0


@pytest.mark.parametrize("shape", cases.PREP_CASES, ids=lambda s: "%dx%dx%d" % s)
def test_prep_is_bit_exact(shape):
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    img = cases.prep_image(shape)
    d_img = img.to(dev())
    out = _guarded((shape[0], shape[1], shape[2], 4), CANARY16, torch.float16)
    check(lib().vipe_enc_prep(ptr(d_img), ptr(out[1:]), shape[0], shape[1], shape[2], stream_ptr(d_img)), "vipe_enc_prep")
    torch.cuda.synchronize()
    assert torch.equal(_inner(out, "prep").view(torch.int16), oel.prep(img).view(torch.int16))


# ------------------------------------------------------------------------------------------------ the whole network
@pytest.mark.parametrize("grid", cases.NET_GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("name", ["fnet", "cnet"])
def test_whole_network_within_the_spread_of_its_references(name, grid):
    from vipe_amd.slam.encoders import DroidEncoders, normalize_images
    e64, e32 = cases.net_reference(name, grid)
    s_max, s_rms = cases.spread(e64, e32)
    enc = DroidEncoders()
    getattr(enc, name).load_state_dict(cases.net_state(name))
    enc = enc.to(dev())
    img = cases.net_images(grid).to(dev())
    assert torch.equal(normalize_images(img).cpu().view(torch.int16), oel.prep(cases.net_images(grid)).view(torch.int16))

    def run(images):
        if name == "fnet":
            return enc.encode_features(images)
        return torch.cat(enc.encode_context(images), 1)

    batched = run(img)
    single = torch.cat([run(img[i:i + 1].contiguous()) for i in range(img.shape[0])], 0)
    torch.cuda.synchronize()
    scale = float(e64.abs().max())
    figs = {}
    for how, got in (("batched", batched), ("single", single)):
        assert got.dtype == torch.float16 and tuple(got.shape) == tuple(e64.shape)
        d = got.cpu().double() - e64
        figs[how] = (float(d.abs().max()), float((d * d).mean().sqrt()))
        print("FIG | %s %dx%d %s | scale %.3f | s_max %.3e s_rms %.3e | max |got - e64| %.3e (%.2f s_max) rms %.3e (%.2f s_rms)" % (
            name, grid[0], grid[1], how, scale, s_max, s_rms, figs[how][0], figs[how][0] / s_max, figs[how][1],
            figs[how][1] / s_rms))
    for how, (e_max, e_rms) in figs.items():
        assert e_max <= 4 * s_max and e_rms <= 2 * s_rms, (how, e_max, s_max, e_rms, s_rms)


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_launch_nothing():
    """the return codes include/vipe_amd.h promises; every call gets valid device pointers, and nothing is written"""
    from vipe_amd._lib import lib, ptr, stream_ptr
    B, H, W = 1, 4, 8
    x = torch.zeros(B, H, W, 160, dtype=torch.float16, device=dev())
    w = torch.zeros(25 * 160 * 64, dtype=torch.float16, device=dev())
    bias = torch.zeros(256, device=dev())
    res = torch.zeros(B, H, W, 64, dtype=torch.float16, device=dev())
    st = torch.zeros(B, 160, 2, device=dev())
    y = torch.full((B, H, W, 256), CANARY16, dtype=torch.float16, device=dev())
    s = stream_ptr(x)

    def conv(cin=32, cout=64, k=3, stride=1, r=None, nchw=0):
        return lib().vipe_enc_conv(ptr(x), None, ptr(w), ptr(bias), ptr(r), ptr(y), None, B, H, W, cin, cout, k, stride, 0,
                                   nchw, -1, s)

    assert conv(k=5) == EUNSUPPORTED
    assert conv(cin=160) == EINVAL
    assert conv(cin=48) == EINVAL
    assert conv(r=res, nchw=1) == EINVAL
    assert conv(cin=0) == EINVAL
    assert conv(cout=0) == EINVAL
    assert lib().vipe_enc_finish(ptr(x), ptr(st), None, None, ptr(y), B, H * W, 12, s) == EINVAL
    assert lib().vipe_enc_finish(ptr(x), ptr(st), None, ptr(st), ptr(y), B, H * W, 32, s) == EINVAL
    torch.cuda.synchronize()
    assert bool((y == CANARY16).all())
