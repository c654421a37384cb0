"""Launches of the frame encoders' layer kernels (csrc/encoder.hip), each at an edge of the kernels' tiling.

ORACLE (test infrastructure).  One place builds them, seeded, so that the CPU test that shows what the intervals of
oracle/encoder_layers.py can tell apart (tests/test_oracle_encoder_layers.py) and the GPU test that feeds the launches to
the kernels (tests/test_gpu_encoder_layers.py) look at the same numbers.  Everything returned is shared between tests: do
not write into it.

The convolution kernel's tile is 4 rows x 32 columns x 32 output channels.  Output grids: 3 x 5 (one partial tile),
4 x 32 (exactly one), 5 x 33 (2 x 2 tiles, the last of one row and one column), 9 x 70 (3 x 3 tiles).  A stride-2 launch
reaches an output size from the odd input 2 Ho - 1 (the last halo row / column half outside the image) and from the even
one 2 Ho; rows and columns take their parities independently.  `conv_cases()` is not the cross product: every (kernel,
channel pair) appears once per mode, the grids rotate so that every kernel meets every grid in every mode, parities and
statistics on / off rotate with the mode.

Inputs are randn plus a per-image, per-channel offset of up to two standard deviations, and the images of a batch have
different scales: statistics read from the wrong image are far outside any interval.  Weights are drawn as
`kaiming_normal_(mode="fan_out", nonlinearity="relu")` draws them in BasicEncoder - normal with std
sqrt(2 / (Cout k k)) - and rounded to fp16; biases ~ 0.1.
"""

import functools
import zlib
from types import SimpleNamespace

import torch

from . import encoder_layers as oel

GRIDS = [(3, 5), (4, 32), (5, 33), (9, 70)]
KERNELS = [(3, 1), (3, 2), (1, 2), (1, 1)]  # (k, stride): the four instantiations of enc_conv_kernel
CHANNELS = [(32, 32), (32, 64), (64, 64), (64, 128), (96, 64), (128, 128)]
MODES = ["plain", "relu", "norm", "residual"]  # norm: normalise on load; residual: relu(res + relu(conv))
SCALES = (1.0, 0.6, 1.5)  # per image


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _conv_case(mode, k, stride, cin, cout, grid, par=(0, 0), B=2, stats=False, prefill=False, nchw=0, tanh_split=-1):
    Ho, Wo = grid
    H, W = (Ho, Wo) if stride == 1 else (2 * Ho - 1 + par[0], 2 * Wo - 1 + par[1])
    cid = "%s-k%ds%d-%dto%d-%dx%d-in%dx%d-B%d%s%s%s" % (
        mode, k, stride, cin, cout, Ho, Wo, H, W, B, "-stats" if stats else "", "-prefill" if prefill else "",
        ("-nchw%d" % tanh_split) if nchw else "")
    return SimpleNamespace(kind="conv", id=cid, mode=mode, k=k, stride=stride, cin=cin, cout=cout, B=B, H=H, W=W, Ho=Ho,
                           Wo=Wo, stats=stats, prefill=prefill, nchw=nchw, tanh_split=tanh_split,
                           relu=int(mode in ("relu", "residual")))


@functools.lru_cache(maxsize=None)
def conv_cases():
    out = []
    for mi, mode in enumerate(MODES):
        for ki, (k, stride) in enumerate(KERNELS):
            chans = CHANNELS + ([(128, 256)] if k == 1 else [])
            for ci, (cin, cout) in enumerate(chans):
                par = ((ci // 4 + mi) % 2, (ci // 4 + ci + mi) % 2)
                out.append(_conv_case(mode, k, stride, cin, cout, GRIDS[(ci + ki) % 4], par,
                                      B=3 if (mode == "plain" and ci == 0) else 2, stats=(ci + mi) % 2 == 0,
                                      prefill=(mode == "plain" and ci == 2 and ki == 0)))
    # the output convolutions: NCHW stores, the context net's tanh / ReLU split at 128, all ReLU (0), all tanh (256);
    # the feature net's (no split) with 128 outputs
    for gi, split in enumerate((128, 0, 256)):
        out.append(_conv_case("plain", 1, 1, 128, 256, GRIDS[gi + 1], nchw=1, tanh_split=split))
    out.append(_conv_case("plain", 1, 1, 128, 128, GRIDS[0], nchw=1))
    out.append(_conv_case("plain", 1, 1, 128, 256, GRIDS[0], B=3, nchw=1, tanh_split=128))
    assert len({c.id for c in out}) == len(out)
    return out


@functools.lru_cache(maxsize=None)
def stem_cases():
    """inputs 7 x 65 (4 x 33 outputs from odd sizes), 8 x 64 (exactly one tile from even sizes), 50 x 90 (25 x 45: what
    the whole-network test's odd grid gives the stem)"""
    out = []
    for (H, W) in ((7, 65), (8, 64), (50, 90)):
        for relu in (0, 1):
            for stats in (False, True):
                B = 3 if (H == 7 and relu == 0 and stats) else 2
                out.append(SimpleNamespace(kind="stem", id="stem-in%dx%d-relu%d-B%d%s" % (H, W, relu, B, "-stats" if stats else ""),
                                           k=7, stride=2, cin=3, cout=32, B=B, H=H, W=W, Ho=(H - 1) // 2 + 1,
                                           Wo=(W - 1) // 2 + 1, relu=relu, stats=stats, prefill=False, mode="relu" if relu else "plain",
                                           nchw=0, tanh_split=-1))
    return out


@functools.lru_cache(maxsize=None)
def finish_cases():
    """(grid, C) x the three forms; 130 x 260 x 128 is past the kernel's cap of 2048 workgroups (its grid-stride loop
    takes a second round)"""
    out = []
    for (grid, C, B) in (((3, 5), 32, 2), ((4, 32), 8, 3), ((5, 33), 64, 2), ((9, 70), 128, 2)):
        for form in ("none", "raw", "norm"):
            out.append(SimpleNamespace(kind="finish", id="finish-%s-%dx%d-C%d-B%d" % (form, grid[0], grid[1], C, B), form=form,
                                       B=B, H=grid[0], W=grid[1], C=C))
    out.append(SimpleNamespace(kind="finish", id="finish-raw-130x260-C128-B1", form="raw", B=1, H=130, W=260, C=128))
    return out


PREP_CASES = [(2, 7, 65), (3, 50, 90), (1, 1030, 1020)]  # the last: past the kernel's cap of 4096 workgroups


def activations(key, B, H, W, C):
    """randn * scale[image] + offset[image, channel], |offset| <= 2 scale -> NHWC fp16"""
    g = _gen("act", key)
    sc = torch.tensor([SCALES[b % 3] for b in range(B)]).view(B, 1, 1, 1)
    off = (torch.rand(B, 1, 1, C, generator=g) * 4.0 - 2.0) * sc
    return (torch.randn(B, H, W, C, generator=g) * sc + off).half()


def stats_of(x):
    """the float32 statistics buffer of NHWC fp16 x as a producer leaves it: the float64 sums rounded once"""
    return oel.stats_sums(x).float().contiguous()


@functools.lru_cache(maxsize=None)
def weights(k, cin, cout):
    """-> (OIHW fp16 weight, float32 bias), the same for every launch of this kernel size and channel pair"""
    g = _gen("weights", k, cin, cout)
    w = (torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cout * k * k)) ** 0.5).half()
    return w, torch.randn(cout, generator=g) * 0.1


def _case(cid):
    return next(c for c in conv_cases() + stem_cases() + finish_cases() if c.id == cid)


@functools.lru_cache(maxsize=None)
def operands(cid):
    """the logical operands of convolution / stem launch `cid`: x, w, bias, res, in_stats, prefill (of the statistics
    buffer, [B,Cout,2] float32 or None)"""
    c = _case(cid)
    x = activations(cid, c.B, c.H, c.W, c.cin)
    w, bias = weights(c.k, c.cin, c.cout)
    g = _gen("extra", cid)
    res = (torch.randn(c.B, c.Ho, c.Wo, c.cout, generator=g) * 2.0).half() if c.mode == "residual" else None
    in_stats = stats_of(x) if c.mode == "norm" else None
    prefill = torch.randn(c.B, c.cout, 2, generator=g) * 10.0 if c.prefill else None
    return SimpleNamespace(case=c, x=x, w=w, bias=bias, res=res, in_stats=in_stats, prefill=prefill)


@functools.lru_cache(maxsize=None)
def reference(cid):
    """oracle/encoder_layers.py::conv_interval of launch `cid`, computed once"""
    o = operands(cid)
    c = o.case
    return oel.conv_interval(o.x, o.w, o.bias, c.stride, c.relu, c.tanh_split, o.res, o.in_stats)


@functools.lru_cache(maxsize=None)
def finish_operands(cid):
    c = _case(cid)
    raw = activations(cid, c.B, c.H, c.W, c.C)
    res = None if c.form == "none" else activations((cid, "res"), c.B, c.H, c.W, c.C)
    return SimpleNamespace(case=c, raw=raw, raw_stats=stats_of(raw), res=res,
                           res_stats=stats_of(res) if c.form == "norm" else None)


@functools.lru_cache(maxsize=None)
def finish_reference(cid):
    o = finish_operands(cid)
    return oel.finish_interval(o.raw, o.raw_stats, o.res, o.res_stats)


@functools.lru_cache(maxsize=None)
def prep_image(shape):
    return torch.rand(shape[0], 3, shape[1], shape[2], generator=_gen("prep", shape))


# ------------------------------------------------------------------------------------------------ the whole network
NET_GRIDS = [(64, 96), (50, 90)]  # 50 x 90: 25 x 45, 13 x 23, 7 x 12 - every intermediate size odd in one direction
NETS = {"fnet": ("instance", 128, -1), "cnet": ("none", 256, 128)}  # norm_fn, outputs, tanh_split


@functools.lru_cache(maxsize=None)
def net_images(grid):
    """three images of different brightness and contrast, [3,3,H,W] float32 in [0,1]"""
    g = _gen("images", grid)
    base = torch.rand(3, 3, grid[0], grid[1], generator=g)
    gain = torch.tensor([1.0, 0.45, 0.7]).view(3, 1, 1, 1)
    lift = torch.tensor([0.0, 0.5, 0.05]).view(3, 1, 1, 1)
    return (base * gain + lift).clamp(0, 1).contiguous()


@functools.lru_cache(maxsize=None)
def net_state(name):
    """BasicEncoder's default initialisation under a fixed seed -> state dict (float32)"""
    from vipe_amd.slam.encoders import BasicEncoder
    norm_fn, out, _ = NETS[name]
    torch.manual_seed(11 if name == "fnet" else 12)
    return {k: v.clone() for k, v in BasicEncoder(output_dim=out, norm_fn=norm_fn).state_dict().items()}


@functools.lru_cache(maxsize=None)
def net_reference(name, grid):
    """-> (e64, e32): `emulate` in float64 and in float32 on prep(net_images(grid)), [3,out,H/8,W/8] each as float64"""
    norm_fn, _, split = NETS[name]
    x = oel.prep(net_images(grid))[..., :3].permute(0, 3, 1, 2)
    sd = net_state(name)
    with torch.no_grad():
        e64 = oel.emulate(sd, x, norm_fn, torch.float64, split)
        e32 = oel.emulate(sd, x, norm_fn, torch.float32, split)
    return e64, e32.double()


def spread(e64, e32):
    """-> (s_max, s_rms) of the two evaluations"""
    d = e64.double() - e32.double()
    return float(d.abs().max()), float((d * d).mean().sqrt())
