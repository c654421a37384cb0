"""Inputs of the fused-convolution launches of the flow-update operator, as csrc/update_op.hip issues them.

ORACLE (test infrastructure).  One place builds them, seeded, so that the CPU test that shows what the reference can tell
apart (tests/test_oracle_conv_epilogues.py) and the GPU test that feeds them to the tile kernels
(tests/test_gpu_conv_epilogues.py) look at the same numbers.  Everything returned is shared between tests: do not write
into it.

`LAUNCHES` is the table of launches: which buffer, channel pitch and channel offset every operand of
`vipe_conv2d_fused` has in `vipe_update_operator` / `vipe_update_gate_state`.  `buffers(grid)` are the operator's buffers
with random contents of the operator's magnitudes (hidden state in (-1, 1), activations ~0.5, the per-image term ~0.1,
initial accumulators ~0.5), `operands(grid, name)` the logical operands of one launch for oracle/conv_epilogues.py.
"""

import functools
import zlib
from types import SimpleNamespace

import torch

from . import conv_epilogues as oce

# (images, rows, columns).  Aligned: made of 4 x 64 tiles.  (2,8,64): two row tiles per image and two images - the image
# index of `extra` matters on tiles after the first; (1,4,128): two 64-column segments, the halo crosses their seam.
GRIDS_ALIGNED = [(2, 8, 64), (1, 4, 128)]
# Flat tiling (256 consecutive positions of the image padded by one column).  (3,5,7): one short tile per image;
# (2,4,63): pitch 64, the padded image is exactly one full tile that ends on a pad position; (2,9,86): four tiles with
# boundaries in mid-row, the last of 15 positions; (1,5,126): the widest flat grid.  H W = 35 and 774 (short last tile of
# the global-context kernel) and 512 (exact).
GRIDS_FLAT = [(3, 5, 7), (2, 4, 63), (2, 9, 86), (1, 5, 126)]
GRIDS = GRIDS_ALIGNED + GRIDS_FLAT

MODE = {"plain": 0, "glo": 1, "zr": 2, "q": 3, "heads": 4, "eta": 5, "partial": 6}


def _launch(mode, cout, k, x0, x1=None, act="none", extra_off=None, init=None, net=None, z=None, y=None, y2=None,
            aligned_only=False):
    """x0 / x1 = (buffer, channel offset, channels read); init = (buffer, channel offset); y / y2 = (pitch, offset)"""
    return SimpleNamespace(mode=mode, cout=cout, k=k, x0=x0, x1=x1, act=act, extra_off=extra_off, init=init, net=net, z=z,
                           y=y, y2=y2, aligned_only=aligned_only, cin=x0[2] + (x1[2] if x1 else 0), split=x0[2])


LAUNCHES = {
    # update_op.hip: the global-context gate with `net` as its own input (conv1x1_glo_kernel) ...
    "glo_net": _launch("glo", 128, 1, ("net", 0, 128), net="net"),
    # ... and with another input tensor: the tile kernel's own GLO fold
    "glo_x": _launch("glo", 128, 1, ("x", 0, 128), net="net"),
    "zr": _launch("zr", 256, 3, ("net", 0, 128), ("xbuf", 0, 320), extra_off=0, net="net", y=(128, 0), y2=(128, 0)),
    "zr_ctx": _launch("zr", 256, 3, ("net", 0, 128), ("xbuf", 128, 192), extra_off=0, init=("pgate", 0), net="net",
                      y=(128, 0), y2=(128, 0)),
    "zr_staged": _launch("zr", 256, 3, ("xbuf", 128, 192), extra_off=0, init=("pzr", 0), net="net", y=(128, 0), y2=(128, 0)),
    "partial": _launch("partial", 256, 3, ("net", 0, 128), init=("pgate", 0), y=(256, 0)),
    "q": _launch("q", 128, 3, ("rnet", 0, 128), ("xbuf", 0, 320), extra_off=256, net="net", z="z", y=(128, 0)),
    "q_ctx": _launch("q", 128, 3, ("rnet", 0, 128), ("xbuf", 128, 192), extra_off=256, init=("pgate", 256), net="net", z="z",
                     y=(128, 0)),
    "heads": _launch("heads", 4, 3, ("hbuf", 0, 256)),
    "eta": _launch("eta", 1, 3, ("a2", 0, 128)),
    # plain convolutions into a channel slice of a wider buffer (the flat grids: tests/test_gpu_grids.py)
    "plain_corr2": _launch("plain", 128, 3, ("c1", 0, 128), act="relu", y=(320, 128), aligned_only=True),
    "plain_flow2": _launch("plain", 64, 3, ("f1", 0, 128), act="relu", y=(320, 256), aligned_only=True),
    "plain_heads0": _launch("plain", 384, 3, ("net", 0, 128), act="relu", y=(384, 0), aligned_only=True),
    # the upsampling mask of GraphAgg (update_engine.py): 576 output channels in a channel tile padded to 640
    "plain_upmask": _launch("plain", 576, 1, ("a2", 0, 128), y=(576, 0)),
}


def launch_grids(name):
    return GRIDS_ALIGNED if LAUNCHES[name].aligned_only else GRIDS


def expected_kernel(name, grid):
    """the kernel `launch_conv`'s documented dispatch order takes for this launch (conv_mfma.hip)"""
    L = LAUNCHES[name]
    flat = grid not in GRIDS_ALIGNED
    if name == "glo_net":
        return "conv1x1_glo_kernel"
    if L.k == 3 and L.cout <= 16:
        return "conv_halo32_narrow_kernel<%s>" % ("FLAT" if flat else "4x64")
    bmc = 128 if L.cout > 64 else (64 if L.cout > 32 else 32)
    var = 2 if L.mode == "partial" else (1 if L.init and L.init[0] == "pzr" else 0)
    return "conv_halo32_kernel<%d,%d,VAR %d,%s>" % (bmc, L.k, var, "FLAT" if flat else "4x64")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=None)
def buffers(grid):
    """the operator's buffers on this grid: name -> CPU tensor (fp16 unless noted)"""
    B, H, W = grid
    g = _gen("buffers", grid)

    def rnd(*shape, scale=0.5):
        return torch.randn(*shape, generator=g) * scale

    return {
        "net": rnd(B, H, W, 128, scale=1.0).tanh().half(),
        "x": rnd(B, H, W, 128).half(),
        "xbuf": rnd(B, H, W, 320).half(),
        "rnet": (torch.sigmoid(rnd(B, H, W, 128, scale=1.0)) * rnd(B, H, W, 128, scale=1.0).tanh()).half(),
        "z": torch.sigmoid(rnd(B, H, W, 128, scale=1.5)).half(),
        "hbuf": rnd(B, H, W, 384).relu().half(),
        "a2": rnd(B, H, W, 128).relu().half(),
        "c1": rnd(B, H, W, 128).relu().half(),
        "f1": rnd(B, H, W, 128).relu().half(),
        "extra": rnd(B, 384, scale=0.1),              # float32
        "pgate": rnd(B, H, W, 384).half(),
        "pzr": rnd(B, H, W, 256),                     # float32
        "glo_prefill": rnd(B + 2, 128, scale=1.0),    # float32: fout of the GLO launches with its two guard rows
    }


@functools.lru_cache(maxsize=None)
def weights(name):
    """-> (OIHW fp16 weight ~ 1 / sqrt(K), float32 bias ~ 0.1) of a launch, the same on every grid"""
    L = LAUNCHES[name]
    g = _gen("weights", name)
    w = (torch.randn(L.cout, L.cin, L.k, L.k, generator=g) / (L.cin * L.k * L.k) ** 0.5).half()
    return w, torch.randn(L.cout, generator=g) * 0.1


def operands(grid, name, bufs=None, wb=None):
    """the logical operands of launch `name` on `grid` (oracle/conv_epilogues.py); `bufs` / `wb` replace the seeded
    buffers / (weight, bias)"""
    L = LAUNCHES[name]
    bufs = buffers(grid) if bufs is None else bufs
    w, b = weights(name) if wb is None else wb

    def src(s):
        return bufs[s[0]][..., s[1]:s[1] + s[2]]

    x = src(L.x0) if L.x1 is None else (src(L.x0), src(L.x1), L.split)
    return SimpleNamespace(launch=L, mode=L.mode, act=L.act, x=x, w=w, b=b,
                           extra=None if L.extra_off is None else bufs["extra"], extra_off=L.extra_off or 0,
                           init=None if L.init is None else bufs[L.init[0]], init_off=L.init[1] if L.init else 0,
                           net=None if L.net is None else bufs[L.net], z=None if L.z is None else bufs[L.z])


@functools.lru_cache(maxsize=None)
def conv_sum(grid, name):
    """the float64 convolution sum of the seeded launch (the expensive part of its reference), computed once"""
    o = operands(grid, name)
    return oce.conv_sum(o.x, o.w)


def reference(o, rounded=True, dtype=torch.float64, raw=None):
    """what launch operands `o` make the kernel write -> tuple of tensors: plain (y), glo (the sum added to fout [B,128]),
    zr (z, r * net), q (y), heads (fout [B,H,W,4]), eta (fout [B,H,W]), partial (fout [B,H,W,Cout])"""
    kw = dict(rounded=rounded, dtype=dtype, raw=raw)
    ex = dict(extra=o.extra, extra_off=o.extra_off, init=o.init, init_off=o.init_off)
    if o.mode == "plain":
        return (oce.plain(o.x, o.w, o.b, o.act, **ex, **kw),)
    if o.mode == "glo":
        return (oce.glo(o.x, o.w, o.b, o.net, **kw),)
    if o.mode == "zr":
        return oce.zr(o.x, o.w, o.b, o.net, **ex, **kw)
    if o.mode == "q":
        return (oce.q(o.x, o.w, o.b, o.net, o.z, **ex, **kw),)
    if o.mode == "heads":
        return (oce.heads(o.x, o.w, o.b, **kw),)
    if o.mode == "eta":
        return (oce.eta(o.x, o.w, o.b, **kw),)
    assert o.mode == "partial"
    return (oce.partial(o.x, o.w, o.init, o.init_off, **kw),)
