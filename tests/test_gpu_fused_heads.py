"""The flow / weight heads contracted in their producer's epilogue (vipe_conv2d_fused mode 7 + vipe_heads_finish) on the
smallest grids at which the contraction can go wrong, E = 2 throughout:

    4 x 64    one tile per image: only the image borders
    8 x 64    one vertical tile border
    8 x 128   horizontal borders and the four corners
    8 x 128 with one faint and one loud image: a partial sum that crosses the image boundary shows

(a) two runs are bit-identical (no atomics; dw and the border records are refilled with NaN between them, so a sum that
    reads a record its tile did not write is NaN);
(b) against the float64 reference of the two launches it replaces (oracle/conv_epilogues.py: `plain` then `heads`), with
    the bound tests/test_gpu_conv_epilogues.py holds the `heads` launch to: largest error <= FP16_CAP, at most
    FP16_SHARE of the outputs beyond two fp16 steps;
(c) against the two-launch result on the same inputs: the two differ in the fp32 summation order before the one fp16
    rounding, so the largest difference has to stay within the two-launch path's own largest error against the reference.

Figures are printed before anything is asserted (`pytest -s`)."""
import functools

import pytest
import torch

from oracle import conv_epilogue_cases as cases
from oracle import conv_epilogues as oce

pytestmark = pytest.mark.gpu

SHAPES = {"4x64": (4, 64, False), "8x64": (8, 64, False), "8x128": (8, 128, False), "8x128_contrast": (8, 128, True)}
E = 2


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _weights():
    w0, b0 = cases.weights("plain_heads0")
    w2d, b2 = cases.weights("heads")
    w2 = torch.zeros_like(w2d)  # heads2 is block diagonal: delta2 reads delta0's channels, weight2 weight0's
    w2[0:2, 0:128], w2[2:4, 128:256] = w2d[0:2, 0:128], w2d[2:4, 128:256]
    return w0[:256].contiguous(), b0[:256].contiguous(), w2, b2


@functools.lru_cache(maxsize=None)
def _case(shape):
    """(input [E,H,W,128] fp16, float64 reference [E,H,W,4]) - computed once per shape, shared by the checks"""
    H, W, contrast = SHAPES[shape]
    g = torch.Generator().manual_seed(100 + H + W + contrast)
    x = torch.randn(E, H, W, 128, generator=g).tanh()
    if contrast:
        x[0] *= 0.02
        x[1] = x[1] * 3.0 + 1.0
    x = x.half()
    w0, b0, w2, b2 = _weights()
    ref = oce.heads(oce.plain(x, w0, b0, "relu"), w2, b2)
    return x, ref


def _engine_parts():
    from vipe_amd.slam.update_engine import _Packed, pack_heads2_fragments
    w0, b0, w2, b2 = _weights()
    return _Packed(w0, b0, dev()), _Packed(w2, b2, dev()), pack_heads2_fragments(w2.to(dev()))


def _conv(pk, x, mode, act, y=None, y2=None, net=None, fout=None, cin=None):
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    B, H, W, _ = x.shape
    check(lib().vipe_conv2d_fused(ptr(x), x.shape[-1], 0, None, 0, 0, cin or pk.cin, ptr(pk.packed), ptr(pk.bias), None, 0, 0,
                                  ptr(y), 0 if y is None else y.shape[-1], 0, ptr(y2), 0, 0, ptr(net), 0, 0, None, ptr(fout),
                                  None, 0, 0, B, H, W, cin or pk.cin, pk.cout, pk.kh, pk.kw, act, mode, stream_ptr(x)), "conv")


def _fused(x, pk0, pk2, frag):
    import ctypes
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    B, H, W, _ = x.shape
    n = ctypes.c_int64()
    check(lib().vipe_heads_border_floats(B, H, W, ctypes.addressof(n)), "border_floats")
    assert n.value == B * (H // 4) * (W // 64) * 140 * 4
    border = torch.full((n.value,), float("nan"), dtype=torch.float32, device=dev())
    dw = torch.full((B + 2, H, W, 4), float("nan"), dtype=torch.float32, device=dev())  # a guard image on either side
    _conv(pk0, x, 7, 1, y2=border, net=frag, fout=dw[1:])
    check(lib().vipe_heads_finish(ptr(dw[1:]), ptr(border), ptr(pk2.bias), B, H, W, stream_ptr(x)), "heads_finish")
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw[0]).all()) and bool(torch.isnan(dw[-1]).all()), "guard image written"
    return dw[1:-1].cpu()


def _two_launches(x, pk0, pk2):
    B, H, W, _ = x.shape
    hbuf = torch.zeros(B, H, W, 384, dtype=torch.float16, device=dev())
    dw = torch.empty(B, H, W, 4, dtype=torch.float32, device=dev())
    _conv(pk0, x, 0, 1, y=hbuf)
    _conv(pk2, hbuf, 4, 0, fout=dw, cin=256)
    torch.cuda.synchronize()
    return dw.cpu()


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fused_heads_on_the_smallest_grids(shape):
    from vipe_amd._lib import lib
    H, W, _ = SHAPES[shape]
    assert lib().vipe_heads_fused_ok(H, W) == 1, "the fused heads are switched off (VIPE_AMD_FUSED_HEADS)"
    x, ref = _case(shape)
    xd = x.to(dev())
    pk0, pk2, frag = _engine_parts()
    got, again = _fused(xd, pk0, pk2, frag), _fused(xd, pk0, pk2, frag)
    two = _two_launches(xd, pk0, pk2)
    err, share = oce.fp16_errors(got.double(), ref)
    err2, share2 = oce.fp16_errors(two.double(), ref)
    diff = float((got.double() - two.double()).abs().max())
    print("FIG | fused heads | %s | max err fused %.3e (share over two steps %.2e) | two launches %.3e (%.2e) | "
          "max |fused - two launches| %.3e" % (shape, err, share, err2, share2, diff))
    assert bool(torch.isfinite(got).all()), shape
    assert torch.equal(got, again), (shape, "two runs differ")                        # (a)
    assert err <= oce.FP16_CAP and share <= oce.FP16_SHARE, (shape, err, share)      # (b)
    assert diff <= err2, (shape, diff, err2)                                         # (c)


def test_fused_heads_refuse_other_grids_and_follow_the_switch():
    """a ragged grid is no grid of 4 x 64 tiles: the predicate says so and the launch is VIPE_EUNSUPPORTED, not a fallback"""
    from vipe_amd._lib import lib, ptr, stream_ptr
    L = lib()
    assert L.vipe_heads_fused_ok(41, 73) == 0 and L.vipe_heads_fused_ok(8, 64) == 1 and L.vipe_heads_fused_ok(6, 64) == 0
    pk0, pk2, frag = _engine_parts()
    x = torch.zeros(1, 6, 64, 128, dtype=torch.float16, device=dev())
    dw = torch.zeros(1, 6, 64, 4, dtype=torch.float32, device=dev())
    border = torch.zeros(4096, dtype=torch.float32, device=dev())
    rc = L.vipe_conv2d_fused(ptr(x), 128, 0, None, 0, 0, 128, ptr(pk0.packed), ptr(pk0.bias), None, 0, 0, None, 0, 0, ptr(border),
                             0, 0, ptr(frag), 0, 0, None, ptr(dw), None, 0, 0, 1, 6, 64, 128, 256, 3, 3, 1, 7, stream_ptr(x))
    assert rc == -3, rc  # VIPE_EUNSUPPORTED
