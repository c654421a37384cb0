"""The fused epilogues of `vipe_conv2d_fused` (csrc/conv_mfma.hip), restated in torch float64 on the CPU.

ORACLE (test infrastructure).  One function per mode of the entry point (0 plain, 1 GLO, 2 ZR, 3 Q, 4 HEADS, 5 ETA,
6 PARTIAL), written from the contract in include/vipe_amd.h ("the flow-update operator's fused convolutions") and the
reference lines cited there (droid_net.py:373-499).  Every function takes the LOGICAL operands of one launch - what the
kernel reads through its pitches and offsets, already sliced:

    x       NHWC [B,H,W,Cin], or (x0, x1, split): input channels [0, split) are x0[..., :split], channels [split, Cin)
            are x1[..., :Cin - split] (the concatenations of the reference are never materialised)
    w, b    OIHW weight, bias [Cout]
    extra   optional [B, stride] per-image additive term, read at [extra_off, extra_off + Cout)
    init    optional [B,H,W,pitch] initial accumulator (fp16 or fp32), read at channels [init_off, init_off + Cout)
    raw     optional: the bare convolution sum [B,H,W,Cout] of (x, w) computed earlier by `conv_sum` (tests that evaluate
            one launch several times with other epilogue operands pass it to pay for the convolution once)

and returns what the kernel writes, computed in `dtype` (float64; float32 gives the evaluation a careful float32
implementation would produce) and ROUNDED WHERE THE KERNEL ROUNDS: the activation is rounded to fp16, a blend with the
hidden state is evaluated on that fp16 value and rounded to fp16 again, HEADS / ETA round to fp16 and widen to float.
`rounded=False` skips every rounding: the mathematical function, which chains into
oracle/update_module.py::update_forward (tests/test_oracle_conv_epilogues.py).

The bounds a kernel has to meet stand next to the functions (`fp16_errors`, `partial_bound`, `glo_bound`,
`glo_exact_bound`).  They come from the number formats and from bounds the project already asserts for the same
operations, not from what a kernel returns.
"""

import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24  # unit roundoff of float32

FP16_CAP = 4e-3         # hard cap on every fp16 output, absolute
FP16_SHARE = 1e-3       # at most this share of an output's elements may exceed the two-step bound


def h16(t):
    """round to fp16 (one correctly rounded conversion: numpy's, torch's double -> half goes through float) and widen"""
    return torch.from_numpy(t.detach().numpy().astype(np.float16)).to(t.dtype)


def _input(x, cin):
    if isinstance(x, (tuple, list)):
        x0, x1, split = x
        x = torch.cat([x0[..., :split], x1[..., :cin - split]], -1)
    assert x.shape[-1] == cin, (x.shape, cin)
    return x


def conv_sum(x, w, dtype=torch.float64):
    """the bare convolution ('same' padding, stride 1) of NHWC x with OIHW w -> [B,H,W,Cout] in `dtype`"""
    x = _input(x, w.shape[1])
    v = F.conv2d(x.permute(0, 3, 1, 2).to(dtype), w.to(dtype), None, padding=(w.shape[2] // 2, w.shape[3] // 2))
    return v.permute(0, 2, 3, 1).contiguous()


def preactivation(x, w, b, extra=None, extra_off=0, init=None, init_off=0, dtype=torch.float64, raw=None):
    """init + conv + bias + extra[image]: the value every epilogue but PARTIAL starts from"""
    cout = w.shape[0]
    v = conv_sum(x, w, dtype) if raw is None else raw.to(dtype)
    if init is not None:
        v = init[..., init_off:init_off + cout].to(dtype) + v
    if b is not None:
        v = v + b.to(dtype)
    if extra is not None:
        v = v + extra[:, None, None, extra_off:extra_off + cout].to(dtype)
    return v


def _act(v, act):
    return {"none": lambda t: t, "relu": torch.relu, "sigmoid": torch.sigmoid, "tanh": torch.tanh}[act](v)


def _r(t, rounded):
    return h16(t) if rounded else t


# ------------------------------------------------------------------------------------------------ the seven modes
def plain(x, w, b, act="none", extra=None, extra_off=0, init=None, init_off=0, rounded=True, dtype=torch.float64, raw=None):
    """mode 0: y = h16(act(conv + bias + extra[image]))   [B,H,W,Cout]"""
    return _r(_act(preactivation(x, w, b, extra, extra_off, init, init_off, dtype, raw), act), rounded)


def glo(x, w, b, net, rounded=True, dtype=torch.float64, raw=None):
    """mode 1 (ConvGRU global context, droid_net.py:392-393): what the kernel ADDS to fout [B,Cout]:
    sum over the pixels of h16(sigmoid(conv + bias)) * net; the sum itself is not rounded (the kernel's float32 order is
    its own: `glo_bound` / `glo_exact_bound`)"""
    s = _r(torch.sigmoid(preactivation(x, w, b, dtype=dtype, raw=raw)), rounded)
    return (s * net.to(dtype)).sum((1, 2))


def zr(x, w, b, net, extra=None, extra_off=0, init=None, init_off=0, rounded=True, dtype=torch.float64, raw=None):
    """mode 2 (droid_net.py:395-397), Cout = 256: (z, r * net) = (h16(sigmoid(.))[..., :128],
    h16(h16(sigmoid(.))[..., 128:] * net)); the product of two fp16 values is exact in the kernel's float32"""
    assert w.shape[0] == 256
    s = _r(torch.sigmoid(preactivation(x, w, b, extra, extra_off, init, init_off, dtype, raw)), rounded)
    return s[..., :128], _r(s[..., 128:] * net.to(dtype), rounded)


def q(x, w, b, net, z, extra=None, extra_off=0, init=None, init_off=0, rounded=True, dtype=torch.float64, raw=None):
    """mode 3 (droid_net.py:397-399), Cout = 128: h16((1 - z) * net + z * h16(tanh(.))).  The kernel blends in float32
    (1 - z is exact there, the two products and the sum round at 2^-24 relative, 2^-13 of an fp16 step)"""
    assert w.shape[0] == 128
    t = _r(torch.tanh(preactivation(x, w, b, extra, extra_off, init, init_off, dtype, raw)), rounded)
    zz = z.to(dtype)
    return _r((1.0 - zz) * net.to(dtype) + zz * t, rounded)


def heads(x, w, b, rounded=True, dtype=torch.float64, raw=None):
    """mode 4 (droid_net.py:486-490), Cout = 4: float [B,H,W,4] = (h16(v0), h16(v1), h16(sigmoid(v2)), h16(sigmoid(v3)))"""
    assert w.shape[0] == 4
    v = preactivation(x, w, b, dtype=dtype, raw=raw)
    return torch.cat([_r(v[..., :2], rounded), _r(torch.sigmoid(v[..., 2:]), rounded)], -1)


def softplus(v):
    """the kernel's form: v above 20 (where log1p(exp(v)) - v < 2.1e-9), log1p(exp(v)) below"""
    return torch.where(v > 20.0, v, torch.log1p(torch.exp(torch.clamp(v, max=20.0))))


def eta(x, w, b, rounded=True, dtype=torch.float64, raw=None):
    """mode 5 (droid_net.py:410,429), Cout = 1: float [B,H,W] = 0.01f * h16(softplus(v)), the product in float32"""
    assert w.shape[0] == 1
    sp = softplus(preactivation(x, w, b, dtype=dtype, raw=raw)[..., 0])
    if not rounded:
        return 0.01 * sp
    return (h16(sp).float() * torch.tensor(0.01, dtype=torch.float32)).to(dtype)


def partial(x, w, init=None, init_off=0, rounded=True, dtype=torch.float64, raw=None):
    """mode 6: float [B,H,W,Cout] = init + conv, the raw sums: NO bias, no extra, no activation (rounded: to float32)"""
    v = preactivation(x, w, None, None, 0, init, init_off, dtype, raw)
    return v.float().to(dtype) if rounded else v


# ------------------------------------------------------------------------------------------------ bounds
def two_step(ref):
    """2^-10 max(1, 2^ceil(log2 |ref|)): two fp16 steps at the value's magnitude, never less than two steps just below 1"""
    a = ref.abs().double().clamp(min=1.0)
    return 2.0 ** -10 * torch.exp2(torch.ceil(torch.log2(a)))


def fp16_errors(got, ref):
    """fp16 outputs (plain, ZR, Q, HEADS, ETA before its 0.01 factor) -> (largest |got - ref|, share of the elements
    beyond `two_step(ref)`).  A kernel has to meet BOTH of
        largest error <= FP16_CAP = 4e-3   what the project asserts for the same operations on the gather path and for the
                                           plain tile convolutions (tests/test_gpu_grids.py); values here stay below 8,
                                           where half an fp16 step is 2e-3
        share <= FP16_SHARE = 0.1 %        a correct kernel differs from the rounded float64 value only where its float32
                                           sum falls on the other side of an fp16 rounding boundary - ONE step, and for few
                                           elements; two steps need an error of a whole step before the rounding
    The float32 evaluation of these functions stays at one step and a share of 0 (tests/test_oracle_conv_epilogues.py), so
    the reference does not use the bounds up."""
    err = (got.double() - ref.double()).abs()
    return float(err.max()), float((err > two_step(ref)).double().mean())


def fp16_ok(got, ref):
    e, share = fp16_errors(got, ref)
    return e <= FP16_CAP and share <= FP16_SHARE


def partial_bound(x, w, init=None, init_off=0):
    """(K + 1) 2^-24 (|init| + sum |x w|) per element, K = taps * Cin: fp16 products are exact in float32, so any order of
    the K float32 additions (and the one of init) stays within K + 1 roundings of partial sums none larger than
    |init| + sum |x w|.  The sum term is the convolution of |x| with |w|."""
    cin = w.shape[1]
    s = conv_sum(_input(x, cin).double().abs(), w.double().abs())
    if init is not None:
        s = s + init[..., init_off:init_off + w.shape[0]].double().abs()
    return (w.shape[2] * w.shape[3] * cin + 1) * U32 * s


def glo_terms(x, w, b, net, raw=None):
    """|h16(sigmoid(.)) * net| summed over the pixels, float64 [B,Cout]"""
    s = h16(torch.sigmoid(preactivation(x, w, b, raw=raw)))
    return (s * net.double()).abs().sum((1, 2))


def glo_bound(terms_abs, n, prefill=None):
    """random weights: 2^-10 sum |sigmoid * net| per image and channel - every term may differ by one fp16 step of the
    sigmoid (tests/test_gpu_grids.py asserts this bound on the gather path) - plus n 2^-24 |prefill| for the at most n
    float32 additions into a prefilled fout.  Loose: at 774 pixels it barely notices a missing pixel, hence
    `glo_exact_bound`."""
    bound = 2.0 ** -10 * terms_abs
    return bound if prefill is None else bound + n * U32 * prefill.double().abs()


def glo_exact_bound(net, prefill=None):
    """zero weights and zero bias: sigmoid(0) = 0.5 on any implementation and 0.5 * net is exact, so only the order of the
    float32 sum is left: (n + 1) 2^-24 (|prefill| + sum |0.5 net|), n = H W.  One dropped or doubled pixel is about thirty
    times this at n = 774."""
    n = net.shape[1] * net.shape[2]
    s = (0.5 * net.double()).abs().sum((1, 2))
    if prefill is not None:
        s = s + prefill.double().abs()
    return (n + 1) * U32 * s
