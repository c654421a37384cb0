"""The layer kernels of the frame encoders (`vipe_enc_prep / _stem / _conv / _finish`, csrc/encoder.hip), restated in
torch float64 on the CPU, and the whole `BasicEncoder.forward_x4` sequenced from them.

ORACLE (test infrastructure).  Written from the contract in include/vipe_amd.h ("Frame encoders") and the reference
lines cited there (droid_net.py:179-232, 290-370, 510-527).  Every function takes the LOGICAL operands of one launch:

    x        NHWC fp16 input [B,H,W,Cin] (the stem: [B,H,W,3], the zero fourth lane left out)
    w, bias  OIHW weight rounded to fp16, float32 bias [Cout]
    res      NHWC fp16 [B,Ho,Wo,Cout] or None
    stats    float32 [B,C,2] (sum, sum of squares) - THE BUFFER THE KERNEL READS, whatever filled it

ONE PRINCIPLE FOR EVERY fp16 OUTPUT: AN INTERVAL, NOT A TOLERANCE.  The kernel's value before its first rounding, v,
differs from the float64 value `ref` by at most a derived `acc`; everything after it is a monotone chain E of fp16
roundings (round, ReLU or tanh, add the residual, round, ReLU).  The chain is evaluated at both ends and the device
value has to satisfy E(ref - acc) <= got <= E(ref + acc), element by element.  Nothing here comes from what a kernel
returns.

    convolution sum     acc = (K + 1) U32 A, A = conv(|x|, |w|) + |bias|, K = taps * Cin (the stem: 49 * 3): fp16
                        products are exact in float32 and any order of the K additions and the bias stays within K + 1
                        roundings of partial sums none larger than A (`partial_bound` of oracle/conv_epilogues.py, which
                        the project asserts on the device for the same matrix instruction).
    tanhf               HIP documents 2 units in the last place; taken at 2^-22 absolute (four float32 units at 1) on both
                        sides before its rounding.
    normalisation       M = s / n, VAR = max(q / n - M^2, 0), R = (VAR + 1e-5)^-1/2, nrm = (x - M) R in float64.  The
                        kernel's float32 value differs from nrm by at most
                            b = R 2 U32 |M| (1 + d) + |nrm| (d + 3 U32),
                            d = (3 U32 q/n + 4 U32 M^2) / (2 (VAR + 1e-5)) + 8 U32.
                        Where the terms come from (e_i: one float32 rounding, |e_i| <= U32):
                          inv = fl(1 / n) = (1 + e1) / n;  m = fl(s inv) = M (1 + e1 + e2): the 2 U32 |M| of b;
                          fl(q inv) = q/n (1 + e1 + e3), fl(m m) = M^2 (1 + 2 e1 + 2 e2 + e4), the difference rounds
                          with e5.  e1 enters as e1 (q/n - 2 M^2), at most U32 q/n because M^2 <= q/n; with e3 and
                          e5 VAR <= e5 q/n that is 3 U32 q/n, and 2 e2 + e4 give 3 U32 M^2 (4 is kept: the bound as it
                          was set).  The clamp at 0 moves the value towards VAR >= 0.  d(R) / R = -d(VAR) / (2 (VAR + eps)).
                          The added epsilon rounds once (U32 / 2 in R) and 1e-5f is not 1e-5 (another U32 / 2); rsqrtf
                          is documented at one unit in the last place, 2 U32.  The 8 U32 of d - rsqrtf taken at four
                          units - holds all three with 5 U32 to spare.  This is the only term that is not IEEE rounding.
                          fl(x - m) and the product with rstd round once each: the 3 U32 next to d (2, and the second
                          order terms).
                        A FLAT channel (VAR ~ 0 against M^2: a black frame's interior) makes d large - the one-pass
                        variance loses its digits to cancellation - and the interval widens accordingly; the cases stay
                        away from it.
    statistics          the sum and the sum of squares of the fp16 value before ReLU, tanh or residual.  Checked against
                        the float64 sums of the kernel's own y of a launch in which y IS that value:
                        (n - 1) U32 sum |term| per image and channel, n = the number of terms (Ho Wo, one more for a
                        non-zero prefill).  The terms are exact in float32 (a square of an fp16 value has 22 bits) and
                        any order of the n - 1 additions stays inside.  One dropped or doubled pixel is 1 / n of the
                        sum: 13 bounds at the largest n used (1125), 40 at 9 x 70.

`emulate` is the whole network: `BasicEncoder.forward_x4` with h16 at every point where a kernel stores fp16.
"""

from types import SimpleNamespace

import torch
import torch.nn.functional as F

from .conv_epilogues import U32, h16

IN_EPS = 1e-5            # nn.InstanceNorm2d default
TANH_SLACK = 2.0 ** -22  # four float32 units at 1
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ convolution sum
def conv_pre(x, w, bias, stride, dtype=torch.float64):
    """conv(x, w) + bias with padding k // 2 -> NHWC [B,Ho,Wo,Cout] in `dtype`; bias None: the bare sum"""
    v = F.conv2d(_nchw(x).to(dtype), w.to(dtype), None if bias is None else bias.to(dtype), stride=stride,
                 padding=w.shape[2] // 2)
    return _nhwc(v)


def conv_acc(x_abs, w, bias, stride):
    """(K + 1) U32 (conv(|x|, |w|) + |bias|), K = taps * Cin; `x_abs` is |x| (or a bound on it)"""
    K = w.shape[1] * w.shape[2] * w.shape[3]
    return (K + 1) * U32 * conv_pre(x_abs.double(), w.double().abs(), bias.double().abs(), stride)


def epilogue(v, relu=0, tanh_split=-1, res=None, side=0, rounded=True):
    """The chain E of the convolution kernels, in the kernel's order, on NHWC `v` (any float dtype):
    h = h16(v); tanh_split >= 0: h16(tanh(h)) below the split, relu(h) above; else relu(h) if `relu`; with `res`:
    relu(h16(res + o)).  side = -1 / +1 widens tanh by TANH_SLACK downwards / upwards before its rounding (the two ends
    of an interval), 0 is the plain value.  res + o is exact in float64 and the kernel's float32 sum, where it is not
    exact, rounds to the same fp16 value: it happens only when one operand is below 2^-13 of the other's step."""
    r = h16 if rounded else (lambda t: t)
    h = r(v)
    if tanh_split >= 0:
        h = torch.cat([r(torch.tanh(h[..., :tanh_split]) + side * TANH_SLACK), torch.relu(h[..., tanh_split:])], -1)
    elif relu:
        h = torch.relu(h)
    if res is not None:
        h = torch.relu(r(res.to(h.dtype) + h))
    return h


# ------------------------------------------------------------------------------------------------ normalisation
def norm_bounds(x, stats):
    """x NHWC fp16, stats [B,C,2] float32 -> (nrm, b): the float64 normalised value and the bound on the kernel's float32
    one before its fp16 rounding (module docstring)"""
    B, H, W, C = x.shape
    n = H * W
    s = stats[..., 0].double().view(B, 1, 1, C)
    q = stats[..., 1].double().view(B, 1, 1, C)
    M = s / n
    var = (q / n - M * M).clamp(min=0.0)
    ve = var + IN_EPS
    R = ve ** -0.5
    nrm = (x.double() - M) * R
    d = (3 * U32 * q / n + 4 * U32 * M * M) / (2 * ve) + 8 * U32
    b = R * 2 * U32 * M.abs() * (1 + d) + nrm.abs() * (d + 3 * U32)
    return nrm, b


def norm_interval(x, stats, relu=True):
    """-> (lo, mid, hi): h16(nrm - b), h16(nrm), h16(nrm + b), each through ReLU if `relu` (normalise on load and the
    finish kernel's main operand; its normalised shortcut has no ReLU)"""
    nrm, b = norm_bounds(x, stats)
    f = torch.relu if relu else (lambda t: t)
    return f(h16(nrm - b)), f(h16(nrm)), f(h16(nrm + b))


# ------------------------------------------------------------------------------------------------ the launches
def conv_interval(x, w, bias, stride, relu=0, tanh_split=-1, res=None, in_stats=None):
    """`vipe_enc_conv` / `vipe_enc_stem` -> .lo, .hi: the interval of every output element, NHWC [B,Ho,Wo,Cout] float64
    (an NCHW launch stores the same values transposed); .ref, .acc: the value before the first rounding and its bound;
    .x_lo, .x_hi: the operand's interval when the launch normalises on load (else both are x).
    Normalise on load: the operand is the interval [lo, hi] of relu(h16(nrm -+ b)); ref = conv(relu(h16(nrm)), w) + bias,
    acc = (K + 1) U32 A' + conv(hi - lo, |w|) with A' formed from max(|lo|, |hi|) = hi.  Padding stays zero: the kernel
    normalises only pixels inside the image, and so does a convolution of the normalised tensor."""
    if in_stats is None:
        x_lo = x_hi = mid = x.double()
        acc = conv_acc(mid.abs(), w, bias, stride)
    else:
        x_lo, mid, x_hi = norm_interval(x, in_stats)
        acc = conv_acc(torch.maximum(x_lo.abs(), x_hi.abs()), w, bias, stride) + \
            conv_pre(x_hi - x_lo, w.double().abs(), None, stride)
    ref = conv_pre(mid, w, bias, stride)
    lo = epilogue(ref - acc, relu, tanh_split, res, side=-1)
    hi = epilogue(ref + acc, relu, tanh_split, res, side=+1)
    return SimpleNamespace(lo=lo, hi=hi, ref=ref, acc=acc, x_lo=x_lo, x_hi=x_hi)


def finish_interval(raw, raw_stats, res=None, res_stats=None):
    """`vipe_enc_finish`: relu(IN(raw)); relu(res + relu(IN(raw))); relu(IN(res) + relu(IN(raw))) -> (lo, hi).  Element-wise
    and monotone in both normalised operands, so the ends of the operands' intervals are the ends of the output's."""
    y_lo, _, y_hi = norm_interval(raw, raw_stats)
    if res is None:
        return y_lo, y_hi
    if res_stats is None:
        x_lo = x_hi = res.double()
    else:
        x_lo, _, x_hi = norm_interval(res, res_stats, relu=False)
    return torch.relu(h16(x_lo + y_lo)), torch.relu(h16(x_hi + y_hi))


def outside(got, lo, hi):
    """-> number of elements of `got` outside [lo, hi]"""
    g = got.double()
    return int(((g < lo) | (g > hi)).sum())


def stats_sums(y):
    """y NHWC (fp16 values) -> float64 [B,C,2]: sum and sum of squares over the pixels"""
    v = y.double().flatten(1, 2)
    return torch.stack([v.sum(1), (v * v).sum(1)], -1)


def stats_bound(y, prefill=None):
    """(n - 1) U32 sum |term| per image and channel [B,C,2]; a non-zero prefill is one more term"""
    v = y.double().flatten(1, 2)
    n = v.shape[1]
    terms = torch.stack([v.abs().sum(1), (v * v).sum(1)], -1)
    if prefill is not None:
        terms, n = terms + prefill.double().abs(), n + 1
    return (n - 1) * U32 * terms


def prep(img):
    """`vipe_enc_prep`: [V,3,H,W] float32 RGB -> [V,H,W,4] fp16, (img - mean) / std in float32 - a subtraction and a
    division, both correctly rounded on any IEEE implementation - then one rounding to fp16; the fourth lane is zero.
    Bit-exact."""
    assert img.dtype == torch.float32
    mean = torch.tensor(MEAN, dtype=torch.float32).view(1, 3, 1, 1)
    std = torch.tensor(STD, dtype=torch.float32).view(1, 3, 1, 1)
    out = torch.zeros(img.shape[0], img.shape[2], img.shape[3], 4, dtype=torch.float16)
    out[..., :3] = _nhwc((img - mean) / std).half()
    return out


# ------------------------------------------------------------------------------------------------ float32 evaluations
# What a careful float32 implementation of the same launches returns: F.conv2d in float32 on the fp16 operands, the
# normalisation in the kernel's float32 formula, the epilogue in float32.  tests/test_oracle_encoder_layers.py holds
# them to the intervals (the reference alone does not use the bounds up) and damages them (the intervals discriminate).
def norm_f32(x, stats, relu=True):
    B, H, W, C = x.shape
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(H) * float(W), dtype=torch.float32)
    s, q = stats[..., 0].float().view(B, 1, 1, C), stats[..., 1].float().view(B, 1, 1, C)
    m = s * inv
    var = (q * inv - m * m).clamp(min=0.0)
    rstd = torch.rsqrt(var + torch.tensor(IN_EPS, dtype=torch.float32))
    y = h16((x.float() - m) * rstd)
    return torch.relu(y) if relu else y


def conv_f32(x, w, bias, stride, relu=0, tanh_split=-1, res=None, in_stats=None):
    xin = x.float() if in_stats is None else norm_f32(x, in_stats)
    return epilogue(conv_pre(xin, w, bias, stride, torch.float32), relu, tanh_split, res)


def finish_f32(raw, raw_stats, res=None, res_stats=None):
    y = norm_f32(raw, raw_stats)
    if res is None:
        return y
    xr = res.float() if res_stats is None else norm_f32(res, res_stats, relu=False)
    return torch.relu(h16(xr + y))


# ------------------------------------------------------------------------------------------------ the whole network
def emulate(sd, x, norm_fn, dtype=torch.float64, tanh_split=-1, rounded=True):
    """`BasicEncoder.forward_x4` (vipe_amd/slam/encoders.py; droid_net.py:352-370, ResidualBlock :221-232) over a state
    dict with the reference's keys.  x [n,3,H,W]: the normalised image as the stem reads it (the fp16 values of
    `prep`) -> [n,out,H/8,W/8] (NCHW).  h16 at every point where a kernel stores fp16 - each convolution's output, the
    normalised value on load and in finish, the residual sum, the tanh / ReLU split - with the weights rounded to fp16;
    the statistics are those of the stored fp16 values (one pass: sum and sum of squares, as the kernels take them);
    everything between those points is evaluated in `dtype`.  rounded=False removes every h16 (weights included): the
    mathematical function, oracle/encoder.py::encoder_forward."""
    r = h16 if rounded else (lambda t: t)
    inorm = norm_fn == "instance"
    assert norm_fn in ("instance", "none")

    def conv(name, t, stride, pad):
        w, b = sd[name + ".weight"], sd[name + ".bias"]
        return r(F.conv2d(t, r(w.to(dtype)), b.to(dtype), stride=stride, padding=pad))

    def norm(t, relu=True):
        """the stored conv output -> what its consumer makes of it; norm_fn "none": the ReLU alone (fused into the
        producer's epilogue on the device, where it commutes with the rounding)"""
        if inorm:
            n = t.shape[2] * t.shape[3]
            M = t.sum((2, 3), keepdim=True) / n
            var = ((t * t).sum((2, 3), keepdim=True) / n - M * M).clamp(min=0.0)
            t = r((t - M) * (var + IN_EPS) ** -0.5)
        return torch.relu(t) if relu else t

    x = norm(conv("conv1", x.to(dtype), 2, 3))
    for li, stride in ((1, 1), (2, 2), (3, 2)):
        for bi, s in ((0, stride), (1, 1)):
            pre = "layer%d.%d" % (li, bi)
            y = norm(conv(pre + ".conv1", x, s, 1))
            y = norm(conv(pre + ".conv2", y, 1, 1))
            if s != 1:
                x = norm(conv(pre + ".downsample.0", x, s, 0), relu=False)
            x = torch.relu(r(x + y))
    h = conv("conv2", x, 1, 0)
    if tanh_split >= 0:
        h = torch.cat([r(torch.tanh(h[:, :tanh_split])), torch.relu(h[:, tanh_split:])], 1)
    return h
