"""grounding_dino_ext on the MI355X: the multi-scale deformable attention kernels (csrc/ms_deform_attn.hip) against the
reference fixture (tests/golden/ms_deform_attn_reference.npz, made by the reference's own grid_sample composition),
against a float64 grid_sample composition on the GPU at GroundingDINO's encoder / decoder sizes and over a shape sweep,
and through autograd.gradcheck."""

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ms_deform_attn_reference.npz")
ENCODER_LEVELS = [(94, 167), (47, 84), (24, 42), (12, 21)]  # 16:9 video resized to a short side of 800


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def gd():
    from vipe_amd.ext import grounding_dino_ext
    return grounding_dino_ext


def compose(value, shapes, loc, attn):
    """multi_scale_deformable_attn_pytorch restated: per level grid_sample (zeros, align_corners=False) on 2 loc - 1."""
    bs, _, heads, C = value.shape
    _, Lq, _, L, P, _ = loc.shape
    vals = value.split([h * w for h, w in shapes], dim=1)
    grids = 2 * loc - 1
    sampled = []
    for lvl, (h, w) in enumerate(shapes):
        v = vals[lvl].flatten(2).transpose(1, 2).reshape(bs * heads, C, h, w)
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False))
    a = attn.transpose(1, 2).reshape(bs * heads, 1, Lq, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * a).sum(-1).view(bs, heads * C, Lq)
    return out.transpose(1, 2).contiguous()


def meta(shapes, device):
    ss = torch.tensor(shapes, dtype=torch.int64, device=device)
    areas = ss[:, 0] * ss[:, 1]
    return ss, torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])


def problem(bs, Lq, heads, C, shapes, P, dtype=torch.float32, seed=0, lo=-0.1, hi=1.1, off_kinks=False):
    """off_kinks: pixel positions with fractional parts in [0.02, 0.98].  The location gradient jumps at integer pixel
    positions; in float32 a position within rounding of one may land on the other side than in the float64 oracle."""
    g = torch.Generator().manual_seed(seed)
    Lv = sum(h * w for h, w in shapes)
    L = len(shapes)
    value = torch.randn(bs, Lv, heads, C, generator=g, dtype=torch.float64)
    loc = torch.rand(bs, Lq, heads, L, P, 2, generator=g, dtype=torch.float64) * (hi - lo) + lo
    if off_kinks:
        size = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float64).view(1, 1, 1, L, 1, 2)
        pix = loc * size - 0.5
        pix = pix.floor() + 0.02 + 0.96 * torch.rand(pix.shape, generator=g, dtype=torch.float64)
        loc = ((pix + 0.5) / size).float().double()
        x32 = loc.float() * size.float() - 0.5  # the kernel's float32 pixel positions
        assert ((x32 - x32.floor() > 0.01) & (x32 - x32.floor() < 0.99)).all()
    attn = torch.rand(bs, Lq, heads, L, P, generator=g, dtype=torch.float64)
    attn = attn / attn.sum((-1, -2), keepdim=True)
    gout = torch.randn(bs, Lq, heads * C, generator=g, dtype=torch.float64)
    d = dev()
    return [t.to(d, dtype) for t in (value, loc, attn, gout)]


def reference(value, shapes, loc, attn, gout):
    """float64 composition on the GPU: output and the three gradients"""
    v, l, a = (t.detach().double().requires_grad_() for t in (value, loc, attn))
    out = compose(v, shapes, l, a)
    out.backward(gout.double())
    return out.detach(), v.grad, l.grad, a.grad


def run(value, shapes, loc, attn, gout, step=64):
    ss, lsi = meta(shapes, value.device)
    out = gd().ms_deform_attn_forward(value, ss, lsi, loc, attn, step)
    grads = gd().ms_deform_attn_backward(value, ss, lsi, loc, attn, gout, step)
    return [out] + list(grads)


def rel_err(got, want):
    return ((got.double() - want.double()).abs().max() / want.double().abs().max().clamp(min=1e-30)).item()


NAMES = ("output", "grad_value", "grad_sampling_loc", "grad_attn_weight")


def fixture_cases():
    d = np.load(FIXTURE)
    return {str(n): {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(f"{n}/")} for n in d["cases"]}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", ["multi_level", "one_head_c32", "c32_heads8", "single_level_p1"])
def test_reference_fixture(case, dtype):
    c = fixture_cases()[case]
    d = dev()
    T = lambda k: torch.from_numpy(c[k]).to(d, dtype)  # noqa: E731
    ss = torch.from_numpy(c["spatial_shapes"]).to(d)
    lsi = torch.from_numpy(c["level_start_index"]).to(d)
    value, loc, attn = T("value"), T("sampling_loc"), T("attn_weight")
    out = gd().ms_deform_attn_forward(value, ss, lsi, loc, attn, 64)
    grads = gd().ms_deform_attn_backward(value, ss, lsi, loc, attn, T("grad_output"), 64)
    assert out.shape == c["output"].shape and out.dtype == dtype
    for name, got in zip(NAMES, [out] + list(grads)):
        want = torch.from_numpy(c[name])
        assert got.shape == want.shape, name
        if dtype == torch.float64:
            err = (got.cpu() - want).abs().max().item()
            assert err < 1e-10, (case, name, err)
        else:
            err = rel_err(got.cpu(), want)
            assert err < (1e-5 if name == "output" else 1e-4), (case, name, err)


class _MSDA(torch.autograd.Function):
    @staticmethod
    def forward(ctx, value, ss, lsi, loc, attn):
        ctx.save_for_backward(value, ss, lsi, loc, attn)
        return gd().ms_deform_attn_forward(value, ss, lsi, loc, attn, 64)

    @staticmethod
    def backward(ctx, g):
        value, ss, lsi, loc, attn = ctx.saved_tensors
        gv, gl, ga = gd().ms_deform_attn_backward(value, ss, lsi, loc, attn, g.contiguous(), 64)
        return gv, None, None, gl, ga


def test_gradcheck_float64():
    d = dev()
    shapes = [(3, 4), (2, 2)]
    ss, lsi = meta(shapes, d)
    g = torch.Generator().manual_seed(3)
    bs, Lq, heads, C, P = 2, 3, 2, 3, 2
    value = torch.randn(bs, 16, heads, C, generator=g, dtype=torch.float64)
    # pixel positions with fractional parts in [0.15, 0.85] (away from the corners' kinks), some in the border band (-1, 0)
    locs = []
    for h, w in shapes:
        px = torch.randint(-1, w, (bs, Lq, heads, P), generator=g) + torch.rand(bs, Lq, heads, P, generator=g) * 0.7 + 0.15
        py = torch.randint(-1, h, (bs, Lq, heads, P), generator=g) + torch.rand(bs, Lq, heads, P, generator=g) * 0.7 + 0.15
        locs.append(torch.stack([(px + 0.5) / w, (py + 0.5) / h], -1).double())
    loc = torch.stack(locs, 3)
    attn = torch.rand(bs, Lq, heads, 2, P, generator=g, dtype=torch.float64)
    args = [t.to(d).requires_grad_() for t in (value, loc, attn)]
    assert torch.autograd.gradcheck(lambda v, l, a: _MSDA.apply(v, ss, lsi, l, a), args, eps=1e-6, atol=1e-7,
                                     nondet_tol=1e-12)  # grad_value: atomics, order-dependent last bits


@pytest.mark.parametrize("Lq", [None, 900], ids=["encoder", "decoder"])
def test_groundingdino_sizes_float32(Lq):
    Lv = sum(h * w for h, w in ENCODER_LEVELS)
    value, loc, attn, gout = problem(1, Lq or Lv, 8, 32, ENCODER_LEVELS, 4, seed=11, off_kinks=True)
    got = run(value, ENCODER_LEVELS, loc, attn, gout, step=64)
    want = reference(value, ENCODER_LEVELS, loc, attn, gout)
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == torch.float32 and a.shape == b.shape, name
        err = rel_err(a, b)
        assert err < (1e-5 if name == "output" else 1e-4), (name, err)


SWEEP = [(C, heads, L, P) for C in (1, 24, 32, 64, 96) for heads in (1, 3, 8) for L in (1, 5) for P in (1, 8)]


@pytest.mark.parametrize("C,heads,L,P", SWEEP)
def test_shape_sweep_float64(C, heads, L, P):
    shapes = [(5, 7), (3, 4), (1, 6), (2, 1), (4, 4)][:L]
    step = (1, 2, 64)[SWEEP.index((C, heads, L, P)) % 3]
    value, loc, attn, gout = problem(2, 7, heads, C, shapes, P, torch.float64, seed=C * 100 + heads * 10 + L + P)
    got = run(value, shapes, loc, attn, gout, step=step)
    want = reference(value, shapes, loc, attn, gout)
    for name, a, b in zip(NAMES, got, want):
        err = (a - b).abs().max().item()
        assert err < 1e-10, (name, err)


def test_edges_and_far_outside_samples():
    d = dev()
    shapes = [(4, 6), (1, 3)]
    value, loc, attn, gout = problem(2, 6, 8, 32, shapes, 4, torch.float64, seed=5)
    edge = torch.tensor([0.0, 1.0], dtype=torch.float64, device=d)
    loc[:, :3] = edge[torch.randint(0, 2, loc[:, :3].shape, generator=torch.Generator().manual_seed(1))].to(d)
    got = run(value, shapes, loc, attn, gout)
    want = reference(value, shapes, loc, attn, gout)
    for name, a, b in zip(NAMES, got, want):
        assert (a - b).abs().max().item() < 1e-10, name
    # every sample far outside: nothing is read, every output and gradient is zero
    far = torch.tensor([-1e6, -3.0, -1.0, 2.0, 7.5, 1e6], dtype=torch.float64, device=d)
    loc_far = far[torch.randint(0, 6, loc.shape, generator=torch.Generator().manual_seed(2))].to(d)
    # one coordinate inside is not enough: the other one keeps the sample outside
    loc_far[..., 0] = torch.where(torch.arange(loc.shape[-2], device=d) % 2 == 0, 0.5, loc_far[..., 0])
    loc_far[..., 1] = torch.where(torch.arange(loc.shape[-2], device=d) % 2 == 0, -2.0, loc_far[..., 1])
    for t in run(value, shapes, loc_far.contiguous(), attn, gout):
        assert t.abs().max().item() == 0.0
    # a level whose start lies beyond value contributes nothing (and reads nothing)
    ss, lsi = meta(shapes, d)
    lsi_bad = lsi.clone()
    lsi_bad[1] = value.shape[1] + 1000
    out_bad = gd().ms_deform_attn_forward(value, ss, lsi_bad, loc, attn, 64)
    attn0 = attn.clone()
    attn0[:, :, :, 1] = 0
    out_ref = gd().ms_deform_attn_forward(value, ss, lsi, loc, attn0, 64)
    assert (out_bad - out_ref).abs().max().item() < 1e-12


def test_loc_and_attn_gradients_bitwise_reproducible():
    value, loc, attn, gout = problem(1, 4000, 8, 32, ENCODER_LEVELS, 4, seed=7)
    a = run(value, ENCODER_LEVELS, loc, attn, gout)
    b = run(value, ENCODER_LEVELS, loc, attn, gout)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_error_paths_and_empty_queries():
    d = dev()
    shapes = [(3, 4), (2, 2)]
    value, loc, attn, gout = problem(2, 5, 2, 8, shapes, 2)
    ss, lsi = meta(shapes, d)
    f = gd().ms_deform_attn_forward
    with pytest.raises(RuntimeError):
        f(value.half(), ss, lsi, loc.half(), attn.half(), 64)
    with pytest.raises(RuntimeError):
        f(value.transpose(1, 2), ss, lsi, loc, attn, 64)
    with pytest.raises(RuntimeError):
        f(value, ss.int(), lsi, loc, attn, 64)
    with pytest.raises(RuntimeError):
        f(value, ss.cpu(), lsi, loc, attn, 64)
    v3, l3, a3, _ = problem(3, 5, 2, 8, shapes, 2)
    with pytest.raises(RuntimeError, match="must divide im2col_step"):
        f(v3, ss, lsi, l3, a3, 2)
    with pytest.raises(RuntimeError):
        gd().ms_deform_attn_backward(value, ss, lsi, loc, attn, gout.double(), 64)
    out = f(value, ss, lsi, loc[:, :0].contiguous(), attn[:, :0].contiguous(), 64)
    assert out.shape == (2, 0, 16) and out.device == value.device
    gv, gl, ga = gd().ms_deform_attn_backward(value, ss, lsi, loc[:, :0].contiguous(), attn[:, :0].contiguous(),
                                              gout[:, :0].contiguous(), 64)
    assert gv.shape == value.shape and gv.abs().max().item() == 0 and gl.numel() == 0 and ga.numel() == 0


def test_vipe_ext_loader_route():
    import vipe_ext as _C
    shapes = [(5, 6), (3, 3)]
    value, loc, attn, gout = problem(2, 9, 8, 32, shapes, 4, seed=9)
    ss, lsi = meta(shapes, value.device)
    via = _C.grounding_dino_ext.ms_deform_attn_forward(value, ss, lsi, loc, attn, 64)
    direct = gd().ms_deform_attn_forward(value, ss, lsi, loc, attn, 64)
    assert torch.equal(via, direct)
