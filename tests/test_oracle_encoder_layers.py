"""oracle/encoder_layers.py checked on the CPU, on the very launches tests/test_gpu_encoder_layers.py feeds the kernels
(oracle/encoder_cases.py): (1) its unrounded whole network IS oracle/encoder.py::encoder_forward (pinned to the
reference classes by tests/test_oracle_golden.py); (2) a float32 evaluation of every launch lies inside every interval,
so the reference alone does not use the bounds up; (3) the intervals are narrow; (4) they discriminate: one weight element
set to zero, statistics of the wrong image, one pixel counted twice all leave them; (5) the float64 and float32
evaluations of the rounded whole network agree as they did when the GPU test's gates were chosen."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder as oenc
from oracle import encoder_cases as cases
from oracle import encoder_layers as oel
from oracle.conv_epilogues import U32, h16

CONV_IDS = [c.id for c in cases.conv_cases()]
STEM_IDS = [c.id for c in cases.stem_cases()]
FINISH_IDS = [c.id for c in cases.finish_cases()]


# ------------------------------------------------------------------------------------------------ helpers
def test_helpers_on_hand_worked_numbers():
    # epilogue order: round first, then the activation, then the residual sum, rounded and clamped again
    v = torch.tensor([[[[1.0 + 2.0 ** -11 + 2.0 ** -30, -0.3, 2.0, -2.0]]]], dtype=torch.float64)
    assert oel.epilogue(v).flatten().tolist() == [1.0 + 2.0 ** -10, float(torch.tensor(-0.3).half()), 2.0, -2.0]
    assert oel.epilogue(v, relu=1).flatten().tolist() == [1.0 + 2.0 ** -10, 0.0, 2.0, 0.0]
    res = torch.tensor([[[[-3.0, 1.0, 2.0 ** -12, 0.5]]]]).half()
    assert oel.epilogue(v, relu=1, res=res).flatten().tolist() == [0.0, 1.0, 2.0, 0.5]  # 2 + 2^-12 rounds to 2
    t = oel.epilogue(v, tanh_split=2).flatten().tolist()
    assert t[0] == float(h16(torch.tanh(torch.tensor([1.0 + 2.0 ** -10], dtype=torch.float64))))
    assert t[1] < 0 and t[2:] == [2.0, 0.0]  # tanh below the split keeps its sign, ReLU above
    # statistics of a 1 x 2 image with one channel: values 1 and 3 -> M = 2, VAR = 1, nrm = -+1 (R = (1 + 1e-5)^-1/2)
    x = torch.tensor([1.0, 3.0]).half().view(1, 1, 2, 1)
    st = torch.tensor([[[4.0, 10.0]]])
    nrm, b = oel.norm_bounds(x, st)
    R = (1.0 + 1e-5) ** -0.5
    assert torch.allclose(nrm.flatten(), torch.tensor([-R, R], dtype=torch.float64), rtol=0, atol=1e-15)
    d = (3 * U32 * 5 + 4 * U32 * 4) / (2 * (1 + 1e-5)) + 8 * U32
    assert abs(float(b.flatten()[0]) - (R * 2 * U32 * 2 * (1 + d) + R * (d + 3 * U32))) < 1e-18
    lo, mid, hi = oel.norm_interval(x, st)
    assert lo.flatten().tolist() == [0.0, float(h16(torch.tensor([R], dtype=torch.float64)))] and torch.equal(lo, hi)
    assert oel.stats_sums(x).flatten().tolist() == [4.0, 10.0]
    assert oel.stats_bound(x).flatten().tolist() == [U32 * 4, U32 * 10]
    assert oel.outside(torch.tensor([0.0, 1.0, 2.0]), torch.tensor([0.0, 1.5, 0.0]), torch.tensor([0.0, 2.0, 1.0])) == 2


def test_case_list_reaches_every_edge_it_names():
    cs = [c for c in cases.conv_cases() if not c.nchw]
    for mode in cases.MODES:
        for (k, s) in cases.KERNELS:
            sel = [c for c in cs if c.mode == mode and (c.k, c.stride) == (k, s)]
            assert {(c.Ho, c.Wo) for c in sel} == set(cases.GRIDS)
            assert {(c.cin, c.cout) for c in sel} >= set(cases.CHANNELS)
            assert {c.stats for c in sel} == {True, False}
    for (k, s) in cases.KERNELS:
        assert any(c.B == 3 for c in cs if (c.k, c.stride) == (k, s))
    for s2 in [c for c in cs if c.stride == 2]:
        assert s2.H in (2 * s2.Ho - 1, 2 * s2.Ho) and s2.W in (2 * s2.Wo - 1, 2 * s2.Wo)
    for (k, s) in ((3, 2), (1, 2)):  # every output grid from an odd and from an even input, rows and columns
        for grid in cases.GRIDS:
            sel = [c for c in cs if (c.k, c.stride, c.Ho, c.Wo) == (k, s) + grid]
            assert {c.H % 2 for c in sel} == {0, 1} and {c.W % 2 for c in sel} == {0, 1}, (k, s, grid)
    assert sum(c.prefill for c in cs) == 1
    assert {c.tanh_split for c in cases.conv_cases() if c.nchw} == {-1, 0, 128, 256}
    assert 25 <= len([c for c in cs if c.mode == "plain"]) <= 40


# ------------------------------------------------------------------------------------------------ (1) the network
@pytest.mark.parametrize("grid", cases.NET_GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("name", ["fnet", "cnet"])
def test_unrounded_emulation_is_the_reference_network(name, grid):
    """float64 round-off: fifteen layers of sums of at most 1152 products, the one-pass variance loses (q/n) / VAR ~ 10
    units of 1e-16, slopes of a few: 1e-10 of the output scale."""
    norm_fn, _, split = cases.NETS[name]
    sd = {k: v.double() for k, v in cases.net_state(name).items()}
    x = oenc.normalize_images(cases.net_images(grid).double())
    with torch.no_grad():
        ref = oenc.encoder_forward(sd, x, norm_fn)
        got = oel.emulate(sd, x, norm_fn, torch.float64, -1, rounded=False)
        assert got.shape == ref.shape == (3, ref.shape[1], grid[0] // 8 + (grid[0] % 8 > 0), grid[1] // 8 + (grid[1] % 8 > 0))
        assert float((got - ref).abs().max()) <= 1e-10 * float(ref.abs().max())
        if split >= 0:
            got = oel.emulate(sd, x, norm_fn, torch.float64, split, rounded=False)
            want = torch.cat([ref[:, :split].tanh(), ref[:, split:].relu()], 1)
            assert float((got - want).abs().max()) <= 1e-10


# ------------------------------------------------------------------------------------------------ (2) float32 inside
def _sum32_in_random_order(y, prefill, g):
    """[B,C,2]: float32 sums of the terms y and y^2, added one after the other in a random order (after the prefill)"""
    v = y.float().flatten(1, 2)
    v = v[:, torch.randperm(v.shape[1], generator=g)]
    out = []
    for j, t in enumerate((v, v * v)):
        t = t.numpy()
        if prefill is not None:
            t = np.concatenate([prefill[:, None, :, j].numpy().astype(np.float32), t], 1)
        out.append(torch.from_numpy(np.cumsum(t, axis=1, dtype=np.float32)[:, -1].copy()))
    return torch.stack(out, -1)


def _conv_f32(o, **kw):
    c = o.case
    a = dict(relu=c.relu, tanh_split=c.tanh_split, res=o.res, in_stats=o.in_stats)
    a.update(kw)
    w = a.pop("w", o.w)
    return oel.conv_f32(o.x, w, o.bias, c.stride, **a)


@pytest.mark.parametrize("cid", CONV_IDS + STEM_IDS)
def test_float32_evaluation_lies_inside_every_interval(cid):
    o, ref = cases.operands(cid), cases.reference(cid)
    got = _conv_f32(o)
    assert got.shape == ref.lo.shape == (o.case.B, o.case.Ho, o.case.Wo, o.case.cout)
    assert bool((ref.lo <= ref.hi).all())
    assert oel.outside(got, ref.lo, ref.hi) == 0
    if o.case.stats:
        y0 = _conv_f32(o, relu=0, tanh_split=-1, res=None)  # the value the statistics are taken of
        st = _sum32_in_random_order(y0, o.prefill, torch.Generator().manual_seed(1))
        want = oel.stats_sums(y0) + (0 if o.prefill is None else o.prefill.double())
        assert bool(((st.double() - want).abs() <= oel.stats_bound(y0, o.prefill)).all())


@pytest.mark.parametrize("cid", FINISH_IDS)
def test_float32_finish_lies_inside_its_interval(cid):
    o = cases.finish_operands(cid)
    lo, hi = cases.finish_reference(cid)
    assert bool((lo <= hi).all())
    assert oel.outside(oel.finish_f32(o.raw, o.raw_stats, o.res, o.res_stats), lo, hi) == 0


def test_prep_is_the_rounded_float64_value_almost_everywhere():
    """the float32 route of `prep` (what the kernel does, bit for bit) against (img - mean) / std in float64 rounded once:
    they may differ only where the float32 quotient falls on the other side of an fp16 tie - by one fp16 step, and rarely"""
    img = cases.prep_image(cases.PREP_CASES[1])
    got = oel.prep(img)
    assert float(got[..., 3].abs().max()) == 0.0 and got.dtype == torch.float16
    mean = torch.tensor(oel.MEAN, dtype=torch.float32).double().view(1, 3, 1, 1)
    std = torch.tensor(oel.STD, dtype=torch.float32).double().view(1, 3, 1, 1)
    want = h16(((img.double() - mean) / std).permute(0, 2, 3, 1))
    diff = (got[..., :3].double() - want).abs()
    assert float(diff.max()) <= 2.0 ** -9 and float((diff > 0).double().mean()) < 1e-3  # |values| < 4: a step is 2^-9


# ------------------------------------------------------------------------------------------------ (3) narrow
def _fp16_step(a):
    """the spacing of fp16 at magnitude a (float64 tensor)"""
    _, e = torch.frexp(a.abs().clamp(min=2.0 ** -14))
    return torch.exp2((e - 11).double())


def _one_step_wide(lo, hi):
    """An interval that is not a point is one fp16 step wide - wherever a step is at least 2 b.  The absolute term of b,
    the rounding of the mean R 2 U32 |M| ~ 1.2e-7 |M| R, does not shrink with the value, while the fp16 spacing does:
    below 2^-10 (spacing 2^-20 and less; |M| R <= 2 in the cases) an interval may span several of the finer steps.  There
    it is held to 2^-20 absolute, the step at 2^-10, and such elements are rare (|nrm| < 1e-3: 8e-4 of a normal sample)."""
    big = torch.maximum(lo.abs(), hi.abs())
    wide = hi - lo
    assert bool((wide <= torch.where(big >= 2.0 ** -10, _fp16_step(big), torch.full_like(big, 2.0 ** -20))).all())
    assert float((wide > _fp16_step(big)).double().mean()) <= 1e-3


@pytest.mark.parametrize("cid", [c.id for c in cases.conv_cases() if c.mode == "norm"])
def test_normalised_operand_is_a_point_almost_everywhere(cid):
    ref = cases.reference(cid)
    share = float((ref.x_lo != ref.x_hi).double().mean())
    print("NARROW %s: %.2f %% of the operand's elements are not a point" % (cid, 100 * share))
    assert share <= 0.02
    _one_step_wide(ref.x_lo, ref.x_hi)


@pytest.mark.parametrize("cid", FINISH_IDS)
def test_finish_interval_is_one_step_wide_at_most(cid):
    """Each normalised operand's interval is one step of ITS magnitude wide where it is not a point.  The sum with the
    shortcut can be smaller than its operands (cancellation), where the same width is many of the sum's finer steps: the
    output's interval is held to the operands' widths plus one step of its own for the final rounding (half a step at
    either end), which is one step wherever the operands are points."""
    o = cases.finish_operands(cid)
    lo, hi = cases.finish_reference(cid)
    y_lo, _, y_hi = oel.norm_interval(o.raw, o.raw_stats)
    _one_step_wide(y_lo, y_hi)
    if o.res is None:
        assert torch.equal(lo, y_lo) and torch.equal(hi, y_hi)
        return
    wx = torch.zeros_like(lo)
    if o.res_stats is not None:
        x_lo, _, x_hi = oel.norm_interval(o.res, o.res_stats, relu=False)
        _one_step_wide(x_lo, x_hi)
        wx = x_hi - x_lo
    assert bool(((hi - lo) <= (y_hi - y_lo) + wx + _fp16_step(torch.maximum(lo.abs(), hi.abs()))).all())
    assert bool(((hi == lo) | (y_hi != y_lo) | (wx != 0)).all())  # point operands give a point
    assert float((lo != hi).double().mean()) <= 0.02


# ------------------------------------------------------------------------------------------------ (4) discriminating
def _first_per_kernel_and_cin(mode):
    seen, out = set(), []
    for c in cases.conv_cases() + cases.stem_cases():
        key = (c.k, c.stride, c.cin)
        if c.mode == mode and not c.nchw and key not in seen:
            seen.add(key)
            out.append(c.id)
    return out


@pytest.mark.parametrize("cid", _first_per_kernel_and_cin("plain"))
def test_one_zeroed_weight_element_leaves_the_interval(cid):
    """a seeded element (output channel, input channel, tap); the outputs it reaches: its output channel at the pixels
    whose tap lies inside the image"""
    o, ref = cases.operands(cid), cases.reference(cid)
    c = o.case
    g = cases._gen("zeroed", cid)
    co, ci, ky, kx = [int(torch.randint(n, (1,), generator=g)) for n in (c.cout, c.cin, c.k, c.k)]
    w = o.w.clone()
    w[co, ci, ky, kx] = 0
    got = _conv_f32(o, w=w)[..., co].double()
    tap = torch.zeros(1, 1, c.k, c.k, dtype=torch.float64)
    tap[0, 0, ky, kx] = 1
    reached = F.conv2d((o.x[..., ci] != 0).double()[:, None], tap, stride=c.stride, padding=c.k // 2)[:, 0] > 0
    out = (got < ref.lo[..., co]) | (got > ref.hi[..., co])
    assert int(reached.sum()) >= 0.4 * reached.numel() and not bool((out & ~reached).any())
    share = float(out[reached].double().mean())
    print("zeroed %s w[%d,%d,%d,%d] = %.3f: %.1f %% of %d reached outputs leave" % (
        cid, co, ci, ky, kx, float(o.w[co, ci, ky, kx]), 100 * share, int(reached.sum())))
    assert share >= 0.5


@pytest.mark.parametrize("cid", _first_per_kernel_and_cin("norm"))
def test_statistics_of_the_wrong_image_leave_the_interval(cid):
    o, ref = cases.operands(cid), cases.reference(cid)
    got = _conv_f32(o, in_stats=o.in_stats.roll(1, 0))
    assert oel.outside(got, ref.lo, ref.hi) >= 0.5 * got.numel()


def test_one_pixel_counted_twice_leaves_the_statistics_bound():
    """the pixel of median magnitude of every (image, channel), counted twice or dropped, moves both sums out of the bound"""
    for c in cases.conv_cases() + cases.stem_cases():
        if not c.stats:
            continue
        o = cases.operands(c.id)
        y0 = _conv_f32(o, relu=0, tanh_split=-1, res=None)
        med = y0.double().flatten(1, 2).abs().median(1).values  # [B,C]
        assert bool((torch.stack([med, med * med], -1) > oel.stats_bound(y0, o.prefill)).all()), c.id


# ------------------------------------------------------------------------------------------------ (5) the two references
@pytest.mark.parametrize("grid", cases.NET_GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("name", ["fnet", "cnet"])
def test_rounded_emulations_agree_as_measured(name, grid):
    """Measured when this was written (s_max, s_rms relative to the output scale): see the figures this test prints
    (`pytest -s`) and DESIGN.md section 2.  3e-3 is twice the largest s_max."""
    e64, e32 = cases.net_reference(name, grid)
    s_max, s_rms = cases.spread(e64, e32)
    scale = float(e64.abs().max())
    print("SPREAD %s %dx%d: scale %.3f s_max %.3e (%.2e of scale) s_rms %.3e (%.2e of scale)" % (
        name, grid[0], grid[1], scale, s_max, s_max / scale, s_rms, s_rms / scale))
    assert 0 < s_max <= 3e-3 * scale
