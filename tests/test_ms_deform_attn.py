"""grounding_dino_ext without a GPU: the C ABI of the multi-scale deformable attention operator, the torch restatement
that the GPU tests use as their oracle (pinned here to the reference fixture), and the host-side argument checks."""

import ctypes
import os

import numpy as np
import pytest
import torch

from vipe_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ms_deform_attn_reference.npz")
NAMES = ("vipe_ms_deform_attn_forward", "vipe_ms_deform_attn_backward")


def msda_restated(value, spatial_shapes, level_start_index, sampling_loc, attn_weight):
    """out[b,q,h*C+c] = sum_{l,p} a * bilinear(level l of value, x W - 0.5, y H - 0.5), corners outside the level zero.
    Written with explicit corner gathers (no grid_sample), so autograd gives the three gradients."""
    bs, Lv, heads, C = value.shape
    _, Lq, _, L, P, _ = sampling_loc.shape
    out = value.new_zeros(bs, Lq, heads, C)
    bidx = torch.arange(bs).view(bs, 1, 1, 1)
    hidx = torch.arange(heads).view(1, 1, heads, 1)
    for lvl in range(L):
        H, W = (int(s) for s in spatial_shapes[lvl])
        start = int(level_start_index[lvl])
        x = sampling_loc[:, :, :, lvl, :, 0] * W - 0.5  # [bs, Lq, heads, P]
        y = sampling_loc[:, :, :, lvl, :, 1] * H - 0.5
        x0, y0 = torch.floor(x), torch.floor(y)
        lx, ly = x - x0, y - y0
        acc = 0
        for dy, dx, wgt in ((0, 0, (1 - ly) * (1 - lx)), (0, 1, (1 - ly) * lx), (1, 0, ly * (1 - lx)), (1, 1, ly * lx)):
            xi, yi = x0.long() + dx, y0.long() + dy
            ok = (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)
            row = start + yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1)
            v = value[bidx, row, hidx]  # [bs, Lq, heads, P, C]
            acc = acc + (wgt * ok)[..., None] * v
        out = out + (attn_weight[:, :, :, lvl, :, None] * acc).sum(3)
    return out.reshape(bs, Lq, heads * C)


def fixture_cases():
    d = np.load(FIXTURE)
    return {str(n): {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(f"{n}/")} for n in d["cases"]}


def test_header_declares_and_library_exports_msda():
    protos = _lib.parse_header()
    for n in NAMES:
        assert n in protos, n
        restype, argtypes = protos[n]
        assert restype is ctypes.c_int and argtypes[-1] is ctypes.c_void_p  # int return, trailing stream
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(raw, n), n
    src = open(_lib.HEADER).read()
    assert "vision.cpp" in src and "ms_deform_attn_cuda.cu" in src


def test_abi_argument_errors_and_empty_problems_do_not_launch():
    L = _lib.lib()
    F32, F64, F16 = 1, 2, 0
    fwd, bwd = L.vipe_ms_deform_attn_forward, L.vipe_ms_deform_attn_backward
    # (bs, Lv, heads, C, L, Lq, P, dtype): bad sizes / dtype -> VIPE_EINVAL, before any pointer is looked at
    for args in ((1, 4, 0, 32, 1, 1, 1, F32), (1, 4, 8, 0, 1, 1, 1, F32), (1, 4, 8, 32, 0, 1, 1, F32),
                 (1, 4, 8, 32, 1, 1, 0, F32), (-1, 4, 8, 32, 1, 1, 1, F32), (1, 4, 8, 32, 1, 1, 1, F16)):
        assert fwd(None, None, None, None, None, None, *args, None) == -1, args
        assert bwd(None, None, None, None, None, None, None, None, None, *args, None) == -1, args
    # null pointers on a non-empty problem
    assert fwd(None, None, None, None, None, None, 1, 4, 8, 32, 1, 1, 1, F64, None) == -1
    # empty problems: OK without launching (there is no device here)
    assert fwd(None, None, None, None, None, None, 0, 4, 8, 32, 4, 10, 4, F32, None) == 0
    assert fwd(None, None, None, None, None, None, 1, 4, 8, 32, 4, 0, 4, F32, None) == 0
    assert bwd(None, None, None, None, None, None, None, None, None, 1, 4, 8, 32, 4, 0, 4, F64, None) == 0


@pytest.mark.parametrize("case", ["multi_level", "one_head_c32", "c32_heads8", "single_level_p1"])
def test_restatement_reproduces_reference_fixture(case):
    """The oracle of the GPU tests equals the reference's grid_sample composition: output and all three gradients."""
    c = fixture_cases()[case]
    value = torch.from_numpy(c["value"]).requires_grad_()
    loc = torch.from_numpy(c["sampling_loc"]).requires_grad_()
    attn = torch.from_numpy(c["attn_weight"]).requires_grad_()
    out = msda_restated(value, torch.from_numpy(c["spatial_shapes"]), torch.from_numpy(c["level_start_index"]), loc, attn)
    out.backward(torch.from_numpy(c["grad_output"]))
    for name, got in (("output", out), ("grad_value", value.grad), ("grad_sampling_loc", loc.grad),
                      ("grad_attn_weight", attn.grad)):
        err = np.abs(got.detach().numpy() - c[name]).max()
        assert err < 1e-12, (case, name, err)


def test_fixture_covers_edges_and_outside_samples():
    for c in fixture_cases().values():
        loc = c["sampling_loc"]
        assert (loc < 0).any() and (loc > 1).any()
        assert c["value"].shape[0] == 2 and c["value"].dtype == np.float64
    shapes = np.concatenate([c["spatial_shapes"] for c in fixture_cases().values()])
    assert (shapes == 1).any()


def _cpu_args(bs=2, Lq=3, heads=2, C=4, P=2):
    ss = torch.tensor([[3, 4], [1, 2]])
    lsi = torch.tensor([0, 12])
    value = torch.zeros(bs, 14, heads, C, dtype=torch.float64)
    loc = torch.rand(bs, Lq, heads, 2, P, 2, dtype=torch.float64)
    attn = torch.rand(bs, Lq, heads, 2, P, dtype=torch.float64)
    return value, ss, lsi, loc, attn


def test_cpu_tensors_raise_not_implemented():
    from vipe_amd.ext import grounding_dino_ext as gd
    value, ss, lsi, loc, attn = _cpu_args()
    with pytest.raises(NotImplementedError, match="Not implemented on the CPU"):
        gd.ms_deform_attn_forward(value, ss, lsi, loc, attn, 64)
    with pytest.raises(NotImplementedError, match="Not implemented on the CPU"):
        gd.ms_deform_attn_backward(value, ss, lsi, loc, attn, torch.zeros(2, 3, 8, dtype=torch.float64), 64)
    with pytest.raises(RuntimeError):  # what callers of the reference catch (AT_ERROR)
        gd.ms_deform_attn_forward(value, ss, lsi, loc, attn, 64)


def test_im2col_step_must_divide_batch_before_the_library(monkeypatch):
    from vipe_amd.ext import grounding_dino_ext as gd

    def no_library():
        raise AssertionError("the library was reached")

    monkeypatch.setattr(gd, "lib", no_library)
    value, ss, lsi, loc, attn = _cpu_args(bs=3)
    with pytest.raises(RuntimeError, match="must divide im2col_step"):
        gd.ms_deform_attn_forward(value, ss, lsi, loc, attn, 2)
    with pytest.raises(RuntimeError, match="must divide im2col_step"):
        gd.ms_deform_attn_backward(value, ss, lsi, loc, attn, torch.zeros(3, 3, 8, dtype=torch.float64), 2)


def test_vipe_ext_reexports_the_module():
    import vipe_ext as _C
    from vipe_amd.ext import grounding_dino_ext
    assert _C.grounding_dino_ext is grounding_dino_ext
    assert _C.grounding_dino_ext.ms_deform_attn_forward is grounding_dino_ext.ms_deform_attn_forward
