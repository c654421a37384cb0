"""`vipe_ext.grounding_dino_ext` (csrc/grounding_dino_ext/vision.cpp:9-33): multi-scale deformable attention, the operator
every encoder and decoder layer of GroundingDINO calls through `MultiScaleDeformableAttnFunction`
(groundingdino/models/main/ms_deform_attn.py:40-89).  One HIP launch per call (csrc/ms_deform_attn.hip) on torch's current
stream; no host synchronisation.

Same names, argument order and checks as the reference (ms_deform_attn_cuda.cu): contiguous device tensors, int64
`spatial_shapes` / `level_start_index`, float32 or float64 data, `bs % min(bs, im2col_step) == 0` - all RuntimeError.  The
reference's non-CUDA branch raises "Not implemented on the CPU" (vision.cpp:12-15, a RuntimeError in Python); here that
is a NotImplementedError, a subclass of RuntimeError.
"""

import torch

from .._lib import DTYPE_CODE, check, lib, ptr, require, stream_ptr

_FLOAT = (torch.float32, torch.float64)


def _cpu_error(fn):
    return NotImplementedError(f"grounding_dino_ext.{fn}: Not implemented on the CPU")


def _check(fn, value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step, grad_output=None):
    """-> (bs, Lv, heads, C, L, Lq, P) after the reference's checks; raises before anything reaches the library."""
    if not torch.is_tensor(value):
        raise _cpu_error(fn)
    require(im2col_step is not None and int(im2col_step) >= 1, f"im2col_step must be positive, got {im2col_step}")
    require(value.dim() == 4, "value must be [bs, Lv, heads, C]")
    batch = int(value.shape[0])  # a condition on the arguments alone: checked before the device (both RuntimeError)
    step = min(batch, int(im2col_step))
    require(batch == 0 or batch % step == 0, f"batch({batch}) must divide im2col_step({step})")
    if not value.is_cuda:
        raise _cpu_error(fn)
    named = [("value", value), ("spatial_shapes", spatial_shapes), ("level_start_index", level_start_index),
             ("sampling_loc", sampling_loc), ("attn_weight", attn_weight)]
    backward = fn.endswith("backward")
    if backward:
        named.append(("grad_output", grad_output))
    for name, t in named:
        require(torch.is_tensor(t), f"{name} must be a tensor")
        require(t.is_contiguous(), f"{name} tensor has to be contiguous")
    for name, t in named:
        require(t.is_cuda, f"{name} must be a CUDA tensor")
        require(t.device == value.device, f"{name} must be on {value.device}")
    # AT_DISPATCH_FLOATING_TYPES: float / double only, every float tensor of the value's type
    require(value.dtype in _FLOAT, f'"{fn}_cuda" not implemented for \'{value.dtype}\'')
    for name, t in named:
        if name in ("spatial_shapes", "level_start_index"):
            require(t.dtype == torch.int64, f"{name}: expected scalar type Long but found {t.dtype}")
        elif name != "value":
            require(t.dtype == value.dtype, f"{name}: expected scalar type {value.dtype} but found {t.dtype}")
    bs, Lv, heads, C = (int(s) for s in value.shape)
    require(spatial_shapes.dim() == 2 and spatial_shapes.shape[1] == 2, "spatial_shapes must be [L, 2]")
    L = int(spatial_shapes.shape[0])
    require(tuple(level_start_index.shape) == (L,), "level_start_index must be [L]")
    require(sampling_loc.dim() == 6 and sampling_loc.shape[0] == bs and sampling_loc.shape[2] == heads
            and sampling_loc.shape[3] == L and sampling_loc.shape[5] == 2, "sampling_loc must be [bs, Lq, heads, L, P, 2]")
    Lq, P = int(sampling_loc.shape[1]), int(sampling_loc.shape[4])
    require(tuple(attn_weight.shape) == (bs, Lq, heads, L, P), "attn_weight must be [bs, Lq, heads, L, P]")
    if backward:
        require(grad_output.numel() == bs * Lq * heads * C, "grad_output must hold [bs, Lq, heads * C]")
    return bs, Lv, heads, C, L, Lq, P


def ms_deform_attn_forward(value=None, spatial_shapes=None, level_start_index=None, sampling_loc=None, attn_weight=None,
                           im2col_step=None):
    """-> output [bs, Lq, heads * C] (vision.cpp:9-16, ms_deform_attn_cuda.cu:20-72)"""
    bs, Lv, heads, C, L, Lq, P = _check("ms_deform_attn_forward", value, spatial_shapes, level_start_index, sampling_loc,
                                        attn_weight, im2col_step)
    output = torch.zeros((bs, Lq, heads * C), dtype=value.dtype, device=value.device)
    check(lib().vipe_ms_deform_attn_forward(ptr(value), ptr(spatial_shapes), ptr(level_start_index), ptr(sampling_loc),
                                            ptr(attn_weight), ptr(output), bs, Lv, heads, C, L, Lq, P,
                                            DTYPE_CODE[value.dtype], stream_ptr(value)), "ms_deform_attn_forward")
    return output


def ms_deform_attn_backward(value=None, spatial_shapes=None, level_start_index=None, sampling_loc=None, attn_weight=None,
                            grad_output=None, im2col_step=None):
    """-> [grad_value, grad_sampling_loc, grad_attn_weight] (vision.cpp:18-27, ms_deform_attn_cuda.cu:74-136)"""
    bs, Lv, heads, C, L, Lq, P = _check("ms_deform_attn_backward", value, spatial_shapes, level_start_index, sampling_loc,
                                        attn_weight, im2col_step, grad_output)
    grad_value = torch.zeros_like(value)  # accumulated by the kernel's atomics
    grad_sampling_loc = torch.zeros_like(sampling_loc)
    grad_attn_weight = torch.zeros_like(attn_weight)
    check(lib().vipe_ms_deform_attn_backward(ptr(value), ptr(spatial_shapes), ptr(level_start_index), ptr(sampling_loc),
                                             ptr(attn_weight), ptr(grad_output), ptr(grad_value), ptr(grad_sampling_loc),
                                             ptr(grad_attn_weight), bs, Lv, heads, C, L, Lq, P, DTYPE_CODE[value.dtype],
                                             stream_ptr(value)), "ms_deform_attn_backward")
    return [grad_value, grad_sampling_loc, grad_attn_weight]
