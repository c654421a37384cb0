"""Sparse keypoint tracker kernels (klt_track.hip): thin wrappers over `vipe_klt_pyramid`, `vipe_klt_detect` and
`vipe_klt_track`.  include/vipe_amd.h states the arithmetic.  Device tensors only - the kernels are HIP, there is no
host path.  Everything runs on torch's current stream; nothing here synchronises."""
import torch

from .._lib import F32, check, check_gpu_contig, lib, ptr, require, stream_ptr

U8 = 3  # VIPE_U8
OOB, LOW_TEXTURE, RESIDUAL, FB, MASKED, DIVERGED = 1, 2, 4, 8, 16, 32  # VIPE_KLT_* status bits
MAX_LEVELS = 6


def pyramid_layout(H, W, levels):
    """-> ([(h, w)] per level, [offset in floats] per level, total floats) of the one-buffer pyramid"""
    require(1 <= levels <= MAX_LEVELS and H > 0 and W > 0, "levels must be 1..6 and the frame non-empty")
    sizes, offs, off = [], [], 0
    for _ in range(levels):
        sizes.append((H, W))
        offs.append(off)
        off += H * W
        H, W = (H + 1) // 2, (W + 1) // 2
    return sizes, offs, off


def _device_only(*tensors):
    if not all(t.is_cuda for t in tensors if t is not None):
        raise NotImplementedError("klt_ext: device tensors only (the tracker kernels are HIP)")


def _mask_arg(mask, H, W):
    if mask is None:
        return None
    require(mask.dtype in (torch.bool, torch.uint8) and tuple(mask.shape) == (H, W), "mask must be [H,W] bool / uint8")
    check_gpu_contig(mask)
    return mask


def pyramid(rgb, levels, out=None):
    """rgb [H,W,3] uint8 or float32 (0-1) -> the `levels`-level gray pyramid as one float32 vector (`pyramid_layout`)"""
    _device_only(rgb, out)
    require(rgb.dim() == 3 and rgb.shape[2] == 3 and rgb.dtype in (torch.uint8, torch.float32), "rgb must be [H,W,3] uint8 / float32")
    H, W = int(rgb.shape[0]), int(rgb.shape[1])
    total = pyramid_layout(H, W, levels)[2]
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=rgb.device)
    require(out.dtype == torch.float32 and out.numel() == total, "out must hold the whole pyramid as float32")
    check_gpu_contig(rgb, out)
    check(lib().vipe_klt_pyramid(ptr(rgb), U8 if rgb.dtype == torch.uint8 else F32, H, W, levels, ptr(out), stream_ptr(rgb)),
          "klt_pyramid")
    return out


def detect(img, cell, border, min_eig, mask=None, cell_busy=None, out=None):
    """img [H,W] float32 (level 0 of a pyramid) -> [ncy*ncx,3] float32 (x, y, response) per cell, x = -1 where the cell is
    busy or has no corner"""
    _device_only(img, mask, cell_busy, out)
    require(img.dim() == 2 and img.dtype == torch.float32, "img must be [H,W] float32")
    H, W = int(img.shape[0]), int(img.shape[1])
    n_cells = -(-H // cell) * -(-W // cell)
    mask = _mask_arg(mask, H, W)
    if cell_busy is not None:
        require(cell_busy.dtype == torch.uint8 and cell_busy.numel() == n_cells, "cell_busy must be uint8 [ncy*ncx]")
        check_gpu_contig(cell_busy)
    if out is None:
        out = torch.empty((n_cells, 3), dtype=torch.float32, device=img.device)
    require(out.dtype == torch.float32 and tuple(out.shape) == (n_cells, 3), "out must be [ncy*ncx,3] float32")
    check_gpu_contig(img, out)
    check(lib().vipe_klt_detect(ptr(img), H, W, ptr(mask), ptr(cell_busy), cell, border, min_eig, ptr(out), stream_ptr(img)),
          "klt_detect")
    return out


def track(pyr_a, pyr_b, H, W, levels, pts, *, win_radius, n_iters, eps, border, min_eig, max_residual, fb_thresh, max_flow,
          mask=None, fb_ref=None, status=None, cell=0, cell_busy=None, out=None, resid=None):
    """Tracks pts [N,2] from pyramid A to pyramid B -> (out [N,2], status [N] uint8, resid [N]).

    Forward pass: fb_ref None, `status` is written (mask = the usable pixels of frame B).  Backward pass: the pyramids
    swapped, pts the forward results, fb_ref the original points, `status` the forward pass's (updated in place with the
    FB bit); with `cell_busy` the cells (of `cell` pixels) of the points that end with status 0 are set to 1."""
    _device_only(pyr_a, pyr_b, pts, mask, fb_ref, status, cell_busy, out, resid)
    total = pyramid_layout(H, W, levels)[2]
    require(pyr_a.dtype == pyr_b.dtype == torch.float32 and pyr_a.numel() == pyr_b.numel() == total, "pyramids must be float32 of the layout's size")
    require(pts.dim() == 2 and pts.shape[1] == 2 and pts.dtype == torch.float32, "pts must be [N,2] float32")
    N = int(pts.shape[0])
    dev = pts.device
    out = torch.empty((N, 2), dtype=torch.float32, device=dev) if out is None else out
    resid = torch.empty(N, dtype=torch.float32, device=dev) if resid is None else resid
    if fb_ref is None:
        status = torch.empty(N, dtype=torch.uint8, device=dev) if status is None else status
    else:
        require(status is not None, "the backward pass updates the forward pass's status")
        require(tuple(fb_ref.shape) == (N, 2) and fb_ref.dtype == torch.float32, "fb_ref must be [N,2] float32")
    require(tuple(out.shape) == (N, 2) and out.dtype == torch.float32, "out must be [N,2] float32")
    require(tuple(resid.shape) == (N,) and resid.dtype == torch.float32, "resid must be [N] float32")
    require(tuple(status.shape) == (N,) and status.dtype == torch.uint8, "status must be [N] uint8")
    mask = _mask_arg(mask, H, W)
    if cell_busy is not None:
        require(cell >= 4 and cell_busy.dtype == torch.uint8 and cell_busy.numel() == -(-H // cell) * -(-W // cell),
                "cell_busy must be uint8 [ncy*ncx]")
    check_gpu_contig(pyr_a, pyr_b, pts, out, resid, status, *[t for t in (fb_ref, cell_busy) if t is not None])
    check(lib().vipe_klt_track(ptr(pyr_a), ptr(pyr_b), H, W, levels, ptr(pts), N, ptr(fb_ref), ptr(mask), win_radius, n_iters,
                               eps, border, min_eig, max_residual, fb_thresh, max_flow, cell, ptr(out), ptr(status),
                               ptr(resid), ptr(cell_busy), stream_ptr(pts)), "klt_track")
    return out, status, resid
