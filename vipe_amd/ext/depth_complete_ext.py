"""Grid kNN scale / shift completion (depth_complete.hip) with the arguments of the reference's `kss_completer`
(priorda/depth_completion.py:341-379): the coarse, network-free stage of its map-prompted depth path - a dense
disparity prediction aligned, pixel by pixel, to the K nearest sparse samples.  A module of our own, as `klt_ext` is: the
reference has no such entry point, it composes `utils_ext.nearest_neighbours` and `torch.linalg.lstsq`.
include/vipe_amd.h states the arithmetic.  Device tensors only - the kernels are HIP, there is no host path."""
import torch

from .._lib import require


def knn_scale_shift(sparse_disparities, pred_disparities, sparse_masks, complete_masks, K=5, radius=64):
    """-> (completed, scale, shift), each [B,H,W] fp32: `sparse_disparities` where `sparse_masks` holds (and the value
    and the prediction there are finite and positive: only such a pixel can anchor a fit); where `complete_masks` holds,
    scale * `pred_disparities` + shift with (scale, shift) fitted to the `K` nearest anchors of the SAME image within
    `radius` pixels (1 to 64), weighted by 1 / distance^2; 0 elsewhere.  scale / shift are (1, 0) at anchors and (0, 0)
    where nothing was fitted.

    Against `kss_completer`: the same least-squares problem (its rows are scaled by 1 / distance, ours are the normal
    equations with 1 / distance^2), without the 1e-5 * rand it adds to the predictions; where the neighbours'
    predictions do not vary, or the fitted scale is not positive, the fit is scale only; ties at the K-th place go to
    the lower (row offset, column offset), where the reference's kd-tree order is unspecified; no anchor within
    `radius` gives 0, where the reference searches the whole image.  The reference's search ignores the batch index
    (`knn_aligns` passes only the (x, y) columns to `nearest_neighbours`), so with B > 1 it mixes the samples of all
    images; here every image is completed on its own."""
    from ..slam.ingest import depth_complete
    s, p = sparse_disparities, pred_disparities
    if not (torch.is_tensor(s) and torch.is_tensor(p) and s.is_cuda and p.is_cuda):
        raise NotImplementedError("knn_scale_shift: device tensors only (vipe_depth_complete is a HIP kernel)")
    require(s.dim() == 3 and s.dtype == torch.float32 and p.dtype == torch.float32 and p.shape == s.shape,
            "sparse_disparities / pred_disparities: [B,H,W] fp32 of one shape")
    for m, what in ((sparse_masks, "sparse_masks"), (complete_masks, "complete_masks")):
        require(torch.is_tensor(m) and m.dtype == torch.bool and m.shape == s.shape and m.device == s.device,
                f"{what}: [B,H,W] bool on the maps' device")
    sparse = torch.where(sparse_masks, s, torch.zeros((), dtype=s.dtype, device=s.device)).contiguous()
    out, scale, shift, _, _ = depth_complete(sparse, p.contiguous(), K=K, radius=radius, domain="disp",
                                             mask=complete_masks.contiguous(), want_fit=True)
    return out, scale, shift
