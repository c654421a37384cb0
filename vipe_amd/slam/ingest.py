"""Native-resolution frame ingest: the step the reference's `SLAMSystem.run` puts in front of the SLAM loop
(vipe/slam/system.py:42-77, 215-218, 306-309) - every stream wrapped in a `StandardResizeStreamProcessor` that rescales
each frame to an area of about 384 x 512 and centre-crops both sides to multiples of 8 (`VideoFrame.resize` / `crop`,
vipe/streams/base.py:164-254), intrinsics rescaled on the way in and recovered to the original frame size on the way out.

    StandardResize(h0, w0)     the size / crop policy and the intrinsics round trip (host arithmetic, float64)
    ingest_frames(frames, ..)  one `vipe_frame_ingest` launch per view: the native frame is read once and everything
                               `_precompute_features` / `_add_keyframe` need is written - images, the encoders'
                               normalised fp16 input, the 1/8 invalid mask, the sensor disparities
    depth_export(disp, ..)     the way back (`vipe_depth_export`): SLAM-resolution disparity maps through the inverse of
                               that crop and resize to the native size, as depth
    depth_consistency(..)      on the same grid (`vipe_depth_consistency`): per pixel of those maps, how many neighbour
                               rows see its point and how many confirm its disparity; `nearest_keyframes` picks the rows
    cloud_fuse(..)             on the same grid again (`vipe_cloud_fuse`): the pixels that count reaches `min_agree` on,
                               back-projected to the world and summed into a voxel hash table on the device;
                               `cloud_extract` (`vipe_cloud_extract`) makes one point per voxel of it
    cloud_render(..)           the way back into the cameras (`vipe_cloud_render`): points splatted into a 64-bit
                               z-buffer (`cloud_zbuffer`) on that grid; `cloud_resolve` (`vipe_cloud_resolve`) makes
                               depth, colour and index images of it
    depth_complete(..)         the last link (`vipe_depth_anchor_bits` + `vipe_depth_complete`): a sparse map - those
                               images - where it has values, elsewhere a dense prediction aligned to the K nearest sparse
                               samples by a weighted scale / shift fit in the disparity domain

Decoding stays with the caller: frames arrive as tensors.  The nearest-neighbour `instance` channel of `VideoFrame` is
not read by the SLAM path and is not carried."""
import math

import torch

from .._lib import F16, F32, check, lib, ptr, require, stream_ptr

U8 = 3  # VIPE_U8
_RGB_CODE = {torch.uint8: U8, torch.float16: F16, torch.float32: F32}


class StandardResize:
    """`StandardResizeStreamProcessor` (system.py:42-77) for frames of `h0` x `w0` pixels.

    size = (h1, w1), crop = (top, bottom, left, right), out_size = (H, W) after the crop; fac_x / fac_y / scx / scy as
    the reference keeps them for `recover_intrinsics`."""

    def __init__(self, h0, w0):
        h0, w0 = int(h0), int(w0)
        require(h0 > 0 and w0 > 0, "frame size must be positive")
        scale = math.sqrt((384 * 512) / (h0 * w0))
        h1, w1 = int(h0 * scale), int(w0 * scale)
        crop_h, crop_w = h1 % 8, w1 % 8
        top, left = crop_h // 2, crop_w // 2
        self.native_size = (h0, w0)
        self.size = (h1, w1)
        self.crop = (top, crop_h - top, left, crop_w - left)
        self.out_size = (h1 - crop_h, w1 - crop_w)
        require(self.out_size[0] > 0 and self.out_size[1] > 0, "frame too elongated: nothing is left after the crop")
        self.fac_x, self.fac_y = w0 / w1, h0 / h1
        self.scx, self.scy = left, top

    def forward_intrinsics(self, K):
        """`VideoFrame.resize` then `crop` on [fx, fy, cx, cy, (MEI xi)] (base.py:193-197, 235-239)."""
        (h0, w0), (h1, w1) = self.native_size, self.size
        K = K.clone()
        K[0:4:2] *= w1 / w0
        K[1:4:2] *= h1 / h0
        K[2] -= self.scx
        K[3] -= self.scy
        return K

    def recover_intrinsics(self, K):
        """system.py:71-77: intrinsics at SLAM resolution -> at the original frame size."""
        K = K.clone()
        K[2] += self.scx
        K[3] += self.scy
        K[0:4:2] *= self.fac_x
        K[1:4:2] *= self.fac_y
        return K


def frame_ingest(rgb, resize, images, x4, mask=None, mask8=None, depth=None, disps_sens=None):
    """One view through `vipe_frame_ingest`: rgb [H0,W0,3] uint8 / fp16 / fp32, mask [H0,W0] bool / uint8 or None,
    depth [H0,W0] fp32 or None -> images [3,H,W] fp32, x4 [H,W,4] fp16, mask8 [H/8,W/8] bool (True = invalid),
    disps_sens [H/8,W/8] fp32 (the last two only where their input is given), all preallocated by the caller."""
    (H0, W0), (h1, w1), (H, W) = resize.native_size, resize.size, resize.out_size
    require(rgb.is_cuda and rgb.is_contiguous() and tuple(rgb.shape) == (H0, W0, 3), f"rgb must be a contiguous device tensor [{H0},{W0},3]")
    require(rgb.dtype in _RGB_CODE, "rgb must be uint8, float16 or float32")
    require(tuple(images.shape) == (3, H, W) and images.dtype == torch.float32 and images.is_contiguous(), "images: [3,H,W] fp32")
    require(tuple(x4.shape) == (H, W, 4) and x4.dtype == torch.float16 and x4.is_contiguous(), "x4: [H,W,4] fp16")
    for t in (images, x4, mask, mask8, depth, disps_sens):
        require(t is None or t.device == rgb.device, "all tensors must live on the frame's device")
    if mask is not None:
        require(mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous() and tuple(mask.shape) == (H0, W0), "mask: [H0,W0] bool / uint8")
        require(mask8 is not None and mask8.dtype == torch.bool and mask8.is_contiguous()
                and tuple(mask8.shape) == (H // 8, W // 8), "mask8: [H/8,W/8] bool")
    if depth is not None:
        require(depth.dtype == torch.float32 and depth.is_contiguous() and tuple(depth.shape) == (H0, W0), "depth: [H0,W0] fp32")
        require(disps_sens is not None and disps_sens.dtype == torch.float32 and disps_sens.is_contiguous()
                and tuple(disps_sens.shape) == (H // 8, W // 8), "disps_sens: [H/8,W/8] fp32")
    top, _, left, _ = resize.crop
    check(lib().vipe_frame_ingest(ptr(rgb), _RGB_CODE[rgb.dtype], ptr(mask), ptr(depth), H0, W0, h1, w1, top, left, H, W,
                                  ptr(images), ptr(x4), ptr(mask8) if mask is not None else None,
                                  ptr(disps_sens) if depth is not None else None, stream_ptr(rgb)), "vipe_frame_ingest")


def export_params(resize_or_params, H, W):
    """-> (h1, w1, top, left, H0, W0) of `vipe_depth_export` for maps of H x W: from a `StandardResize` (whose
    `out_size` must be that size), from such a tuple as it is, or - None - the identity"""
    r = resize_or_params
    if r is None:
        return (H, W, 0, 0, H, W)
    if isinstance(r, StandardResize):
        require(r.out_size == (H, W), f"the maps are {H} x {W}, the resize's out_size is {r.out_size}")
        return (*r.size, r.crop[0], r.crop[2], *r.native_size)
    p = tuple(int(v) for v in r)
    require(len(p) == 6, "export parameters: (h1, w1, top, left, H0, W0)")
    return p


def depth_export(disp, resize_or_params, rows=None, out=None, dtype=torch.float16, depth_scale=1.0):
    """Disparity maps at SLAM resolution -> depth maps at the frames' native size, one `vipe_depth_export` launch: the
    inverse of `frame_ingest`'s geometry (the cropped band replicate-padded back, bilinear resample with
    align_corners=False, in the disparity domain), then depth = depth_scale / d where d > 0 and 0 elsewhere.

    disp [R,H,W] fp32; `resize_or_params` a `StandardResize` with out_size (H, W), a tuple (h1, w1, top, left, H0, W0)
    or None for the identity (H0 = H, W0 = W: exactly depth_scale / disp); rows int64 [N] or None (N = R, out[n] from
    disp[n]): out[n] is made from disp[rows[n]], entries outside [0, R) leave out[n] as it is; out [N,H0,W0] fp16 / fp32
    (fresh and zero-filled, of `dtype`, when None).  Device tensors only.  The single route from Python to the kernel."""
    if not disp.is_cuda:
        raise NotImplementedError("depth_export: device tensors only (vipe_depth_export is a HIP kernel)")
    require(disp.dim() == 3 and disp.dtype == torch.float32 and disp.is_contiguous(), "disp: contiguous [R,H,W] fp32")
    R, H, W = (int(v) for v in disp.shape)
    h1, w1, top, left, H0, W0 = export_params(resize_or_params, H, W)
    if rows is not None:
        require(rows.is_cuda and rows.device == disp.device and rows.dtype == torch.int64 and rows.dim() == 1
                and rows.is_contiguous(), "rows: contiguous int64 [N] on disp's device")
    N = R if rows is None else int(rows.shape[0])
    if out is None:
        out = torch.zeros((N, H0, W0), dtype=dtype, device=disp.device)
    require(out.is_cuda and out.device == disp.device and out.is_contiguous() and tuple(out.shape) == (N, H0, W0)
            and out.dtype in (torch.float16, torch.float32), f"out: contiguous [{N},{H0},{W0}] fp16 / fp32 on disp's device")
    check(lib().vipe_depth_export(ptr(disp), ptr(rows), ptr(out), F16 if out.dtype == torch.float16 else F32, N, R, H, W,
                                  h1, w1, top, left, H0, W0, float(depth_scale), stream_ptr(disp)), "vipe_depth_export")
    return out


def depth_consistency(disp, poses, rig, intrinsics, camera, resize_or_params, rows, nbr, tol, out=None):
    """Multi-view consistency count of the maps `depth_export` makes of the same `disp` and `rows`, one
    `vipe_depth_consistency` launch: per native-size pixel, how many of its map's K neighbour rows see the pixel's point
    (high nibble) and how many of those hold a disparity within `tol` (relative) of the one the point would have there
    (low nibble); `interface.unpack_depth_conf` splits the byte.  0 where the blended disparity is not positive.

    disp [R,H,W] fp32: rows of `GraphBuffer.flattened_disps_up`, row = slot * V + view; poses [R / V,7] world -> camera;
    rig [V,7]; intrinsics [V,4] ([V,5] MEI) at SLAM resolution; camera "pinhole" / "mei" / "panorama" (the panorama takes
    no crop or resize of a cropped frame: identity parameters or a pure resize); rows int64 [N] or None (out[n] from
    disp[n]), entries outside [0, R) leave out[n] as it is; nbr int64 [N,K], 1 <= K <= 8, neighbour rows, entries
    outside [0, R) (-1) or equal to the map's own row are skipped; out [N,H0,W0] uint8 (fresh and zero-filled when
    None).  Device tensors only.  The single route from Python to the kernel."""
    from .._lib import CAMERA_CODE
    if not disp.is_cuda:
        raise NotImplementedError("depth_consistency: device tensors only (vipe_depth_consistency is a HIP kernel)")
    require(camera in CAMERA_CODE, f"camera: one of {sorted(CAMERA_CODE)}")
    require(disp.dim() == 3 and disp.dtype == torch.float32 and disp.is_contiguous(), "disp: contiguous [R,H,W] fp32")
    R, H, W = (int(v) for v in disp.shape)
    h1, w1, top, left, H0, W0 = export_params(resize_or_params, H, W)
    require(rig.dim() == 2 and rig.shape[1] == 7, "rig: [V,7]")
    V = int(rig.shape[0])
    require(1 <= V <= 8 and R % V == 0, "rig: 1 to 8 views, and disp holds whole slots (R a multiple of V)")
    idim = 5 if camera == "mei" else 4
    for t, shape, what in ((poses, (R // V, 7), "poses"), (rig, (V, 7), "rig"), (intrinsics, (V, idim), "intrinsics")):
        require(t.is_cuda and t.device == disp.device and t.dtype == torch.float32 and t.is_contiguous()
                and tuple(t.shape) == shape, f"{what}: contiguous fp32 {list(shape)} on disp's device")
    if rows is not None:
        require(rows.is_cuda and rows.device == disp.device and rows.dtype == torch.int64 and rows.dim() == 1
                and rows.is_contiguous(), "rows: contiguous int64 [N] on disp's device")
    N = R if rows is None else int(rows.shape[0])
    require(nbr.is_cuda and nbr.device == disp.device and nbr.dtype == torch.int64 and nbr.dim() == 2 and nbr.is_contiguous()
            and nbr.shape[0] == N and 1 <= nbr.shape[1] <= 8, f"nbr: contiguous int64 [{N},K] on disp's device, 1 <= K <= 8")
    require(float(tol) > 0, "tol must be positive")
    if out is None:
        out = torch.zeros((N, H0, W0), dtype=torch.uint8, device=disp.device)
    require(out.is_cuda and out.device == disp.device and out.is_contiguous() and tuple(out.shape) == (N, H0, W0)
            and out.dtype == torch.uint8, f"out: contiguous [{N},{H0},{W0}] uint8 on disp's device")
    check(lib().vipe_depth_consistency(ptr(disp), ptr(poses), ptr(rig), ptr(intrinsics), idim, CAMERA_CODE[camera], ptr(rows),
                                       ptr(nbr), ptr(out), N, int(nbr.shape[1]), R, V, H, W, h1, w1, top, left, H0, W0,
                                       float(tol), stream_ptr(disp)), "vipe_depth_consistency")
    return out


def cloud_table(capacity, device):
    """An empty voxel hash table for `cloud_fuse` -> (keys [cap] int64 of -1, acc [cap,8] int32 of 0, stats [4] int64 of
    0); `capacity` a power of two."""
    cap = int(capacity)
    require(cap > 0 and cap & (cap - 1) == 0 and cap <= 1 << 30, "capacity: a power of two, at most 2^30")
    return (torch.full((cap,), -1, dtype=torch.int64, device=device), torch.zeros((cap, 8), dtype=torch.int32, device=device),
            torch.zeros(4, dtype=torch.int64, device=device))


def cloud_fuse(disp, poses, rig, intrinsics, camera, resize_or_params, rows, table, voxel, conf=None, min_agree=0, rgb=None,
               stride=1):
    """The maps `depth_export` makes of `disp` and `rows`, back-projected to the world and accumulated into the voxel hash
    `table` = (keys, acc, stats) of `cloud_table`, one `vipe_cloud_fuse` launch: a pixel takes part if x and y are
    multiples of `stride`, its blended disparity is positive and - with `conf` [N,H0,W0] uint8, `depth_consistency`'s
    output for the same rows - the low nibble of its byte is at least `min_agree`; it adds 1, its in-voxel offset in
    1/256 of `voxel` and - with `rgb` [N,H0,W0,3] uint8 / fp16 / fp32 - its colour to the slot of its voxel.  Integer
    sums: the table's content does not depend on order, chunking or run.  stats += (inserted, dropped because the table
    was full, out of range, dropped because the voxel is saturated).

    disp, poses, rig, intrinsics, camera, resize_or_params, rows as for `depth_consistency`.  Device tensors only.  The
    single route from Python to the kernel.  -> table"""
    from .._lib import CAMERA_CODE
    if not disp.is_cuda:
        raise NotImplementedError("cloud_fuse: device tensors only (vipe_cloud_fuse is a HIP kernel)")
    require(camera in CAMERA_CODE, f"camera: one of {sorted(CAMERA_CODE)}")
    require(disp.dim() == 3 and disp.dtype == torch.float32 and disp.is_contiguous(), "disp: contiguous [R,H,W] fp32")
    R, H, W = (int(v) for v in disp.shape)
    h1, w1, top, left, H0, W0 = export_params(resize_or_params, H, W)
    require(rig.dim() == 2 and rig.shape[1] == 7, "rig: [V,7]")
    V = int(rig.shape[0])
    require(1 <= V <= 8 and R % V == 0, "rig: 1 to 8 views, and disp holds whole slots (R a multiple of V)")
    idim = 5 if camera == "mei" else 4
    for t, shape, what in ((poses, (R // V, 7), "poses"), (rig, (V, 7), "rig"), (intrinsics, (V, idim), "intrinsics")):
        require(t.is_cuda and t.device == disp.device and t.dtype == torch.float32 and t.is_contiguous()
                and tuple(t.shape) == shape, f"{what}: contiguous fp32 {list(shape)} on disp's device")
    if rows is not None:
        require(rows.is_cuda and rows.device == disp.device and rows.dtype == torch.int64 and rows.dim() == 1
                and rows.is_contiguous(), "rows: contiguous int64 [N] on disp's device")
    N = R if rows is None else int(rows.shape[0])
    if conf is not None:
        require(conf.is_cuda and conf.device == disp.device and conf.dtype == torch.uint8 and conf.is_contiguous()
                and tuple(conf.shape) == (N, H0, W0), f"conf: contiguous [{N},{H0},{W0}] uint8 on disp's device")
    require(0 <= int(min_agree) <= 8, "min_agree: 0 to 8")
    if rgb is not None:
        require(rgb.is_cuda and rgb.device == disp.device and rgb.dtype in _RGB_CODE and rgb.is_contiguous()
                and tuple(rgb.shape) == (N, H0, W0, 3), f"rgb: contiguous [{N},{H0},{W0},3] uint8 / fp16 / fp32 on disp's device")
    require(1 <= int(stride) <= 8, "stride: 1 to 8")
    inv_voxel = 1.0 / float(voxel) if float(voxel) > 0 else 0.0
    require(inv_voxel > 0 and math.isfinite(inv_voxel), "voxel must be positive and finite")
    keys, acc, stats = _check_table(table, disp.device)
    check(lib().vipe_cloud_fuse(ptr(disp), ptr(poses), ptr(rig), ptr(intrinsics), idim, CAMERA_CODE[camera], ptr(rows),
                                ptr(conf), int(min_agree), ptr(rgb), _RGB_CODE[rgb.dtype] if rgb is not None else U8,
                                int(stride), inv_voxel, ptr(keys), ptr(acc), int(keys.shape[0]), ptr(stats), N, R, V, H, W,
                                h1, w1, top, left, H0, W0, stream_ptr(disp)), "vipe_cloud_fuse")
    return table


def _check_table(table, device=None):
    require(isinstance(table, (tuple, list)) and len(table) == 3, "table: (keys, acc, stats) of `cloud_table`")
    keys, acc, stats = table
    if not keys.is_cuda:
        raise NotImplementedError("the voxel hash table lives on the device (the kernels are HIP)")
    cap = int(keys.shape[0]) if keys.dim() == 1 else 0
    require(cap > 0 and cap & (cap - 1) == 0, "table keys: [cap], cap a power of two")
    for t, shape, dtype, what in ((keys, (cap,), torch.int64, "keys"), (acc, (cap, 8), torch.int32, "acc"),
                                  (stats, (4,), torch.int64, "stats")):
        require(t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape
                and t.device == (device or keys.device), f"table {what}: contiguous {dtype} {list(shape)} on the maps' device")
    return keys, acc, stats


def cloud_extract(table, voxel, min_count=1, color=True, max_out=None):
    """The table `cloud_fuse` filled -> (xyz [M,3] fp32, rgb [M,3] uint8 or None, count [M] int32, key [M] int64, num): one
    point per voxel with at least `min_count` points - the centroid, the mean colour (`color`), the number of points,
    the voxel's key - in the table's order, which means nothing (`interface.FusedCloud` sorts by key).  `num` is the
    number of such voxels.  With `max_out` None the voxels are counted first (a launch that writes nothing, one
    read-back) and the outputs hold all of them; with a number the outputs have that many rows, of which the first
    min(num, max_out) are written.  Device tensors only.  The single route from Python to `vipe_cloud_extract`."""
    keys, acc, _ = _check_table(table)
    require(float(voxel) > 0 and math.isfinite(float(voxel)), "voxel must be positive and finite")
    require(int(min_count) >= 1, "min_count: at least 1")
    require(max_out is None or int(max_out) >= 0, "max_out: None or a size")
    dev, cap = keys.device, int(keys.shape[0])
    num = torch.zeros(1, dtype=torch.int64, device=dev)

    def launch(xyz, rgb, count, key, m):
        check(lib().vipe_cloud_extract(ptr(keys), ptr(acc), cap, float(voxel), int(min_count), ptr(xyz), ptr(rgb), ptr(count),
                                       ptr(key), m, ptr(num), stream_ptr(keys)), "vipe_cloud_extract")

    if max_out is None:
        launch(None, None, None, None, 0)
        max_out = int(num.item())
    m = int(max_out)
    xyz = torch.zeros((m, 3), dtype=torch.float32, device=dev)
    rgb = torch.zeros((m, 3), dtype=torch.uint8, device=dev) if color else None
    count = torch.zeros(m, dtype=torch.int32, device=dev)
    key = torch.full((m,), -1, dtype=torch.int64, device=dev)
    launch(xyz, rgb, count, key, m)
    return xyz, rgb, count, key, int(num.item())


def render_params(resize_or_params, zbuf_size=None):
    """-> (H, W, h1, w1, top, left, H0, W0) of `vipe_cloud_render`: from a `StandardResize`, from such a tuple as it is,
    from a size (H, W) - the identity at that size - or, None, the identity at `zbuf_size`"""
    r = resize_or_params
    if r is None:
        require(zbuf_size is not None, "no geometry given")
        r = zbuf_size
    if isinstance(r, StandardResize):
        return (*r.out_size, *r.size, r.crop[0], r.crop[2], *r.native_size)
    p = tuple(int(v) for v in r)
    if len(p) == 2:
        return (*p, *p, 0, 0, *p)
    require(len(p) == 8, "render geometry: a StandardResize, (H, W) or (H, W, h1, w1, top, left, H0, W0)")
    return p


def cloud_zbuffer(B, H0, W0, device):
    """An empty z-buffer for `cloud_render` -> [B,H0,W0] int64 of -1 (all ones: as uint64 the largest value)"""
    B, H0, W0 = int(B), int(H0), int(W0)
    require(B >= 0 and H0 > 0 and W0 > 0, "z-buffer: B >= 0 images of a positive size")
    return torch.full((B, H0, W0), -1, dtype=torch.int64, device=device)


def cloud_render(xyz, cams, intrinsics, camera, resize_or_params, zbuf, point_size, max_radius=2, index_base=0, stats=None):
    """World points splatted into the z-buffer `zbuf` of `cloud_zbuffer`, one `vipe_cloud_render` launch: point m is
    carried into each of the B cameras `cams` (world -> camera rows), projected with that image's `intrinsics` row onto
    the export grid of `resize_or_params` (`render_params`: a `StandardResize`, (H, W) for the identity, the eight
    numbers, or None for the identity at the buffer's size), and every pixel of its square footprint - radius
    min(max_radius, int(0.5 * point_size * focal / depth)) pixels - takes the minimum of what it holds and
    (depth bits << 32 | index_base + m).  Integer minima: the buffer does not depend on order, chunking or run, and
    rendering twice changes nothing.  stats [3] int64 += (pairs drawn, invalid, outside the image); a fresh one when None.

    xyz [M,3] fp32; cams [B,7] fp32; intrinsics [B,4] ([B,5] MEI) at SLAM resolution; camera "pinhole" / "mei" /
    "panorama" (identity crop only); zbuf [B,H0,W0] int64.  Device tensors only.  The single route from Python to the
    kernel.  -> stats"""
    from .._lib import CAMERA_CODE
    if not (xyz.is_cuda and zbuf.is_cuda):
        raise NotImplementedError("cloud_render: device tensors only (vipe_cloud_render is a HIP kernel)")
    require(camera in CAMERA_CODE, f"camera: one of {sorted(CAMERA_CODE)}")
    require(xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.dtype == torch.float32 and xyz.is_contiguous(), "xyz: contiguous [M,3] fp32")
    require(zbuf.dim() == 3 and zbuf.dtype == torch.int64 and zbuf.is_contiguous() and zbuf.device == xyz.device,
            "zbuf: contiguous [B,H0,W0] int64 on the points' device (`cloud_zbuffer`)")
    M, (B, H0, W0) = int(xyz.shape[0]), (int(v) for v in zbuf.shape)
    H, W, h1, w1, top, left, h0, w0 = render_params(resize_or_params, (H0, W0))
    require((h0, w0) == (H0, W0), f"the z-buffer's images are {H0} x {W0}, the geometry's {h0} x {w0}")
    idim = 5 if camera == "mei" else 4
    for t, shape, what in ((cams, (B, 7), "cams"), (intrinsics, (B, idim), "intrinsics")):
        require(t.is_cuda and t.device == xyz.device and t.dtype == torch.float32 and t.is_contiguous()
                and tuple(t.shape) == shape, f"{what}: contiguous fp32 {list(shape)} on the points' device")
    require(float(point_size) >= 0 and math.isfinite(float(point_size)), "point_size: a finite length, not negative")
    require(0 <= int(max_radius) <= 4, "max_radius: 0 to 4")
    require(int(index_base) >= 0 and int(index_base) + M <= 2 ** 31 - 1, "index_base + M must stay below 2^31")
    if stats is None:
        stats = torch.zeros(3, dtype=torch.int64, device=xyz.device)
    require(stats.is_cuda and stats.device == xyz.device and stats.dtype == torch.int64 and stats.is_contiguous()
            and tuple(stats.shape) == (3,), "stats: contiguous int64 [3] on the points' device")
    check(lib().vipe_cloud_render(ptr(xyz), M, int(index_base), ptr(cams), ptr(intrinsics), idim, CAMERA_CODE[camera], B, H, W,
                                  h1, w1, top, left, H0, W0, float(point_size), int(max_radius), ptr(zbuf), ptr(stats),
                                  stream_ptr(xyz)), "vipe_cloud_render")
    return stats


def cloud_resolve(zbuf, rgb_points=None, dtype=torch.float16, want_index=False):
    """The z-buffer `cloud_render` filled -> (depth [B,H0,W0] of `dtype`, rgb [B,H0,W0,3] uint8 or None, index [B,H0,W0]
    int32 or None), one `vipe_cloud_resolve` launch: the winner's depth (0 where nothing was drawn; fp16 is the
    round-to-nearest-even of the fp32 value), with `rgb_points` [M,3] uint8 its colour (0 where nothing was drawn, and
    for an index past M), with `want_index` its index (-1 where nothing was drawn).  Device tensors only.  The single
    route from Python to the kernel."""
    if not zbuf.is_cuda:
        raise NotImplementedError("cloud_resolve: device tensors only (vipe_cloud_resolve is a HIP kernel)")
    require(zbuf.dim() == 3 and zbuf.dtype == torch.int64 and zbuf.is_contiguous(), "zbuf: contiguous [B,H0,W0] int64")
    require(dtype in (torch.float16, torch.float32), "dtype: float16 or float32")
    B, H0, W0 = (int(v) for v in zbuf.shape)
    require(H0 > 0 and W0 > 0, "zbuf: images of a positive size")
    M = 0
    if rgb_points is not None:
        require(rgb_points.is_cuda and rgb_points.device == zbuf.device and rgb_points.dtype == torch.uint8
                and rgb_points.dim() == 2 and rgb_points.shape[1] == 3 and rgb_points.is_contiguous(),
                "rgb_points: contiguous [M,3] uint8 on the buffer's device")
        M = int(rgb_points.shape[0])
    depth = torch.empty((B, H0, W0), dtype=dtype, device=zbuf.device)
    rgb = torch.empty((B, H0, W0, 3), dtype=torch.uint8, device=zbuf.device) if rgb_points is not None else None
    index = torch.empty((B, H0, W0), dtype=torch.int32, device=zbuf.device) if want_index else None
    check(lib().vipe_cloud_resolve(ptr(zbuf), B, H0, W0, ptr(depth), F16 if dtype == torch.float16 else F32,
                                   ptr(rgb_points) if M else None, M, ptr(rgb), ptr(index), stream_ptr(zbuf)),
          "vipe_cloud_resolve")
    return depth, rgb, index


_COMPLETE_DOMAIN = {"disp": 0, "depth": 1}  # VIPE_COMPLETE_*
_ANCHOR_BITS = {}  # (device, stream) -> int64 buffer the anchor bits of `depth_complete` are packed into, grown on demand


def _anchor_bits(n, device):
    """one buffer per device and stream: calls on one stream are ordered, so the next call may overwrite it"""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _ANCHOR_BITS.get(key)
    if buf is None or buf.numel() < n:
        buf = _ANCHOR_BITS[key] = torch.empty(n, dtype=torch.int64, device=device)
    return buf[:n]


def depth_complete(sparse, pred, K=5, radius=32, domain="depth", mask=None, wrap_x=False, out=None, want_fit=False,
                   want_neighbours=False, stats=None):
    """A sparse map completed by a dense prediction, one `vipe_depth_anchor_bits` and one `vipe_depth_complete` launch
    (the rule is in include/vipe_amd.h): where `sparse` and `pred` are both finite and positive - an anchor - the output is
    the sparse value, bit for bit; at every other pixel with a finite positive prediction (and `mask` non-zero, when one
    is given) it is s * pred + t in the disparity domain, (s, t) fitted to the `K` nearest anchors within `radius` pixels
    (ties: smaller distance, then lower row offset, then lower column offset) by least squares weighted with
    1 / distance^2 - affine where the neighbours' predictions vary and the scale comes out positive, scale only
    otherwise; 0 where no anchor is in reach, where the result is not positive, and where there is no prediction.
    Images are completed independently of each other.  Nothing but the counters is atomic: the same inputs give the same
    bits.

    sparse, pred [B,H,W] fp16 / fp32 of one dtype; K 1..8; radius 1..64; domain "depth" (the values are depths: fitted
    as 1 / x, returned as 1 / r) or "disp"; mask [B,H,W] bool / uint8 or None; wrap_x: the columns are a circle (the
    panorama; needs W >= 2 * radius + 1); out [B,H,W] of that dtype (fresh when None; what it held does not matter);
    stats [4] int64 += (affine, scale-only, unreached, rejected targets), a fresh one when None.  Device tensors only.
    The single route from Python to the two kernels; the bit buffer is kept per device and reused.
    -> (out, scale [B,H,W] fp32 or None, shift likewise (`want_fit`; (1, 0) at anchors, (0, 0) where the output is 0 for
    lack of a fit), neighbours [B,H,W,K] int32 or None (`want_neighbours`; pixel indices y * W + x in key order, -1
    padded), stats)"""
    if not (sparse.is_cuda and pred.is_cuda):
        raise NotImplementedError("depth_complete: device tensors only (vipe_depth_complete is a HIP kernel)")
    require(sparse.dim() == 3 and sparse.dtype in (torch.float16, torch.float32) and sparse.is_contiguous(),
            "sparse: contiguous [B,H,W] fp16 / fp32")
    B, H, W = (int(v) for v in sparse.shape)
    require(pred.device == sparse.device and pred.dtype == sparse.dtype and pred.is_contiguous() and tuple(pred.shape) == (B, H, W),
            f"pred: contiguous [{B},{H},{W}] of sparse's dtype on its device")
    require(H > 0 and W > 0 and H <= 1 << 24 and W <= 1 << 24 and H * W <= 2 ** 31 - 1 and B <= 65535,
            "images of a positive size, sides up to 2^24, fewer than 2^31 pixels each; at most 65535 of them")
    require(1 <= int(K) <= 8, "K: 1 to 8")
    require(1 <= int(radius) <= 64, "radius: 1 to 64")
    require(domain in _COMPLETE_DOMAIN, f"domain: one of {sorted(_COMPLETE_DOMAIN)}")
    require(not wrap_x or W >= 2 * int(radius) + 1, "wrap_x: the image must be at least 2 * radius + 1 columns wide")
    if mask is not None:
        require(mask.is_cuda and mask.device == sparse.device and mask.dtype in (torch.bool, torch.uint8) and mask.is_contiguous()
                and tuple(mask.shape) == (B, H, W), f"mask: contiguous [{B},{H},{W}] bool / uint8 on sparse's device")
    dev, K = sparse.device, int(K)
    if out is None:
        out = torch.empty((B, H, W), dtype=sparse.dtype, device=dev)
    require(out.is_cuda and out.device == dev and out.dtype == sparse.dtype and out.is_contiguous() and tuple(out.shape) == (B, H, W),
            f"out: contiguous [{B},{H},{W}] of sparse's dtype on its device")
    if stats is None:
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
    require(stats.is_cuda and stats.device == dev and stats.dtype == torch.int64 and stats.is_contiguous()
            and tuple(stats.shape) == (4,), "stats: contiguous int64 [4] on sparse's device")
    scale = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_fit else None
    shift = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_fit else None
    nbr = torch.empty((B, H, W, K), dtype=torch.int32, device=dev) if want_neighbours else None
    if B == 0:
        return out, scale, shift, nbr, stats
    code = F16 if sparse.dtype == torch.float16 else F32
    bits = _anchor_bits(B * H * ((W + 63) // 64), dev)
    check(lib().vipe_depth_anchor_bits(ptr(sparse), ptr(pred), code, B, H, W, ptr(bits), stream_ptr(sparse)), "vipe_depth_anchor_bits")
    check(lib().vipe_depth_complete(ptr(sparse), ptr(pred), code, ptr(mask), ptr(bits), B, H, W, _COMPLETE_DOMAIN[domain], K,
                                    int(radius), int(bool(wrap_x)), ptr(out), ptr(scale), ptr(shift), ptr(nbr), ptr(stats),
                                    stream_ptr(sparse)), "vipe_depth_complete")
    return out, scale, shift, nbr, stats


def nearest_keyframes(frame_tstamps, kf_tstamps, kf_valid, k):
    """The neighbour rule of `SLAMConfig.frame_depth_conf`, host arithmetic: for each frame the slots of the `k` keyframes
    nearest in time -> int64 [n, k].  Keyframes are ordered by |kt - t|, ties to the earlier one; a keyframe with kt == t
    is left out (a frame that is a keyframe never tests against itself), so is one whose `kf_valid` entry is false (its
    `disps_up` row is not there); short lists are padded with -1.  Slot = index into `kf_tstamps`."""
    kts = [int(t) for t in kf_tstamps]
    ok = [bool(v) for v in kf_valid]
    require(len(kts) == len(ok) and k >= 1, "one validity flag per keyframe, k >= 1")
    out = torch.full((len(frame_tstamps), k), -1, dtype=torch.int64)
    for i, t in enumerate(int(t) for t in frame_tstamps):
        order = sorted((abs(kt - t), kt, s) for s, kt in enumerate(kts) if ok[s] and kt != t)
        for j, (_, _, s) in enumerate(order[:k]):
            out[i, j] = s
    return out


def ingest_frames(frames, resize, device):
    """The per-view list of `Frame` of one time step -> (images [V,3,H,W] fp32, x4 [V,H,W,4] fp16, masks [V,h,w] bool
    True = INVALID or None, disps_sens [V,h,w] fp32 or None) at `resize.out_size`, h = H/8, w = W/8.  `resize` is one
    `StandardResize` or one per view (all of one size).  masks is None unless every view carries a mask
    (`_precompute_features`); disps_sens is None unless a view carries metric depth, and rows of views without one
    are left as allocated - the caller reads the rows of the views that have it."""
    resizes = list(resize) if isinstance(resize, (list, tuple)) else [resize] * len(frames)
    require(len(resizes) == len(frames), "one StandardResize per view")
    H, W = resizes[0].out_size
    V = len(frames)
    images = torch.empty((V, 3, H, W), dtype=torch.float32, device=device)
    x4 = torch.empty((V, H, W, 4), dtype=torch.float16, device=device)
    with_mask = all(f.mask is not None for f in frames)
    masks = torch.empty((V, H // 8, W // 8), dtype=torch.bool, device=device) if with_mask else None
    with_depth = any(f.metric_depth is not None for f in frames)
    disps = torch.empty((V, H // 8, W // 8), dtype=torch.float32, device=device) if with_depth else None
    for v, (f, r) in enumerate(zip(frames, resizes)):
        require(r.out_size == (H, W), "all views must share one size")
        rgb = f.rgb.to(device)
        if rgb.dtype not in _RGB_CODE:
            rgb = rgb.float()
        mask = f.mask.to(device).contiguous() if with_mask else None
        depth = f.metric_depth.to(device=device, dtype=torch.float32).contiguous() if f.metric_depth is not None else None
        frame_ingest(rgb.contiguous(), r, images[v], x4[v], mask, masks[v] if with_mask else None, depth,
                     disps[v] if depth is not None else None)
    return images, x4, masks, disps
