"""SLAM map container - host-side mirror of `SLAMMap` (vipe/slam/interface.py:25-141): the filtered dense-disparity
point cloud that `GraphBuffer.extract_slam_map` (buffer.py:595-645) produces after the update path, and its projection
into a target camera for depth alignment.  SURVEY 8(f) row 3."""
from dataclasses import dataclass

import numpy as np
import torch

from .._lib import require


@dataclass(kw_only=True)
class SLAMMap:
    dense_disp_xyz: torch.Tensor       # (M, 3)
    dense_disp_rgb: torch.Tensor       # (M, 3) RGB 0-1
    dense_disp_packinfo: torch.Tensor  # (N, V, 2) [start, count] per keyframe and view
    dense_disp_frame_inds: list        # frame index of each keyframe, sorted

    def scale(self, factor):
        self.dense_disp_xyz *= factor

    @staticmethod
    def from_masked_dense_disp(xyz, rgb, mask, tstamps):
        """xyz, rgb (N,V,H,W,3); mask (N,V,H,W); tstamps (N,)  (interface.py:40-60)"""
        assert torch.all(tstamps[1:] > tstamps[:-1]), "Timestamps should be sorted."
        N, V, H, W, C = xyz.shape
        flat = mask.reshape(-1)
        valid_count = mask.sum([2, 3]).reshape(-1)
        packinfo = torch.stack([torch.cumsum(valid_count, 0) - valid_count, valid_count], dim=-1).reshape(N, V, 2)
        return SLAMMap(dense_disp_xyz=xyz.reshape(-1, C)[flat], dense_disp_rgb=rgb.reshape(-1, C)[flat],
                       dense_disp_packinfo=packinfo, dense_disp_frame_inds=tstamps.tolist())

    def get_dense_disp_pcd(self, keyframe_idx, view_idx=-1):
        if view_idx == -1:
            parts = [self.get_dense_disp_pcd(keyframe_idx, v) for v in range(self.dense_disp_packinfo.shape[1])]
            return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)
        start, count = [int(x) for x in self.dense_disp_packinfo[keyframe_idx, view_idx]]
        return self.dense_disp_xyz[start:start + count], self.dense_disp_rgb[start:start + count]

    def get_dense_disp_full_pcd(self):
        parts = [self.get_dense_disp_pcd(k) for k in range(len(self.dense_disp_frame_inds))]
        return torch.cat([p[0] for p in parts], 0), torch.cat([p[1] for p in parts], 0)

    def project_map(self, frame_tstamp, view_idx, target_size, target_intrinsics, target_pose, infill=False, tstamp_nn=3):
        """Depth image [H,W] of the points of the keyframes around `frame_tstamp` seen from the camera whose
        camera->world pose is `target_pose` (an SE3), through a pinhole camera (interface.py:92-141).  Where several points fall into one pixel the
        reference keeps whichever its scatter writes last (unspecified); here the nearest one is kept.  `infill`: every
        pixel takes the depth of the projected point nearest to its centre (`utils_ext.nearest_neighbours`,
        interface.py:126-139)."""
        right = int(np.searchsorted(self.dense_disp_frame_inds, frame_tstamp))
        right = min(right + tstamp_nn, len(self.dense_disp_frame_inds) - 1)
        left = max(right - 2 * tstamp_nn, 0)
        xyz = torch.cat([self.get_dense_disp_pcd(k, view_idx)[0] for k in range(left, right + 1)], 0)
        # the reference transforms with target_pose.inv().matrix(): target_pose is camera->world there
        T = target_pose.inv().matrix()
        xyz = xyz @ T[:3, :3].T + T[:3, 3]
        fx, fy, cx, cy = [float(v) for v in target_intrinsics[:4]]
        z = xyz[:, 2]  # limit_min_depth=False: no clamp before the division (cameras.py:175-177)
        uu, vv = fx * xyz[:, 0] / z + cx, fy * xyz[:, 1] / z + cy
        H, W = target_size
        ok = (uu > 0) & (uu < W) & (vv > 0) & (vv < H) & (1.0 / z > 0)
        uu, vv, depth = uu[ok], vv[ok], z[ok]
        if infill:
            from ..ext import utils_ext
            tree = torch.stack((uu, vv), dim=-1).contiguous()
            qx, qy = torch.meshgrid(torch.arange(W, device=xyz.device).float() + 0.5,
                                    torch.arange(H, device=xyz.device).float() + 0.5, indexing="xy")
            query = torch.stack((qx, qy), dim=-1).reshape(-1, 2).contiguous()
            _, inds = utils_ext.nearest_neighbours(query, tree, 1)
            return depth[inds.view(-1).long()].reshape(H, W)
        out = torch.full((H * W,), float("inf"), device=xyz.device)
        out.scatter_reduce_(0, vv.floor().long() * W + uu.floor().long(), depth, reduce="amin")
        return torch.where(torch.isinf(out), torch.zeros_like(out), out).view(H, W)


def rescale_marginals(disp_var, pose_cov, s):
    """The marginals of a result that is rescaled by the metric-depth factor `s` the way `FilledReturn.scale` does it
    (disparities / s, translations * s): disparity variance / s^2; of the pose covariance [...,6,6] in the order
    (translation, rotation) the translation block * s^2, the translation-rotation blocks * s.  -> new tensors."""
    d = torch.ones(6, dtype=pose_cov.dtype, device=pose_cov.device)
    d[:3] = s
    return disp_var / (s * s), pose_cov * (d[:, None] * d[None, :])


def rescale_frame_depths(frame_depths, s):
    """`SLAMOutput.frame_depths` (or one map of a `frame_depth_sink`) of a result that is rescaled by the metric-depth
    factor `s` the way `FilledReturn.scale` does it (disparities / s, translations * s): depths * s.  `run` itself
    applies no metric rescaling, so the maps are in the trajectory's units until this is applied.  -> a new tensor of
    the same dtype (fp16 maps are scaled in fp32 and rounded once).  It fits `SLAMOutput.fused_depths` (and the maps of
    a `fused_depth_sink`) as it is: they are depths in the same units, and an empty pixel's 0 stays 0.  So it does
    `SLAMOutput.complete_depths` (and the maps of a `complete_depth_sink`): scale and shift are fitted between two maps
    in those units, so the completed depth scales with them."""
    return (frame_depths.float() * s).to(frame_depths.dtype)


class FusedCloud:
    """`SLAMOutput.fused_cloud` (`SLAMConfig.fused_cloud`): one point per occupied voxel of the clip's voxel
    hash - `xyz` [M,3] fp32 the centroid of the voxel's points (in the trajectory's units, quantised to 1/256 of a
    voxel per point), `rgb` [M,3] uint8 their mean colour or None when no colour was fed, `count` [M] int32 how many
    pixels fell in, `key` [M] int64 the voxel's index (ix + 2^20) | (iy + 2^20) << 21 | (iz + 2^20) << 42 - sorted by
    `key` (the table's own order means nothing), `voxel` the edge length, `stats` a dict of the four counters of
    `vipe_cloud_fuse`: inserted, dropped_full, out_of_range, saturated."""

    STATS = ("inserted", "dropped_full", "out_of_range", "saturated")

    def __init__(self, xyz, rgb, count, key, voxel, stats):
        key, order = torch.sort(key)
        self.xyz, self.count, self.key = xyz[order], count[order], key
        self.rgb = None if rgb is None else rgb[order]
        self.voxel = float(voxel)
        self.stats = dict(zip(self.STATS, (int(v) for v in stats))) if not isinstance(stats, dict) else dict(stats)

    def __len__(self):
        return int(self.key.shape[0])

    def voxel_index(self):
        """-> int64 [M,3]: the voxels' integer coordinates, decoded from `key`"""
        return torch.stack([((self.key >> (21 * i)) & 0x1FFFFF) - (1 << 20) for i in range(3)], dim=1)

    def render(self, cams_w2c, intrinsics, camera, size_or_resize, point_size=None, max_radius=2, dtype=torch.float16,
               color=True, want_index=False):
        """The cloud seen from B cameras: one `ingest.cloud_render` and one `ingest.cloud_resolve` launch ->
        (depth [B,H0,W0] of `dtype`, rgb [B,H0,W0,3] uint8 or None, index [B,H0,W0] int32 or None).  Per pixel the
        nearest point whose square footprint covers it - z for pinhole / MEI, the range for the panorama, in the units
        of `xyz` - 0 where nothing is drawn; with `color` (and a coloured cloud) that point's colour, with `want_index`
        its row in this cloud (-1 where nothing is drawn).

        cams_w2c [B,7] fp32 world -> camera rows (rig[v]^-1 G[f]); intrinsics [B,4] ([B,5] MEI) at SLAM resolution, or
        one row for all images; camera "pinhole" / "mei" / "panorama"; size_or_resize (H, W) - images at SLAM
        resolution - or the clip's `StandardResize` - images at the native size, pixel for pixel beside `frame_depths`;
        point_size the points' edge length (default: `voxel`); max_radius 0 to 4 pixels.  A cloud rescaled with
        `rescale_fused_cloud` renders depths in the rescaled units when it is given the rescaled cameras."""
        from . import ingest
        require(torch.is_tensor(cams_w2c) and cams_w2c.dim() == 2 and cams_w2c.shape[1] == 7, "cams_w2c: [B,7]")
        dev, B = self.xyz.device, int(cams_w2c.shape[0])
        intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32, device=dev)
        if intrinsics.dim() == 1:
            intrinsics = intrinsics[None]
        require(intrinsics.dim() == 2 and intrinsics.shape[0] in (1, B), "intrinsics: one row, or one per image")
        require(size_or_resize is not None, "size_or_resize: (H, W) or a StandardResize")
        geom = ingest.render_params(size_or_resize)
        require(point_size is None or float(point_size) >= 0, "point_size: a length, not negative")
        if not self.xyz.is_cuda:
            raise NotImplementedError("FusedCloud.render: the cloud must live on the device (vipe_cloud_render is a HIP kernel)")
        zbuf = ingest.cloud_zbuffer(B, geom[6], geom[7], dev)
        ingest.cloud_render(self.xyz.contiguous(), cams_w2c.to(device=dev, dtype=torch.float32).contiguous(),
                            intrinsics.expand(B, -1).contiguous(), camera, geom, zbuf,
                            self.voxel if point_size is None else point_size, max_radius=max_radius)
        rgb = self.rgb.contiguous() if color and self.rgb is not None else None
        return ingest.cloud_resolve(zbuf, rgb, dtype=dtype, want_index=want_index)


def rescale_fused_cloud(cloud, s):
    """`SLAMOutput.fused_cloud` of a result that is rescaled by the metric-depth factor `s` the way `FilledReturn.scale`
    does it (disparities / s, translations * s): points * s, voxel * s; colours, counts and keys (voxel indices) stay.
    -> a new `FusedCloud`."""
    out = FusedCloud.__new__(FusedCloud)
    out.xyz, out.voxel = cloud.xyz * s, cloud.voxel * float(s)
    out.rgb, out.count, out.key, out.stats = cloud.rgb, cloud.count, cloud.key, dict(cloud.stats)
    return out


def unpack_depth_conf(conf):
    """`SLAMOutput.frame_depth_conf` (or one map of a `frame_depth_conf_sink`), uint8 -> (agree, visible), two uint8
    tensors of its shape: of the pixel's neighbour keyframes, how many confirm its depth and how many see its point at
    all (agree <= visible <= `SLAMConfig.frame_depth_conf_neighbours`).  visible == 0 says nothing either way."""
    require(conf.dtype == torch.uint8, "depth confidence maps are uint8")
    return conf & 15, conf >> 4


class SLAMOutput:
    """interface.py:143-163: what `SLAMSystem.run` returns - trajectory (camera -> world per frame, SE3 [N]), intrinsics
    [V,4], the rig, the map, the BA residual.

    Not in the reference, None unless `SLAMConfig.upsample_disps`: `keyframe_disps_up` [N_kf,V,H,W] f32, the keyframes'
    disparities at full SLAM resolution (the 1/8 maps through the update operator's learned convex upsampling, DROID-SLAM's
    `disps_up`), and `keyframe_disps_up_valid` [N_kf,V] bool, both aligned with `keyframe_ids`.  H x W is the resolution
    SLAM ran at: for `run(..., native_resolution=True)` the resized and cropped size, not the native one.

    Likewise None unless `SLAMConfig.disp_uncertainty`: `keyframe_disp_var` [N_kf,V,h,w] f32 at the BA's 1/8 grid and
    `keyframe_pose_cov` [N_kf,6,6] f64 (left tangent of the world -> camera keyframe pose, X <- Exp(dx) X, order
    translation, rotation), aligned with `keyframe_ids`: marginal covariances of the last global BA's damped, weighted
    linear system - the network's confidence weights act as inverse variances, without a noise scale, so they rank how
    well pixels and poses are determined rather than give metric error bars.  NaN where not free (the gauge keyframe).

    None unless `SLAMConfig.frame_depth`: `frame_depths` [T,V,H0,W0] (`SLAMConfig.frame_depth_dtype`, fp16 by default),
    one depth map per frame and view of the video - the reciprocal of the frame's full-resolution disparity (a
    keyframe's from the global BA, every other frame's from pass 2), for `run(..., native_resolution=True)` at the
    frames' native size, otherwise at SLAM resolution; 0 where the disparity is not positive; in the trajectory's units
    (`rescale_frame_depths` for a metric factor).  For the panorama camera the disparities are inverse ranges, so the
    maps are ranges.  It stays None when a `SLAMConfig.frame_depth_sink` took the maps instead.  `frame_disps_lowres`
    [T,V,h,w] f32: pass 2's disparities of every frame at the BA's 1/8 grid (`FilledReturn.dense_disps`).

    None unless `SLAMConfig.frame_depth_conf` (and no `frame_depth_conf_sink`): `frame_depth_conf` [T,V,H0,W0] uint8,
    pixel for pixel beside `frame_depths`: the multi-view consistency count against the frame's nearest keyframes of
    the same view, agree | visible << 4 (`unpack_depth_conf`).

    None unless `SLAMConfig.fused_cloud`: `fused_cloud`, a `FusedCloud` - the confident pixels of all those maps in one
    voxel-fused, coloured point cloud of bounded size (`rescale_fused_cloud` for a metric factor,
    `driver.artifacts.write_ply` for a file).

    None unless `SLAMConfig.fused_depth` (and no `fused_depth_sink`): `fused_depths` [T,V,H0,W0]
    (`SLAMConfig.frame_depth_dtype`), pixel for pixel beside `frame_depths`: the fused cloud drawn into every frame's
    camera with the final poses (`FusedCloud.render`), 0 where nothing is drawn, in the trajectory's units
    (`rescale_frame_depths` for a metric factor); with `SLAMConfig.fused_depth_color` `fused_rgb` [T,V,H0,W0,3] uint8, the
    colour of the point each pixel shows.

    None unless `SLAMConfig.complete_depth`: `complete_depths` [T,V,H0,W0] (`SLAMConfig.frame_depth_dtype`; None when a
    `complete_depth_sink` took the maps), `fused_depths` without holes: the fused value where there is one, elsewhere the
    frame's own depth aligned to the nearest fused pixels (`ingest.depth_complete`), 0 where neither can be had
    (`rescale_frame_depths` for a metric factor); and `complete_depth_stats`, the clip's counters of filled pixels:
    a dict of affine, scale_only, unreached, rejected."""

    def __init__(self, *, trajectory, intrinsics, rig=None, slam_map=None, ba_residual=0.0, keyframe_disps_up=None,
                 keyframe_disps_up_valid=None, keyframe_disp_var=None, keyframe_pose_cov=None, frame_depths=None,
                 frame_disps_lowres=None, frame_depth_conf=None, fused_cloud=None, fused_depths=None, fused_rgb=None,
                 complete_depths=None, complete_depth_stats=None):
        self.complete_depths, self.complete_depth_stats = complete_depths, complete_depth_stats
        self.fused_depths, self.fused_rgb = fused_depths, fused_rgb
        self.frame_depths, self.frame_disps_lowres = frame_depths, frame_disps_lowres
        self.frame_depth_conf, self.fused_cloud = frame_depth_conf, fused_cloud
        self.keyframe_disp_var, self.keyframe_pose_cov = keyframe_disp_var, keyframe_pose_cov
        self.trajectory, self.intrinsics, self.rig, self.slam_map, self.ba_residual = trajectory, intrinsics, rig, slam_map, ba_residual
        self.keyframe_disps_up, self.keyframe_disps_up_valid = keyframe_disps_up, keyframe_disps_up_valid

    @property
    def keyframe_ids(self):
        assert self.slam_map is not None, "SLAM map not available."
        return np.array(self.slam_map.dense_disp_frame_inds)

    def get_view_trajectory(self, view_idx):
        assert self.rig is not None, "Rig not available."
        return self.trajectory * self.rig[view_idx][None]

