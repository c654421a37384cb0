"""Result artifacts in the reference's on-disk formats (vipe/utils/io.py:144-225), so that clips processed here can be
compared with / consumed like the reference's outputs.  SURVEY 8(f) row 4.

  pose/<name>.npz        data [F,4,4] float32 OpenCV cam2world matrices, inds [F] frame indices (io.py:144-162)
  intrinsics/<name>.npz  data [F,4|5] float32 [fx,fy,cx,cy(,k1)], inds [F]                       (io.py:181-203)
  intrinsics/<name>_camera.txt   "<frame_idx>: <CAMERA_TYPE>" per line                            (io.py:205-214)
  depth/<name>.zip       one `<frame_idx:05d>.exr` per frame: a single HALF channel `Z` (metric depth), ZIP_DEFLATED
                         archive (io.py:250-277).  The OpenEXR bindings are absent here: the container is written and
                         read by `vipe_amd/driver/exr.py` from the published file layout (parity unpinned)."""
import os
import zipfile

import numpy as np
import torch

from ..ext.lietorch import SE3


def cam2world_matrices(poses_w2c):
    """[F,7] world->camera rows (the SLAM buffer's convention) -> [F,4,4] float32 cam2world"""
    return SE3(torch.as_tensor(poses_w2c, dtype=torch.float32)).inv().matrix().cpu().numpy().astype(np.float32)


def save_pose_artifacts(path, poses_w2c, inds=None):
    data = cam2world_matrices(poses_w2c)
    inds = np.arange(data.shape[0]) if inds is None else np.asarray(inds)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, data=data, inds=inds)


def read_pose_artifacts(path):
    """-> (inds [F], cam2world [F,4,4])"""
    d = np.load(path)
    return d["inds"], d["data"]


def save_intrinsics_artifacts(path, intrinsics, inds=None, camera_type="PINHOLE", camera_path=None):
    data = np.asarray(torch.as_tensor(intrinsics).cpu().numpy(), dtype=np.float32)
    if data.ndim == 1:
        data = data[None]
    inds = np.arange(data.shape[0]) if inds is None else np.asarray(inds)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, data=data, inds=inds)
    if camera_path is not None:
        with open(camera_path, "w") as f:
            for i in inds:
                f.write(f"{int(i)}: {camera_type}\n")


def read_intrinsics_artifacts(path, camera_path=None):
    d = np.load(path)
    inds, data = d["inds"], d["data"]
    if camera_path is None or not os.path.exists(camera_path):
        assert data.shape[1] == 4
        types = ["PINHOLE"] * data.shape[0]
    else:
        types = [line.split(":")[1].strip() for line in open(camera_path)]
    return inds, data, types


def save_depth_artifacts(path, depths, inds=None):
    """io.py:250-277: metric depth maps [F,H,W] (or an iterable of [H,W], None entries skipped) -> zipped EXR files"""
    from .exr import write_exr_half
    items = [(i if inds is None else int(inds[i]), d) for i, d in enumerate(depths) if d is not None]
    if not items:
        return
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for frame_idx, d in items:
            d = d.detach().cpu().numpy() if torch.is_tensor(d) else np.asarray(d)
            z.writestr(f"{frame_idx:05d}.exr", write_exr_half(d))


class DepthZipWriter:
    """`save_depth_artifacts` one map at a time: the archive is opened once and every call writes one
    `<frame_idx:05d>.exr` - usable as `SLAMConfig.frame_depth_sink`, so that a long clip's native-size maps leave the
    device as pass 2's chunks complete (each call copies its map to the host).  One archive holds one view's maps (the
    reference writes one `depth/<name>.zip` per stream): calls for other views than `view_idx` are ignored.  Close it
    (or use it as a context manager) before reading the file.  `SLAMConfig.fused_depth_sink` has the same contract: a
    second writer (another archive) takes the fused cloud's maps as it is, after pass 2."""

    def __init__(self, path, view_idx=0):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self.view_idx, self.count = view_idx, 0
        self._zip = zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED)

    def __call__(self, frame_idx, view_idx, depth):
        from .exr import write_exr_half
        if view_idx != self.view_idx:
            return
        d = depth.detach().cpu().numpy() if torch.is_tensor(depth) else np.asarray(depth)
        self._zip.writestr(f"{int(frame_idx):05d}.exr", write_exr_half(d))
        self.count += 1

    def close(self):
        if self._zip is not None:
            self._zip.close()
            self._zip = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def read_depth_artifacts(path):
    """io.py:279-310 -> iterator of (frame_idx, float32 [H,W] tensor); an unreadable member yields an all-NaN map of the
    last good size, as the reference does"""
    from .exr import read_exr_half
    shape = None
    with zipfile.ZipFile(path, "r") as z:
        for name in sorted(z.namelist()):
            frame_idx = int(name.split(".")[0])
            try:
                d = read_exr_half(z.read(name))
            except (OSError, KeyError, ValueError, zipfile.BadZipFile):
                assert shape is not None
                yield frame_idx, torch.full(shape, float("nan"), dtype=torch.float32)
                continue
            shape = d.shape
            yield frame_idx, torch.from_numpy(d.astype(np.float32))


def write_ply(path, cloud):
    """`SLAMOutput.fused_cloud` (an `interface.FusedCloud`) -> a binary little-endian PLY file: per vertex x, y, z as
    float, red, green, blue as uchar when the cloud carries colour, and the voxel's hit count as the int property
    `count`.  Host code: the tensors are brought over once.  -> number of vertices written"""
    xyz = cloud.xyz.detach().cpu().numpy().astype("<f4", copy=False)
    count = cloud.count.detach().cpu().numpy().astype("<i4", copy=False)
    rgb = None if cloud.rgb is None else cloud.rgb.detach().cpu().numpy().astype(np.uint8, copy=False)
    m = xyz.shape[0]
    assert xyz.shape == (m, 3) and count.shape == (m,) and (rgb is None or rgb.shape == (m, 3))
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if rgb is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    fields.append(("count", "<i4"))
    props.append("property int count")
    v = np.empty(m, dtype=np.dtype(fields))  # packed: 16 bytes per vertex, 19 with colour
    v["x"], v["y"], v["z"], v["count"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], count
    if rgb is not None:
        v["red"], v["green"], v["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    header = "\n".join(["ply", "format binary_little_endian 1.0", f"comment fused cloud, voxel {cloud.voxel:.9g}",
                        f"element vertex {m}"] + props + ["end_header"]) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(v.tobytes())
    return m


def save_clip_results(out_dir, results, name_of=lambda r: f"clip_{r.clip_id:05d}"):
    """Rank 0 after `clip_shard.gather_results`: one pose + intrinsics artifact per successful clip."""
    written = []
    for r in results:
        if not r.ok or r.poses.shape[0] == 0:
            continue
        name = name_of(r)
        save_pose_artifacts(os.path.join(out_dir, "pose", name + ".npz"), r.poses)
        save_intrinsics_artifacts(os.path.join(out_dir, "intrinsics", name + ".npz"),
                                  r.intrinsics[None].expand(r.poses.shape[0], -1),
                                  camera_path=os.path.join(out_dir, "intrinsics", name + "_camera.txt"))
        written.append(name)
    return written
