"""The fused point cloud end to end: `SLAMConfig.fused_cloud` -> one `cloud_fuse` launch per pass-2 chunk, directly behind
the consistency launch, on its rows and its bytes -> one `cloud_extract` per clip -> `SLAMOutput.fused_cloud`.  The clips
are those of tests/test_gpu_frame_depth.py / test_gpu_frame_depth_conf.py.

`ingest.cloud_fuse` and `ingest.cloud_extract` are the single routes to the kernels, so the tests wrap them: every call's
inputs are copied as the kernel saw them, and the clip's table is compared with the float64 reference of exactly those
inputs under the criterion of tests/cloud_fuse_reference.py.  Two RUNS are not compared bit for bit: the dense BA
accumulates with float atomics (tests/test_gpu_frame_depth_conf.py)."""
import numpy as np
import pytest
import torch

import cloud_fuse_reference as cf
import test_gpu_frame_depth as fd

pytestmark = pytest.mark.gpu


class CloudRecorder:
    def __init__(self):
        from vipe_amd.slam import ingest
        self.mod = ingest
        self.real = dict(fuse=ingest.cloud_fuse, extract=ingest.cloud_extract, conf=ingest.depth_consistency)
        self.calls, self.order, self.extracts, self.last_conf, self.sysm = [], [], [], None, None

    def __enter__(self):
        rec = self

        def conf(disp, poses, rig, intrinsics, camera, resize_or_params, rows, nbr, tol, out=None):
            res = rec.real["conf"](disp, poses, rig, intrinsics, camera, resize_or_params, rows, nbr, tol, out=out)
            rec.last_conf = (res, rows)
            rec.order.append("conf")
            return res

        def fuse(disp, poses, rig, intrinsics, camera, resize_or_params, rows, table, voxel, conf=None, min_agree=0, rgb=None,
                 stride=1):
            s = rec.sysm
            state = lambda: [x.clone() for x in (disp, poses, s.buffer.disps_up_valid, conf)
                             + tuple(x.view(torch.uint8) for x in (s.frame_depths, s.frame_depth_conf) if x is not None)]
            before = state()
            res = rec.real["fuse"](disp, poses, rig, intrinsics, camera, resize_or_params, rows, table, voxel, conf=conf,
                                   min_agree=min_agree, rgb=rgb, stride=stride)
            torch.cuda.synchronize()
            rec.calls.append(dict(disp=before[0], poses=before[1], rig=rig.clone(), intrinsics=intrinsics.clone(), camera=camera,
                                  params=rec.mod.export_params(resize_or_params, *disp.shape[1:]), rows=rows.cpu().numpy(),
                                  voxel=voxel, conf=before[3].cpu().numpy(), min_agree=min_agree, stride=stride,
                                  rgb=None if rgb is None else rgb.cpu().numpy(), table_ptr=table[0].data_ptr(),
                                  unchanged=all(torch.equal(a, b) for a, b in zip(before, state())),
                                  same_inputs=rec.last_conf is not None and conf is rec.last_conf[0] and rows is rec.last_conf[1],
                                  disp_ptr=disp.data_ptr()))
            rec.order.append("fuse")
            return res

        def extract(table, voxel, **kw):
            res = rec.real["extract"](table, voxel, **kw)
            rec.extracts.append(dict(table=tuple(x.cpu().numpy() for x in table), voxel=voxel, kw=kw, table_ptr=table[0].data_ptr()))
            rec.order.append("extract")
            return res

        self.mod.cloud_fuse, self.mod.cloud_extract, self.mod.depth_consistency = fuse, extract, conf
        return self

    def __exit__(self, *exc):
        self.mod.cloud_fuse, self.mod.cloud_extract, self.mod.depth_consistency = self.real["fuse"], self.real["extract"], self.real["conf"]


def run_clip(frames, rig=None, **cfg_kw):
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    native = cfg_kw.pop("native_resolution", False)
    torch.manual_seed(0)
    cfg = SLAMConfig(buffer=40, filter_thresh=0.0, frontend_backend_iters=(), frontend=FrontendArgs(keyframe_thresh=0.0),
                     infill=InfillArgs(infill_chunk_size=4), frame_depth=True, frame_depth_conf=True,
                     fused_cloud_capacity=1 << 21, fused_cloud_voxel=0.05, **cfg_kw)
    sysm = SLAMSystem(fd.dev(), cfg, motion_filter_cls=fd.scripted_filter(4))
    with CloudRecorder() as rec:
        rec.sysm = sysm
        out = sysm.run(frames, rig=rig, native_resolution=native)
        torch.cuda.synchronize()
    return dict(out=out, sysm=sysm, rec=rec, cfg=cfg, frames=frames)


@pytest.fixture(scope="module")
def off_run():
    return run_clip(fd.one_view_frames())


@pytest.fixture(scope="module")
def on_run():
    return run_clip(fd.one_view_frames(), fused_cloud=True, fused_cloud_min_agree=0, fused_cloud_min_count=1)


@pytest.fixture(scope="module")
def native_run():
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(6)
    T, H, W = 9, 160, 600
    rgb = (255 * torch.rand(T, H, W, 3, generator=gen)).to(torch.uint8).to(fd.dev())  # decoded frames: bytes
    depth = (1.0 + 4.0 * torch.rand(T, H, W, generator=gen)).to(fd.dev())
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    frames = [Frame(rgb=rgb[t], metric_depth=depth[t], intrinsics=intr) for t in range(T)]
    return run_clip(frames, fused_cloud=True, fused_cloud_min_agree=1, fused_cloud_stride=2, native_resolution=True)


@pytest.fixture(scope="module")
def rig_run():
    frames, rig = fd.two_view_frames()
    return run_clip(frames, rig=rig, fused_cloud=True, fused_cloud_min_agree=0, frame_depth_conf_neighbours=2)


@pytest.fixture(scope="module")
def sink_run():
    sunk = []
    return run_clip(fd.one_view_frames(), fused_cloud=True, fused_cloud_min_agree=0, fused_cloud_color=False,
                    frame_depth_sink=lambda f, v, d: sunk.append(f), frame_depth_conf_sink=lambda f, v, c: sunk.append(f))


def check_run(run, T, what, min_kept=1000):
    """every launch of a run and the cloud it returns -> the expected table"""
    out, rec, sysm, cfg = run["out"], run["rec"], run["sysm"], run["cfg"]
    b = sysm.buffer
    V = b.n_views
    chunks = [list(range(c0, min(c0 + 4, T))) for c0 in range(0, T, 4)]
    assert rec.order == ["conf", "fuse"] * len(chunks) + ["extract"], f"{what}: one fuse per chunk behind its consistency launch, one extract"
    refs = []
    for call, frames in zip(rec.calls, chunks):
        assert call["same_inputs"], f"{what}: the rows and the bytes of the consistency launch, as objects"
        assert call["unchanged"], f"{what}: the launch only reads (buffer, poses, flags, depths, confidences)"
        assert call["disp_ptr"] == b.flattened_disps_up.data_ptr() and call["table_ptr"] == rec.extracts[0]["table_ptr"]
        assert (call["voxel"], call["min_agree"], call["stride"]) == (cfg.fused_cloud_voxel, cfg.fused_cloud_min_agree, cfg.fused_cloud_stride)
        assert call["conf"].shape[0] == len(frames) * V == call["rows"].shape[0]
        if cfg.fused_cloud_color:
            want = torch.stack([fr.rgb for f in frames for fr in (run["frames"][f] if V > 1 else [run["frames"][f]])])
            assert np.array_equal(call["rgb"], want.cpu().numpy()), f"{what}: the chunk's frames as they were handed in"
        else:
            assert call["rgb"] is None
        slots = sorted({int(r) // V for r in call["rows"]})  # the reference gets only the slots that are named
        rows_of = [s * V + v for s in slots for v in range(V)]
        pos = {r: i for i, r in enumerate(rows_of)}
        refs.append(cf.cloud_fuse_ref(call["disp"][rows_of].cpu().numpy(), call["poses"][slots].cpu().numpy(),
                                      call["rig"].cpu().numpy(), call["intrinsics"].cpu().numpy(), call["camera"], call["params"],
                                      np.array([pos[int(r)] for r in call["rows"]]), call["voxel"], conf=call["conf"],
                                      min_agree=call["min_agree"], rgb=call["rgb"], stride=call["stride"]))
    ref = {k: np.concatenate([r[k] for r in refs]) for k in refs[0] if k != "inv_voxel"}
    exp = cf.expected_table(ref)
    ex = rec.extracts[0]
    firm, loose = cf.compare_table(*ex["table"], exp)
    stats = [int(v) for v in ex["table"][2]]
    print(f"{what}: kept {exp['n_kept']}, undecided {exp['n_undecided']}; {firm} voxels exact, {loose} within bounds; counters {stats}; "
          f"table load {(ex['table'][0] != -1).mean():.3f}")
    assert exp["n_kept"] > min_kept and firm > 0 and stats[1] == 0 and stats[3] == 0
    # the cloud is the extraction of that table
    assert ex["voxel"] == cfg.fused_cloud_voxel and ex["kw"] == dict(min_count=cfg.fused_cloud_min_count, color=cfg.fused_cloud_color)
    keys, sums, _ = cf.table_rows(*ex["table"][:2])
    xyz, rgb, count, key = cf.extract_ref(keys, sums, cfg.fused_cloud_voxel, cfg.fused_cloud_min_count)
    cloud = out.fused_cloud
    assert np.array_equal(cloud.key.cpu().numpy(), key) and np.array_equal(cloud.count.cpu().numpy(), count)
    assert np.array_equal(cloud.xyz.cpu().numpy(), xyz) and cloud.voxel == cfg.fused_cloud_voxel
    assert cloud.stats == dict(zip(cf.STATS, stats)) and len(cloud) > 0 and cloud.xyz.is_cuda
    if cfg.fused_cloud_color:
        assert np.array_equal(cloud.rgb.cpu().numpy(), rgb)
    else:
        assert cloud.rgb is None
    assert sysm._cloud is None, "the table is released with the run"
    return exp


def test_off_nothing_is_called_or_returned(off_run):
    out, rec = off_run["out"], off_run["rec"]
    assert out.fused_cloud is None and out.frame_depth_conf is not None
    assert rec.order == ["conf"] * 4 and not rec.calls and not rec.extracts
    assert off_run["sysm"]._cloud is None


def test_on_every_launch_and_the_cloud(on_run, off_run):
    exp = check_run(on_run, 13, "one view")
    out = on_run["out"]
    assert exp["n_kept"] > 13 * 128 * 512 * 0.5, "the gate is open: every pixel with a positive disparity"
    assert out.keyframe_ids.tolist() == off_run["out"].keyframe_ids.tolist()
    assert out.frame_depths.shape == off_run["out"].frame_depths.shape and out.frame_depth_conf is not None


def test_native_resolution_gate_stride_and_byte_frames(native_run):
    from vipe_amd.slam.ingest import StandardResize, export_params
    r = StandardResize(160, 600)
    assert all(c["params"] == export_params(r, *r.out_size) and c["rgb"].dtype == np.uint8 and c["rgb"].shape[1:] == (160, 600, 3)
               for c in native_run["rec"].calls)
    check_run(native_run, 9, "native resolution", min_kept=0)  # random frames: few pixels find agreement


def test_two_view_rig(rig_run):
    assert rig_run["sysm"].buffer.n_views == 2
    check_run(rig_run, 10, "two views")


def test_sinks_and_no_colour(sink_run):
    out = sink_run["out"]
    assert out.frame_depths is None and out.frame_depth_conf is None
    check_run(sink_run, 13, "sinks")
