"""Per-frame depth confidence end to end: `SLAMConfig.frame_depth_conf` -> one `depth_consistency` launch per pass-2 chunk,
right after the depth export and on its rows -> `SLAMOutput.frame_depth_conf` (or the sink).  The clips are those of
tests/test_gpu_frame_depth.py (13 frames, every 4th a keyframe, chunks of 4; a native-resolution clip; a two-view rig).

`ingest.depth_consistency` is the single route to the kernel, so the tests wrap it: every call's inputs are copied as
the kernel saw them (the buffer's rows, poses and flags at that moment), and the output is compared with the float64
reference of exactly those inputs under the criterion of tests/depth_consistency_reference.py."""
import numpy as np
import pytest
import torch

import depth_consistency_reference as cr
import test_gpu_frame_depth as fd

pytestmark = pytest.mark.gpu


class ConfRecorder:
    def __init__(self):
        from vipe_amd.slam import ingest
        self.mod, self.real, self.real_export = ingest, ingest.depth_consistency, ingest.depth_export
        self.calls, self.order, self.exported, self.sysm = [], [], [], None

    def __enter__(self):
        rec = self

        def consistency(disp, poses, rig, intrinsics, camera, resize_or_params, rows, nbr, tol, out=None):
            b = rec.sysm.buffer
            fdp = rec.sysm.frame_depths  # torch.empty behind the chunks exported so far: compared as bytes
            before = (disp.clone(), poses.clone(), b.disps_up_valid.clone(), None if fdp is None else fdp.view(torch.uint8).clone())
            res = rec.real(disp, poses, rig, intrinsics, camera, resize_or_params, rows, nbr, tol, out=out)
            torch.cuda.synchronize()
            unchanged = (torch.equal(before[0], disp) and torch.equal(before[1], poses) and torch.equal(before[2], b.disps_up_valid)
                         and (fdp is None or torch.equal(before[3], fdp.view(torch.uint8))))
            rec.calls.append(dict(disp=before[0], poses=before[1], valid=before[2], rig=rig.clone(), intrinsics=intrinsics.clone(),
                                  camera=camera, params=rec.mod.export_params(resize_or_params, *disp.shape[1:]),
                                  rows=rows.cpu().numpy(), nbr=nbr.cpu().numpy(), tol=tol, out=res.clone(), unchanged=unchanged,
                                  disp_ptr=disp.data_ptr(), n_frames=b.n_frames, given_out=out is not None))
            rec.order.append("conf")
            return res

        def export(*a, **kw):
            rec.order.append(("export", kw["rows"].cpu().tolist()))
            res = rec.real_export(*a, **kw)
            rec.exported.append(res.clone())
            return res

        self.mod.depth_consistency, self.mod.depth_export = consistency, export
        return self

    def __exit__(self, *exc):
        self.mod.depth_consistency, self.mod.depth_export = self.real, self.real_export


def run_clip(frames, rig=None, **cfg_kw):
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    native = cfg_kw.pop("native_resolution", False)
    torch.manual_seed(0)
    cfg = SLAMConfig(buffer=40, filter_thresh=0.0, frontend_backend_iters=(), frontend=FrontendArgs(keyframe_thresh=0.0),
                     infill=InfillArgs(infill_chunk_size=4), frame_depth=True, **cfg_kw)
    sysm = SLAMSystem(fd.dev(), cfg, motion_filter_cls=fd.scripted_filter(4))
    with ConfRecorder() as rec:
        rec.sysm = sysm
        out = sysm.run(frames, rig=rig, native_resolution=native)
        torch.cuda.synchronize()
    return dict(out=out, sysm=sysm, rec=rec, cfg=cfg)


@pytest.fixture(scope="module")
def off_run():
    return run_clip(fd.one_view_frames())


@pytest.fixture(scope="module")
def on_run():
    return run_clip(fd.one_view_frames(), frame_depth_conf=True)


@pytest.fixture(scope="module")
def native_run():
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(6)
    T, H, W = 9, 160, 600
    rgb = torch.rand(T, H, W, 3, generator=gen).to(fd.dev())
    depth = (1.0 + 4.0 * torch.rand(T, H, W, generator=gen)).to(fd.dev())
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    frames = [Frame(rgb=rgb[t], metric_depth=depth[t], intrinsics=intr) for t in range(T)]
    return run_clip(frames, frame_depth_conf=True, native_resolution=True)


@pytest.fixture(scope="module")
def rig_run():
    frames, rig = fd.two_view_frames()
    return run_clip(frames, rig=rig, frame_depth_conf=True, frame_depth_conf_neighbours=2)


@pytest.fixture(scope="module")
def sink_run():
    calls = []
    run = run_clip(fd.one_view_frames(), frame_depth_conf=True,
                   frame_depth_conf_sink=lambda f, v, conf: calls.append((f, v, conf.clone())))
    run["calls"] = calls
    return run


def check_calls(run, T, K, what):
    """every launch of a run: one per chunk, directly behind the chunk's export and on its rows; the neighbour lists; the
    state it read; its output against the reference of the recorded inputs -> the concatenated outputs [T*V,H0,W0]"""
    from vipe_amd.slam.ingest import nearest_keyframes
    out, rec, sysm = run["out"], run["rec"], run["sysm"]
    b = sysm.buffer
    V, kf = b.n_views, out.keyframe_ids.tolist()
    n_kf = len(kf)
    chunks = [list(range(c0, min(c0 + 4, T))) for c0 in range(0, T, 4)]
    assert len(rec.calls) == len(chunks), f"{what}: one launch per chunk"
    assert [o if o == "conf" else "export" for o in rec.order] == ["export", "conf"] * len(chunks)
    exports = [o[1] for o in rec.order if o != "conf"]
    kf_up = out.keyframe_disps_up.reshape(n_kf * V, *out.keyframe_disps_up.shape[2:])
    outs = []
    for ci, (call, frames, exp_rows) in enumerate(zip(rec.calls, chunks, exports)):
        n = len(frames)
        assert call["rows"].tolist() == exp_rows, f"{what}: the rows of the export"
        assert call["disp_ptr"] == b.flattened_disps_up.data_ptr() and call["n_frames"] == n_kf
        assert call["unchanged"], f"{what}: the launch only reads"
        assert call["tol"] == run["cfg"].frame_depth_conf_tol and call["nbr"].shape == (n * V, K)
        slots = nearest_keyframes(frames, kf, [True] * n_kf, K).numpy()
        want = np.stack([np.where(slots >= 0, slots * V + v, -1) for v in range(V)], axis=1).reshape(n * V, K)
        assert np.array_equal(call["nbr"], want), f"{what}: nbr = nearest_keyframes of the chunk's timestamps, same view"
        for j, f in enumerate(frames):
            for v in range(V):
                if f in kf:  # its map is the keyframe's row: that row is no neighbour of it
                    assert call["rows"][j * V + v] == kf.index(f) * V + v and kf.index(f) * V + v not in call["nbr"][j * V + v]
        # what the kernel read: the keyframes' final rows, the chunk's rows while their flags were still set, the
        # chunk's own poses (not the previous chunk's)
        assert torch.equal(call["disp"][:n_kf * V], kf_up), f"{what}: keyframe rows"
        assert bool(call["valid"][n_kf:n_kf + n].all()) and bool(call["valid"][:n_kf].all()), f"{what}: before the flags are cleared"
        filled = sysm.inner_filler.filled_poses[ci].data
        assert torch.equal(call["poses"][n_kf:n_kf + n], filled), f"{what}: the chunk's poses"
        if ci > 0:
            assert not torch.equal(call["poses"][n_kf:n_kf + n], rec.calls[ci - 1]["poses"][n_kf:n_kf + n])
        # the reference gets only the slots that are named
        used = sorted(set(call["rows"].tolist()) | set(call["nbr"][call["nbr"] >= 0].tolist()))
        slots_used = sorted({r // V for r in used})
        rows_of = [s * V + v for s in slots_used for v in range(V)]
        pos = {r: i for i, r in enumerate(rows_of)}
        ref = cr.depth_consistency_ref(call["disp"][rows_of].cpu().numpy(), call["poses"][slots_used].cpu().numpy(),
                                       call["rig"].cpu().numpy(), call["intrinsics"].cpu().numpy(), call["camera"], call["params"],
                                       np.array([pos[r] for r in call["rows"]]),
                                       np.array([[pos[q] if q >= 0 else -1 for q in row] for row in call["nbr"].tolist()]),
                                       call["tol"])
        got = call["out"].cpu().numpy()
        exact, loose = cr.compare(got, ref)
        s = cr.summary(ref)
        print(f"{what} chunk {ci}: {exact} pixels exact, {loose} with undecided pairs; pairs {s}")
        assert ref["written"].all() and exact > 0
        outs.append(call["out"])
    return torch.cat(outs)


def test_off_nothing_is_called_or_returned(off_run):
    out, sysm, rec = off_run["out"], off_run["sysm"], off_run["rec"]
    assert out.frame_depth_conf is None and out.frame_depths is not None
    assert len(rec.calls) == 0 and sum(o != "conf" for o in rec.order) == 4
    assert sysm.frame_depth_conf is None and sysm._kf_times is None


def test_on_every_launch_and_the_output(on_run):
    out = on_run["out"]
    conf = out.frame_depth_conf
    assert tuple(conf.shape) == (13, 1, 128, 512) and conf.dtype == torch.uint8 and out.frame_depths.shape == conf.shape
    got = check_calls(on_run, 13, 4, "one view")
    assert torch.equal(got.view(13, 1, 128, 512), conf)
    assert all(c["given_out"] for c in on_run["rec"].calls), "written in place: no copy per chunk"
    from vipe_amd.slam.interface import unpack_depth_conf
    agree, visible = unpack_depth_conf(conf)
    assert bool((agree <= visible).all()) and int(visible.max()) <= 4
    kf = out.keyframe_ids.tolist()
    assert 0 in kf and 12 in kf and 3 <= len(kf) <= 6, "both kinds of frame are needed"
    assert int(visible[1].max()) > 0, "a frame between keyframes is seen by some of them"


def test_flag_only_reads(off_run, on_run):
    """The launch changes nothing that `run` returns or that pass 2 goes on to use.  Within the run with the flag: across
    every launch the whole `disps_up` buffer, the poses, the rows' flags and `frame_depths` are bitwise what they were
    (`unchanged`, asserted per launch in `check_calls`), and what `run` returns is what was there before the launches -
    `frame_depths` the export's outputs, the trajectory the chunks' poses, the keyframe rows those of the start of
    pass 2.  Against the run without the flag: the same keyframes and the same launches otherwise.
    Depths and trajectory of two RUNS are not compared bit for bit: the dense BA accumulates with float atomics, so two
    runs of one configuration differ in the last digits (tests/test_gpu_frame_depth.py compares decisions only, for the
    same reason).  Measured on the MI355X on this clip: largest trajectory difference 6.3e-5 and 1.5e-5 between the run
    with the flag and two runs without it, 4.9e-5 between those two; 1.2-1.5 % of the fp16 depths differ by one ulp in
    every one of the three comparisons."""
    from vipe_amd.ext import lietorch as lt
    a, b, rec = off_run["out"], on_run["out"], on_run["rec"]
    assert a.keyframe_ids.tolist() == b.keyframe_ids.tolist()
    assert [o for o in off_run["rec"].order] == [o for o in rec.order if o != "conf"], "the same exports, in the same order"
    assert all(c["unchanged"] for c in rec.calls) and len(rec.calls) == 4
    assert torch.equal(torch.cat(rec.exported).view(b.frame_depths.shape), b.frame_depths)
    assert torch.equal(lt.cat(on_run["sysm"].inner_filler.filled_poses, dim=0).inv().data, b.trajectory.data)
    n_kf = len(b.keyframe_ids)
    assert all(torch.equal(c["disp"][:n_kf].view(b.keyframe_disps_up.shape), b.keyframe_disps_up) for c in rec.calls)
    assert a.frame_depths.shape == b.frame_depths.shape and a.frame_depths.dtype == b.frame_depths.dtype


def test_native_resolution(native_run):
    from vipe_amd.slam.ingest import StandardResize, export_params
    out = native_run["out"]
    r = StandardResize(160, 600)
    assert tuple(out.frame_depth_conf.shape) == (9, 1, 160, 600) == tuple(out.frame_depths.shape)
    assert all(c["params"] == export_params(r, *r.out_size) for c in native_run["rec"].calls)
    got = check_calls(native_run, 9, 4, "native resolution")
    assert torch.equal(got.view(9, 1, 160, 600), out.frame_depth_conf)


def test_two_view_rig(rig_run):
    out = rig_run["out"]
    assert rig_run["sysm"].buffer.n_views == 2 and tuple(out.frame_depth_conf.shape) == (10, 2, 128, 512)
    got = check_calls(rig_run, 10, 2, "two views")  # rows and neighbours are slot * V + view
    assert torch.equal(got.view(10, 2, 128, 512), out.frame_depth_conf)


def test_sink(sink_run, on_run):
    """the sink receives, in frame order, exactly the maps the launches wrote (the tensor run's maps are those of its own
    launches, `test_on_every_launch_and_the_output`; two runs are not compared bit for bit, `test_flag_only_reads`)"""
    out, calls = sink_run["out"], sink_run["calls"]
    assert out.frame_depth_conf is None and out.frame_depths is not None
    assert [(f, v) for f, v, _ in calls] == [(f, 0) for f in range(13)]
    assert all(tuple(c.shape) == (128, 512) and c.dtype == torch.uint8 and c.is_cuda for _, _, c in calls)
    got = check_calls(sink_run, 13, 4, "sink")
    assert torch.equal(got, torch.stack([c for _, _, c in calls]))
    assert not any(c["given_out"] for c in sink_run["rec"].calls)
    assert out.keyframe_ids.tolist() == on_run["out"].keyframe_ids.tolist()
    assert [c["nbr"].tolist() for c in sink_run["rec"].calls] == [c["nbr"].tolist() for c in on_run["rec"].calls]
