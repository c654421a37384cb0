"""Per-frame depth end to end: `SLAMConfig.frame_depth` -> pass 2 with dense disparities, upsampled in the last of its ten
updates for the chunk's own rows only -> one `depth_export` launch per chunk -> `SLAMOutput.frame_depths` (or the sink).
Short random clips with random-init weights (seed 0), every 4th frame a keyframe (a scripted motion filter), pass 2 in
chunks of 4 frames, so that there are several chunks and both kinds of frame: keyframes, whose depth comes from the
keyframe's `disps_up` row (the global BA's result), and the others, whose depth comes from their pass-2 row.

`ingest.depth_export` and `droid_net_ext.cvx_upsample` are the single routes to their kernels, so the tests wrap them, and
they wrap `InnerFiller.compute` to snapshot the chunk's final 1/8 disparities.  Values of two runs are never compared
(the BA's atomics are order dependent); keyframe decisions are."""
import numpy as np
import pytest
import torch

import cvx_reference as cr
import depth_export_reference as dr

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def scripted_filter(keep_every):
    """every `keep_every`-th frame becomes a keyframe (bench.scripted_filter: the score of a random-weight flow network has
    no meaningful scale); all of the filter's work still runs"""
    from vipe_amd.slam.motion_filter import MotionFilter

    class ScriptedMotionFilter(MotionFilter):
        def finish(self, h):
            if self.initialized:
                self.thresh = -1.0 if (self.current_frame_idx + 1) % keep_every == 0 else float("inf")
            return super().finish(h)

    return ScriptedMotionFilter


def one_view_frames(T=13, H=128, W=512):
    from vipe_amd.ext.lietorch import SE3
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(5)
    rgb = torch.rand(T, H, W, 3, generator=gen).to(dev())
    depth = (1.0 + 4.0 * torch.rand(T, H, W, generator=gen)).to(dev())
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    out = []
    for t in range(T):
        pose = SE3(torch.tensor([[-0.05 * t, 0, 0, 0, 0, 0, 1.0]], device=dev())).inv()  # camera -> world
        out.append(Frame(rgb=rgb[t], metric_depth=depth[t], intrinsics=intr, pose=SE3(pose.data[0]),
                         mask=torch.ones(H, W, dtype=torch.bool, device=dev())))
    return out


def two_view_frames(T=10, V=2, H=128, W=512):
    from vipe_amd.ext.lietorch import SE3
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(8)
    rgb = torch.rand(T, V, H, W, 3, generator=gen).to(dev())
    depth = (1.0 + 4.0 * torch.rand(T, V, H, W, generator=gen)).to(dev())
    intr = torch.tensor([460.8, 460.8, 256.0, 64.0])
    rig = SE3(torch.tensor([[0, 0, 0, 0, 0, 0, 1.0], [0.3, 0.0, 0.0, 0.0, 0.05, 0.0, 0.99875]], device=dev()))
    frames = [[Frame(rgb=rgb[t, v], metric_depth=depth[t, v], intrinsics=intr * (1.0 + 0.02 * v)) for v in range(V)]
              for t in range(T)]
    return frames, rig


class Recorder:
    """wraps cvx_upsample (per flattened buffer row the mask row it was LAST upsampled with, the calls in order),
    depth_export (rows, a copy of the input rows it names, parameters, a copy of what it wrote) and
    InnerFiller.compute (before the first: the keyframes' disps_up; after each: the chunk's disps, the last mask of each
    of its rows, the upsampling calls it made, the graph's flags)"""

    def __init__(self):
        from vipe_amd.ext import droid_net_ext
        from vipe_amd.slam import ingest, inner_filler
        self.cvx_mod, self.cvx_real = droid_net_ext, droid_net_ext.cvx_upsample
        self.ing_mod, self.exp_real = ingest, ingest.depth_export
        self.filler_cls, self.compute_real = inner_filler.InnerFiller, inner_filler.InnerFiller.compute
        self.cvx_calls, self.last, self.exports, self.chunks = [], {}, [], []
        self.kf_up_before_pass2 = None

    def __enter__(self):
        rec = self

        def cvx(data, mask, rows=None, out=None, **kw):
            res = rec.cvx_real(data, mask, rows=rows, out=out, **kw)
            keep = mask.clone()
            idx = list(range(mask.shape[0])) if rows is None else rows.cpu().tolist()
            rec.cvx_calls.append(idx)
            for s, r in enumerate(idx):
                rec.last[int(r)] = (keep, s)
            return res

        def export(disp, resize_or_params, rows=None, out=None, **kw):
            idx = rows.cpu().tolist()
            inp = disp[rows].clone()
            res = rec.exp_real(disp, resize_or_params, rows=rows, out=out, **kw)
            rec.exports.append(dict(rows=idx, inp=inp, out=res.clone(), disp_ptr=disp.data_ptr(), kw=kw,
                                    params=rec.ing_mod.export_params(resize_or_params, *disp.shape[1:])))
            return res

        def compute(filler):
            v, s = filler.video, filler.start_idx
            total, V = v.n_frames, v.n_views
            if rec.kf_up_before_pass2 is None and v.disps_up is not None:
                rec.kf_up_before_pass2 = v.disps_up[:s].clone()
            n0 = len(rec.cvx_calls)
            rec.compute_real(filler)
            g = filler.last_graph
            rec.chunks.append(dict(s=s, n=total - s, disps=v.disps[s:total].clone(), cvx_calls=rec.cvx_calls[n0:],
                                   masks={r: rec.last.get(r) for r in range(s * V, total * V)},
                                   upsample=g.upsample, from_row=g.upsample_from_row,
                                   up_rows=v.flattened_disps_up[s * V:total * V].clone() if v.disps_up is not None else None))

        self.cvx_mod.cvx_upsample, self.ing_mod.depth_export, self.filler_cls.compute = cvx, export, compute
        return self

    def __exit__(self, *exc):
        self.cvx_mod.cvx_upsample, self.ing_mod.depth_export, self.filler_cls.compute = self.cvx_real, self.exp_real, self.compute_real


def run_clip(frames, rig=None, keep_every=4, **cfg_kw):
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.motion_filter import MotionFilter
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    native = cfg_kw.pop("native_resolution", False)
    torch.manual_seed(0)
    cfg = SLAMConfig(buffer=40, filter_thresh=0.0, frontend_backend_iters=(), frontend=FrontendArgs(keyframe_thresh=0.0),
                     infill=InfillArgs(infill_chunk_size=4), **cfg_kw)
    sysm = SLAMSystem(dev(), cfg, motion_filter_cls=scripted_filter(keep_every) if keep_every > 1 else MotionFilter)
    with Recorder() as rec:
        out = sysm.run(frames, rig=rig, native_resolution=native)
        torch.cuda.synchronize()
    return dict(out=out, sysm=sysm, rec=rec, cfg=cfg)


@pytest.fixture(scope="module")
def off_run():
    return run_clip(one_view_frames())


@pytest.fixture(scope="module")
def on_run():
    return run_clip(one_view_frames(), frame_depth=True)


@pytest.fixture(scope="module")
def up_only_run():
    return run_clip(one_view_frames(), upsample_disps=True)


@pytest.fixture(scope="module")
def native_run():
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(6)
    T, H, W = 9, 160, 600
    rgb = torch.rand(T, H, W, 3, generator=gen).to(dev())
    depth = (1.0 + 4.0 * torch.rand(T, H, W, generator=gen)).to(dev())
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    frames = [Frame(rgb=rgb[t], metric_depth=depth[t], intrinsics=intr) for t in range(T)]
    return run_clip(frames, frame_depth=True, native_resolution=True)


@pytest.fixture(scope="module")
def rig_run():
    frames, rig = two_view_frames()
    return run_clip(frames, rig=rig, frame_depth=True, frame_depth_dtype=torch.float32)  # the f32 store, too


@pytest.fixture(scope="module")
def sink_run(tmp_path_factory):
    from vipe_amd.driver.artifacts import DepthZipWriter
    path = str(tmp_path_factory.mktemp("depth") / "clip.zip")
    calls = []
    with DepthZipWriter(path) as writer:
        def sink(frame_idx, view_idx, depth):
            calls.append((frame_idx, view_idx, depth.clone()))
            writer(frame_idx, view_idx, depth)
        run = run_clip(one_view_frames(), frame_depth=True, frame_depth_sink=sink)
    run.update(calls=calls, path=path, written=writer.count)
    return run


def expected_rows(run, T):
    """per chunk of 4 frames: the keyframe's row for a frame that is a keyframe, the pass-2 row (slot n_kf + j) otherwise"""
    kf = run["out"].keyframe_ids.tolist()
    V, s = run["sysm"].buffer.n_views, len(kf)
    return [[(kf.index(f) if f in kf else s + j) * V + v for j, f in enumerate(range(c0, min(c0 + 4, T))) for v in range(V)]
            for c0 in range(0, T, 4)]


def check_exports(run, T, what):
    """every export call: the rows, the non-keyframe inputs against the convex-upsampling reference of the chunk's final
    disparities under the last mask of each row, the keyframe inputs against `keyframe_disps_up`, the outputs against the
    depth-export reference of the recorded inputs -> the concatenated outputs [T*V,H0,W0]"""
    out, rec, b = run["out"], run["rec"], run["sysm"].buffer
    V, n_kf = b.n_views, len(out.keyframe_ids)
    want_rows = expected_rows(run, T)
    assert [e["rows"] for e in rec.exports] == want_rows, f"{what}: export rows"
    assert len(rec.chunks) == len(want_rows)
    kf_up = out.keyframe_disps_up.reshape(n_kf * V, *out.keyframe_disps_up.shape[2:])
    worst_cvx = worst_exp = 0.0
    outs = []
    for e, ch in zip(rec.exports, rec.chunks):
        assert e["disp_ptr"] == b.flattened_disps_up.data_ptr(), "the export reads the buffer's rows in place: no gathers"
        # the chunk's graph upsampled once, in its last update, and only its own rows
        assert ch["upsample"] and ch["from_row"] == ch["s"] * V and ch["s"] == n_kf
        assert len(ch["cvx_calls"]) == 1, "only the last of the ten updates upsamples"
        named = [r for r in ch["cvx_calls"][0] if r >= 0]
        assert sorted(named) == list(range(n_kf * V, (n_kf + ch["n"]) * V)), "exactly the chunk's own rows, keyframe rows skipped"
        assert -1 in ch["cvx_calls"][0], "the keyframes are sources of the graph: their mask rows are skipped, not dropped"
        disps = ch["disps"].reshape(ch["n"] * V, *ch["disps"].shape[2:]).cpu().numpy()[..., None]
        mask = torch.stack([ch["masks"][r][0][ch["masks"][r][1]] for r in range(n_kf * V, (n_kf + ch["n"]) * V)]).cpu().numpy()
        ref_up, bound_up = cr.cvx_upsample_ref(disps, mask)[..., 0], cr.cvx_bound(disps)[..., 0]
        inp = e["inp"].cpu().numpy()
        for k, r in enumerate(e["rows"]):
            if r >= n_kf * V:  # a pass-2 row
                q = r - n_kf * V
                err = np.abs(inp[k].astype(np.float64) - ref_up[q])
                worst_cvx = max(worst_cvx, float((err / np.maximum(bound_up[q], 1e-300)).max()))
                assert (err <= bound_up[q]).all(), f"{what}: row {r} is not the final disparity under the last mask"
            else:  # a keyframe's frame: the global BA's row, bit for bit
                assert torch.equal(e["inp"][k], kf_up[r]), f"{what}: keyframe row {r}"
        ref, bound = dr.depth_export_ref(inp, e["params"]), dr.depth_bound(inp, e["params"])
        assert np.isfinite(bound).all()
        got = e["out"]
        if got.dtype == torch.float16:  # the f16 store is monotone: between the roundings of the interval's ends
            lo = torch.from_numpy(ref - bound).half().float().numpy()
            hi = torch.from_numpy(ref + bound).half().float().numpy()
            g = got.float().cpu().numpy()
            assert ((g >= lo) & (g <= hi)).all(), f"{what}: f16 export output"
        else:
            err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
            worst_exp = max(worst_exp, float((err / bound).max()))
            assert (err <= bound).all(), f"{what}: export output"
        outs.append(got)
    print(f"{what}: pass-2 rows max err / cvx bound = {worst_cvx:.3f}, f32 export max err / bound = {worst_exp:.3f}")
    return torch.cat(outs)


def test_off_nothing_is_called_or_returned(off_run, on_run):
    out, sysm, rec = off_run["out"], off_run["sysm"], off_run["rec"]
    assert out.frame_depths is None and out.frame_disps_lowres is None and out.keyframe_disps_up is None
    assert sysm.buffer.disps_up is None
    assert len(rec.exports) == 0 and len(rec.cvx_calls) == 0
    assert len(rec.chunks) == 4 and not any(ch["upsample"] for ch in rec.chunks)
    assert all(ch["from_row"] is None for ch in rec.chunks)
    assert not sysm.inner_filler.args.infill_dense_disp and not sysm.inner_filler.upsample_own_rows
    assert out.keyframe_ids.tolist() == on_run["out"].keyframe_ids.tolist()
    kf = out.keyframe_ids.tolist()
    assert 0 in kf and 12 in kf and 3 <= len(kf) <= 6, "both kinds of frame are needed"


def test_on_shapes_and_lowres(on_run):
    out, sysm, rec = on_run["out"], on_run["sysm"], on_run["rec"]
    fd = out.frame_depths
    assert tuple(fd.shape) == (13, 1, 128, 512) and fd.dtype == torch.float16
    assert bool(torch.isfinite(fd).all()) and bool((fd > 0).all())
    assert tuple(out.frame_disps_lowres.shape) == (13, 1, 16, 64) and out.frame_disps_lowres.dtype == torch.float32
    assert torch.equal(out.frame_disps_lowres, torch.cat([ch["disps"] for ch in rec.chunks]))
    assert [ch["n"] for ch in rec.chunks] == [4, 4, 4, 1]
    assert sysm.inner_filler.args.infill_dense_disp and not on_run["cfg"].infill.infill_dense_disp  # the caller's stays
    assert sysm.frontend.graph.upsample and sysm.backend.last_graph.upsample


def test_on_non_keyframe_and_keyframe_frames(on_run):
    out, sysm = on_run["out"], on_run["sysm"]
    got = check_exports(on_run, 13, "one view")
    assert torch.equal(got.view(13, 1, 128, 512), out.frame_depths)
    n_kf = len(out.keyframe_ids)
    # the keyframes' rows are the global BA's: pass 2 left them alone, and the slots behind them are free again
    assert torch.equal(on_run["rec"].kf_up_before_pass2, out.keyframe_disps_up)
    assert torch.equal(sysm.buffer.disps_up[:n_kf], out.keyframe_disps_up)
    assert bool(out.keyframe_disps_up_valid.all())
    assert not bool(sysm.buffer.disps_up_valid[n_kf:].any())


def test_native_resolution(native_run):
    from vipe_amd.slam.ingest import StandardResize, export_params
    out = native_run["out"]
    r = StandardResize(160, 600)
    assert tuple(out.frame_depths.shape) == (9, 1, 160, 600) and out.frame_depths.dtype == torch.float16
    assert tuple(out.frame_disps_lowres.shape) == (9, 1, r.out_size[0] // 8, r.out_size[1] // 8)
    assert all(e["params"] == export_params(r, *r.out_size) for e in native_run["rec"].exports)
    got = check_exports(native_run, 9, "native resolution")
    assert torch.equal(got.view(9, 1, 160, 600), out.frame_depths)
    assert bool(torch.isfinite(out.frame_depths).all()) and bool((out.frame_depths > 0).all())


def test_two_view_rig(rig_run):
    out, sysm = rig_run["out"], rig_run["sysm"]
    assert sysm.buffer.n_views == 2
    assert tuple(out.frame_depths.shape) == (10, 2, 128, 512) and out.frame_depths.dtype == torch.float32
    assert tuple(out.frame_disps_lowres.shape) == (10, 2, 16, 64)
    kf = out.keyframe_ids.tolist()
    assert 0 < len(kf) < 10, "both kinds of frame are needed"
    got = check_exports(rig_run, 10, "two views")  # rows are frame * V + view
    assert torch.equal(got.view(10, 2, 128, 512), out.frame_depths)
    assert not bool(sysm.buffer.disps_up_valid[len(kf):].any())


def test_sink_and_artifacts(sink_run):
    from vipe_amd.driver.artifacts import read_depth_artifacts
    out, calls = sink_run["out"], sink_run["calls"]
    assert out.frame_depths is None and out.frame_disps_lowres is not None
    assert [(f, v) for f, v, _ in calls] == [(f, 0) for f in range(13)]
    assert all(tuple(d.shape) == (128, 512) and d.dtype == torch.float16 and d.is_cuda for _, _, d in calls)
    got = check_exports(sink_run, 13, "sink")
    assert torch.equal(got, torch.stack([d for _, _, d in calls]))
    assert sink_run["written"] == 13
    read = list(read_depth_artifacts(sink_run["path"]))
    assert [i for i, _ in read] == list(range(13))
    for (i, d), (_, _, want) in zip(read, calls):
        assert d.dtype == torch.float32 and torch.equal(d.half(), want.cpu())


def test_upsample_disps_alone_keeps_pass_2_motion_only(up_only_run):
    out, sysm, rec = up_only_run["out"], up_only_run["sysm"], up_only_run["rec"]
    assert out.frame_depths is None and out.frame_disps_lowres is None and out.keyframe_disps_up is not None
    assert len(rec.exports) == 0
    assert not any(ch["upsample"] for ch in rec.chunks) and not sysm.inner_filler.last_graph.upsample
    assert not any(ch["cvx_calls"] for ch in rec.chunks)
    assert not sysm.inner_filler.args.infill_dense_disp
    assert not bool(sysm.buffer.disps_up_valid[len(out.keyframe_ids):].any())


def test_rescale_helper():
    from vipe_amd.slam.interface import rescale_frame_depths
    d = torch.tensor([[0.5, 2.0, 0.0]], dtype=torch.float16, device=dev())
    r = rescale_frame_depths(d, 3.0)
    assert r.dtype == torch.float16 and r.cpu().tolist() == [[1.5, 6.0, 0.0]]
