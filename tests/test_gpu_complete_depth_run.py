"""The completed depth maps end to end: `SLAMConfig.complete_depth` -> in `_render_fused_depths`' chunk loop, right after
the resolve, one `vipe_depth_anchor_bits` and one `vipe_depth_complete` launch per pass-2 chunk -> `SLAMOutput.complete_depths`
beside `fused_depths` and `frame_depths`.  The clips are those of tests/test_gpu_fused_depth_run.py, run through its
`run_clip` (so every render and resolve is still checked against its own reference by `check_run`).

`ingest.depth_complete` is the single route to the two kernels, so the tests wrap it: every call's arguments are copied as
the kernels saw them and each chunk's result is held against tests/depth_complete_reference.py of exactly those arguments
(`check_image`: anchors bit for bit, every other pixel inside the bound of a branch it may take, 0 only where the
reference admits it).  The library handle `ingest` calls through is wrapped as well, which gives the order of the
launches.  The runs use radius 8, so that the reference's offset walk stays quick on 128 x 512 and 160 x 600 images.

The share of undecided targets.  A fused point is drawn over a footprint of up to 5 x 5 pixels, all with one depth, so in
these maps the nearest anchors of a hole pixel often hold one and the same sparse value.  Then cov is zero in exact
arithmetic and the sign of s = cov / var is rounding's: whether the pixel comes out by the affine fit (s about 0, t about
that value) or by the scale-only one is decided by no bound, in float32 or any other precision.  Such targets
(`flat` of the reference) are held to the bound of either branch like every undecided target, but they are counted
apart; the 2 % cap of the seeded cases is asserted on the rest.  The counts of the first device run are in DESIGN.md
section 20."""
import numpy as np
import pytest
import torch

import depth_complete_reference as dr
import test_gpu_frame_depth as fd
import test_gpu_fused_depth_run as fr

pytestmark = pytest.mark.gpu

STAGE = ("vipe_cloud_render", "vipe_cloud_resolve", "vipe_depth_anchor_bits", "vipe_depth_complete")
K, R = 4, 8


class CompleteRecorder:
    """wraps `ingest.depth_complete` (arguments, result, inputs untouched) and `ingest.lib` (the order of the launches)"""

    def __init__(self):
        from vipe_amd.slam import ingest
        self.mod, self.real, self.real_lib = ingest, ingest.depth_complete, ingest.lib
        self.calls, self.launches = [], []

    def __enter__(self):
        rec = self

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(rec.real_lib(), name)

                def call(*a):
                    rec.launches.append(name)
                    return fn(*a)
                return call

        def depth_complete(sparse, pred, **kw):
            before = (sparse.clone(), pred.clone())
            res = rec.real(sparse, pred, **kw)
            torch.cuda.synchronize()
            rec.calls.append(dict(sparse=sparse.cpu().numpy(), pred=pred.cpu().numpy(), kw=dict(kw), out=res[0],
                                  got=res[0].cpu().numpy(), stats=res[4].cpu().numpy().copy(),
                                  untouched=torch.equal(before[0].view(torch.uint8), sparse.view(torch.uint8))
                                  and torch.equal(before[1].view(torch.uint8), pred.view(torch.uint8))))
            return res

        self.mod.depth_complete, self.mod.lib = depth_complete, lambda: Proxy()
        return self

    def __exit__(self, *exc):
        self.mod.depth_complete, self.mod.lib = self.real, self.real_lib


def run_clip(frames, rig=None, **cfg_kw):
    with CompleteRecorder() as crec:
        run = fr.run_clip(frames, rig=rig, fused_depth=True, **cfg_kw)
    run["crec"] = crec
    return run


ON = dict(complete_depth=True, complete_depth_k=K, complete_depth_radius=R)


@pytest.fixture(scope="module")
def off_run():
    return run_clip(fd.one_view_frames())


@pytest.fixture(scope="module")
def on_run():
    return run_clip(fd.one_view_frames(), **ON)


@pytest.fixture(scope="module")
def native_run():
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(6)
    T, H, W = 9, 160, 600
    rgb = (255 * torch.rand(T, H, W, 3, generator=gen)).to(torch.uint8).to(fd.dev())
    depth = (1.0 + 4.0 * torch.rand(T, H, W, generator=gen)).to(fd.dev())
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    frames = [Frame(rgb=rgb[t], metric_depth=depth[t], intrinsics=intr) for t in range(T)]
    return run_clip(frames, fused_depth_max_radius=1, frame_depth_dtype=torch.float32, native_resolution=True, **ON)


@pytest.fixture(scope="module")
def rig_run():
    frames, rig = fd.two_view_frames()
    return run_clip(frames, rig=rig, frame_depth_conf_neighbours=2, **ON)


@pytest.fixture(scope="module")
def sink_run():
    calls = []
    run = run_clip(fd.one_view_frames(), complete_depth_sink=lambda f, v, d: calls.append((f, v, d.clone())), **ON)
    run["calls"] = calls
    return run


def check_run(run, T, what, maps=None):
    """the fused stage as before (`fr.check_run`), then every completion call against the reference of its arguments"""
    fused = fr.check_run(run, T, what)
    out, crec, cfg, b = run["out"], run["crec"], run["cfg"], run["sysm"].buffer
    V = b.n_views
    chunks = [list(range(c0, min(c0 + 4, T))) for c0 in range(0, T, 4)]
    assert [n for n in crec.launches if n in STAGE] == list(STAGE) * len(chunks), \
        f"{what}: per chunk one bits and one complete launch, right after the resolve"
    assert len(crec.calls) == len(chunks)
    maps = out.complete_depths if maps is None else maps
    size = tuple(out.frame_depths.shape[2:])
    assert tuple(maps.shape) == (T, V) + size and maps.dtype == cfg.frame_depth_dtype
    bits = torch.int16 if maps.dtype == torch.float16 else torch.int32
    targets = undecided = flat = 0
    want = np.zeros(4, dtype=np.int64)
    for call, frames in zip(crec.calls, chunks):
        n = len(frames)
        assert call["untouched"], f"{what}: the chunk's fused and frame maps are bitwise what they were"
        kw = call["kw"]
        assert (kw["K"], kw["radius"], kw["domain"], kw["wrap_x"]) == (K, R, "depth", False) and kw.get("mask") is None
        # the arguments: the chunk's fused maps and the chunk's frame maps
        assert np.array_equal(call["sparse"], fused[frames[0]:frames[0] + n].reshape(n * V, *size).cpu().numpy())
        assert np.array_equal(call["pred"], out.frame_depths[frames[0]:frames[0] + n].reshape(n * V, *size).cpu().numpy())
        got = maps[frames[0]:frames[0] + n].reshape(n * V, *size)
        assert torch.equal(got.view(bits), call["out"].view(bits)), f"{what}: frames {frames}"
        for i in range(n * V):
            ref = dr.complete_ref(call["sparse"][i], call["pred"][i], K, R, "depth", scan=True)
            t, u = dr.check_image(ref, call["sparse"][i], call["got"][i])
            targets, undecided, want = targets + t, undecided + u, want + ref["stats"]
            flat += int((~ref["decided"] & ref["flat"]).sum())
    stats = np.array([out.complete_depth_stats[k] for k in ("affine", "scale_only", "unreached", "rejected")])
    assert np.array_equal(stats, crec.calls[-1]["stats"]), "one set of counters per clip, added to by every chunk"
    print(f"{what}: {targets} targets, {undecided} undecided of which {flat} with one sparse value at all neighbours, "
          f"counters {stats.tolist()} against {want.tolist()}")
    assert int(stats.sum()) == targets and np.abs(stats - want).max() <= undecided
    assert undecided - flat <= dr.UNDECIDED_CAP * targets
    # the fused surface is kept where it exists, and most of what it lacks is filled
    has = fused > 0
    assert torch.equal(maps.view(bits)[has], fused.view(bits)[has]), f"{what}: fused pixels are copied bit for bit"
    assert targets > 1000 and stats[0] + stats[1] > 0.5 * targets, f"{what}: holes are filled"
    assert float((maps > 0).float().mean()) > float(has.float().mean())
    return maps


def test_off_neither_route_is_called(off_run):
    out, crec = off_run["out"], off_run["crec"]
    assert out.complete_depths is None and out.complete_depth_stats is None and out.fused_depths is not None
    assert not crec.calls and "vipe_depth_anchor_bits" not in crec.launches and "vipe_depth_complete" not in crec.launches
    assert [n for n in crec.launches if n in STAGE] == ["vipe_cloud_render", "vipe_cloud_resolve"] * 4


def test_on_every_launch_and_the_maps(on_run, off_run):
    check_run(on_run, 13, "one view")
    assert on_run["out"].keyframe_ids.tolist() == off_run["out"].keyframe_ids.tolist()


def test_native_resolution_and_f32(native_run):
    maps = check_run(native_run, 9, "native resolution")
    assert tuple(maps.shape[2:]) == (160, 600) and maps.dtype == torch.float32


def test_two_view_rig(rig_run):
    assert rig_run["sysm"].buffer.n_views == 2
    check_run(rig_run, 10, "two views")


def test_sink_takes_the_maps_in_frame_order(sink_run):
    out = sink_run["out"]
    assert out.complete_depths is None and out.fused_depths is not None and out.frame_depths is not None
    assert [(f, v) for f, v, _ in sink_run["calls"]] == [(f, 0) for f in range(13)]
    check_run(sink_run, 13, "sink", maps=torch.stack([d for _, _, d in sink_run["calls"]])[:, None])
