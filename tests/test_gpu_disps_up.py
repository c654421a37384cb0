"""Full-resolution keyframe disparities end to end: `SLAMConfig.upsample_disps` -> `GraphBuffer.disps_up` ->
`SLAMOutput.keyframe_disps_up`, on short random clips with random-init weights (seed 0).

`droid_net_ext.cvx_upsample` is the single route from the graph to the kernel, so the tests wrap it: a call counter for
the run with the feature off, and for the runs with it on a record of the last mask every buffer row was upsampled
with.  After the run `disps_up` of every keyframe must be the float64 reference (tests/cvx_reference.py) of the FINAL
`buffer.disps` under that last mask, within the kernel's derived bound - which fails if the upsampling ran before the
BA, if `update_batch` used the mask of an earlier pass, or if mask rows and buffer rows are misaligned.  Values of two
runs are never compared: the BA's atomics are order dependent; the keyframe decisions are the reproducible part."""
import numpy as np
import pytest
import torch

import cvx_reference as cr

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


class Recorder:
    """wraps droid_net_ext.cvx_upsample: counts the calls and keeps, per flattened buffer row, the mask row it was last
    upsampled with (a clone: the graph's mask tensors are recycled)"""

    def __init__(self):
        from vipe_amd.ext import droid_net_ext
        self.mod, self.real = droid_net_ext, droid_net_ext.cvx_upsample
        self.calls, self.last = 0, {}

    def __enter__(self):
        def wrapped(data, mask, rows=None, out=None, **kw):
            self.calls += 1
            res = self.real(data, mask, rows=rows, out=out, **kw)
            keep = mask.clone()
            idx = range(mask.shape[0]) if rows is None else rows.cpu().tolist()
            for s, r in enumerate(idx):
                self.last[int(r)] = (keep, s)
            return res
        self.mod.cvx_upsample = wrapped
        return self

    def __exit__(self, *exc):
        self.mod.cvx_upsample = self.real


def one_view_frames(T=12, H=128, W=512):
    from vipe_amd.ext.lietorch import SE3
    from vipe_amd.slam.system import Frame
    gen = torch.Generator().manual_seed(5)
    rgb = torch.rand(T, H, W, 3, generator=gen).to(dev())
    depth = (1.0 + 4.0 * torch.rand(T, H, W, generator=gen)).to(dev())
    intr = torch.tensor([460.8, 460.8, 256.0, 64.0])
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


def run_clip(frames, upsample, rig=None, backend_at=(10,)):
    """-> dict(out, sysm, rec) of one SLAMSystem.run with the wrapper in place"""
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    torch.manual_seed(0)
    cfg = SLAMConfig(buffer=40, filter_thresh=0.0, frontend_backend_iters=backend_at,
                     frontend=FrontendArgs(keyframe_thresh=0.0), infill=InfillArgs(infill_chunk_size=4),
                     upsample_disps=upsample)
    sysm = SLAMSystem(dev(), cfg)
    fired = {"n": 0}
    real_build = sysm._build_components

    def build(*a, **k):
        real_build(*a, **k)
        real_run = sysm.backend.run_if_necessary

        def run_if(*a, **k):
            fired["n"] += 1
            return real_run(*a, **k)
        sysm.backend.run_if_necessary = run_if
    sysm._build_components = build
    with Recorder() as rec:
        out = sysm.run(frames, rig=rig)
        torch.cuda.synchronize()
    return dict(out=out, sysm=sysm, rec=rec, fired=fired["n"])


@pytest.fixture(scope="module")
def off_run():
    return run_clip(one_view_frames(), upsample=False)


@pytest.fixture(scope="module")
def on_run():
    return run_clip(one_view_frames(), upsample=True)


@pytest.fixture(scope="module")
def rig_run():
    frames, rig = two_view_frames()
    return run_clip(frames, upsample=True, rig=rig, backend_at=())


def check_against_last_masks(run, what):
    """staleness + convexity of every keyframe row against the final 1/8 disparities"""
    b, out, rec = run["sysm"].buffer, run["out"], run["rec"]
    n_kf, V = out.keyframe_disps_up.shape[:2]
    rows = list(range(n_kf * V))
    assert all(r in rec.last for r in rows), "a keyframe row was never upsampled"
    disps = b.flattened_disps[: n_kf * V].cpu().numpy()[..., None]           # [rows,h,w,1], the FINAL 1/8 maps
    mask = torch.stack([rec.last[r][0][rec.last[r][1]] for r in rows]).cpu().numpy()  # row r's last mask, exact fp16 values
    got = out.keyframe_disps_up.reshape(n_kf * V, *out.keyframe_disps_up.shape[2:]).cpu().numpy()[..., None]
    assert np.array_equal(got, b.flattened_disps_up[: n_kf * V].cpu().numpy()[..., None])
    ref = cr.cvx_upsample_ref(disps, mask)
    bound = cr.cvx_bound(disps)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{what}: staleness max |err| / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), f"{what}: disps_up is not the final disparities under the last mask"
    lo, hi = cr.neighbourhood_minmax(disps)  # the padding's 0 is in the range at the border
    assert (got >= lo - bound).all() and (got <= hi + bound).all(), f"{what}: not a convex combination"


def test_off_nothing_is_allocated_or_called(off_run):
    out, b = off_run["out"], off_run["sysm"].buffer
    assert out.keyframe_disps_up is None and out.keyframe_disps_up_valid is None
    assert getattr(b, "disps_up", None) is None and getattr(b, "disps_up_valid", None) is None
    assert off_run["rec"].calls == 0
    assert off_run["fired"] == 1  # the configured keyframe count was reached once
    assert not off_run["sysm"].frontend.graph.upsample and not off_run["sysm"].backend.last_graph.upsample


def test_on_shapes_and_bookkeeping(on_run, off_run):
    out, sysm = on_run["out"], on_run["sysm"]
    n_kf = len(out.keyframe_ids)
    assert n_kf == sysm.buffer.n_frames == 12
    assert tuple(out.keyframe_disps_up.shape) == (n_kf, 1, 128, 512) and out.keyframe_disps_up.dtype == torch.float32
    assert tuple(out.keyframe_disps_up_valid.shape) == (n_kf, 1) and bool(out.keyframe_disps_up_valid.all())
    assert bool(torch.isfinite(out.keyframe_disps_up).all())
    assert out.keyframe_ids.tolist() == off_run["out"].keyframe_ids.tolist()
    assert on_run["rec"].calls > 0 and on_run["fired"] == 1
    assert sysm.frontend.graph.upsample and sysm.backend.last_graph.upsample
    assert not sysm.inner_filler.last_graph.upsample  # pass 2 (non-keyframe depth) is out of scope
    assert not bool(sysm.buffer.disps_up_valid[n_kf:].any())  # nothing beyond the keyframes was ever upsampled


def test_on_disps_up_is_the_final_disparity_under_the_last_mask(on_run):
    check_against_last_masks(on_run, "one view")


def test_two_view_rig(rig_run):
    out, sysm = rig_run["out"], rig_run["sysm"]
    assert sysm.buffer.n_views == 2 and out.keyframe_ids.tolist() == list(range(10))
    assert tuple(out.keyframe_disps_up.shape) == (10, 2, 128, 512)
    assert tuple(out.keyframe_disps_up_valid.shape) == (10, 2) and bool(out.keyframe_disps_up_valid.all())
    assert bool(torch.isfinite(out.keyframe_disps_up).all())
    check_against_last_masks(rig_run, "two views")  # rows are frame * V + view


def test_remove_second_newest_shifts_disps_up():
    from vipe_amd.slam.buffer import GraphBuffer
    b = GraphBuffer(64, 128, n_views=2, buffer_size=6, device=dev(), upsample_disps=True)
    assert tuple(b.disps_up.shape) == (6, 2, 64, 128) and b.disps_up.dtype == torch.float32 and not bool(b.disps_up.any())
    assert tuple(b.disps_up_valid.shape) == (6, 2) and b.disps_up_valid.dtype == torch.bool and not bool(b.disps_up_valid.any())
    for k in range(6):
        for v in range(2):
            b.disps_up[k, v] = 10.0 * k + v + 1.0
            b.disps[k, v] = 100.0 * k + v + 1.0
    b.disps_up_valid[:] = torch.tensor([[1, 1], [1, 0], [0, 1], [0, 0], [1, 0], [0, 0]], dtype=torch.bool, device=dev())
    up0, d0, valid0 = b.disps_up.clone(), b.disps.clone(), b.disps_up_valid.clone()
    b.n_frames = 5
    b.remove_second_newest(3)
    assert b.n_frames == 4
    keep = [0, 1, 2, 4, 5]
    assert torch.equal(b.disps_up[3], up0[4]) and torch.equal(b.disps_up[keep], up0[keep])      # like disps ...
    assert torch.equal(b.disps[3], d0[4]) and torch.equal(b.disps[keep], d0[keep])
    assert torch.equal(b.disps_up_valid[3], valid0[4]) and torch.equal(b.disps_up_valid[[0, 1, 2, 5]], valid0[[0, 1, 2, 5]])
    assert not bool(b.disps_up_valid[4].any())  # ... and the freed slot is not valid for whatever keyframe takes it next
    off = GraphBuffer(64, 128, n_views=2, buffer_size=6, device=dev())
    assert off.disps_up is None and off.disps_up_valid is None and off.flattened_disps_up is None
