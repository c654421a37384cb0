"""`SLAMConfig.disp_uncertainty` end to end: `SLAMSystem.run` -> `FactorGraph.marginals` on the last backend graph ->
`SLAMOutput.keyframe_disp_var` / `keyframe_pose_cov`, on the 12-frame clip and the two-camera rig clip of
tests/test_gpu_disps_up.py (random-init weights, seed 0).

`slam_ext.dense_ba_marginals` is the single route from the graphs to the library, so the tests wrap it with a call
counter.  Values of two runs are never compared (the BA's atomics are order dependent); the output of the run with the flag
on is compared with a direct `GraphBuffer.ba_marginals` on `backend.last_graph` at the final state: pass 2 leaves the
keyframes' poses and disparities as the last backend pass left them, so both evaluate the same linear system and differ
only by the summation order of the accumulate kernels' atomics.  The clips' conditioning is not known in advance (random
weights), so that comparison is held to 1e-3 relative: a wrong window, damping, flag or row alignment moves the values by
O(1).  `run` applies no metric rescaling in this build; the rule itself is pinned on the CPU (tests/test_ba_marginals_abi.py).
"""
import numpy as np
import pytest
import torch

from test_gpu_disps_up import dev, one_view_frames, two_view_frames

pytestmark = pytest.mark.gpu


class Counter:
    def __init__(self):
        from vipe_amd.ext import slam_ext
        self.mod, self.real, self.calls = slam_ext, slam_ext.dense_ba_marginals, 0

    def __enter__(self):
        def wrapped(*a, **k):
            self.calls += 1
            return self.real(*a, **k)
        self.mod.dense_ba_marginals = wrapped
        return self

    def __exit__(self, *exc):
        self.mod.dense_ba_marginals = self.real


def run_clip(frames, on, rig=None, backend_at=(10,)):
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    torch.manual_seed(0)
    cfg = SLAMConfig(buffer=40, filter_thresh=0.0, frontend_backend_iters=backend_at,
                     frontend=FrontendArgs(keyframe_thresh=0.0), infill=InfillArgs(infill_chunk_size=4),
                     **({"disp_uncertainty": True} if on else {}))
    sysm = SLAMSystem(dev(), cfg)
    with Counter() as cnt:
        out = sysm.run(frames, rig=rig)
        torch.cuda.synchronize()
    return dict(out=out, sysm=sysm, calls=cnt.calls)


@pytest.fixture(scope="module")
def off_run():
    return run_clip(one_view_frames(), on=False)


@pytest.fixture(scope="module")
def on_run():
    return run_clip(one_view_frames(), on=True)


@pytest.fixture(scope="module")
def rig_run():
    frames, rig = two_view_frames()
    return run_clip(frames, on=True, rig=rig, backend_at=())


def test_off_nothing_is_computed(off_run):
    out = off_run["out"]
    assert out.keyframe_disp_var is None and out.keyframe_pose_cov is None
    assert off_run["calls"] == 0 and not hasattr(off_run["sysm"], "marginals")


def check_run(run, n_kf, V, what):
    out, sysm = run["out"], run["sysm"]
    b, g = sysm.buffer, sysm.backend.last_graph
    assert run["calls"] == 1, "one marginals call per clip"
    assert len(out.keyframe_ids) == n_kf == b.n_frames
    dv, pc = out.keyframe_disp_var, out.keyframe_pose_cov
    assert tuple(dv.shape) == (n_kf, V, 16, 64) and dv.dtype == torch.float32
    assert tuple(pc.shape) == (n_kf, 6, 6)
    # the backend's problem: t0 = 1, t1 = n_kf; keyframe 0 is a source outside the window (the gauge), every other pose is
    # free; a disparity frame is free iff it is the source of a term
    edges = g.host_edges()
    assert 0 in edges["ii"]
    src = np.zeros(n_kf, bool)
    src[np.unique(edges["ii"])] = True
    fin_d = torch.isfinite(dv).flatten(2).all(2).cpu().numpy()
    nan_d = torch.isnan(dv).flatten(2).all(2).cpu().numpy()
    assert np.array_equal(fin_d, np.repeat(src[:, None], V, 1)) and np.array_equal(nan_d, ~fin_d)
    assert bool((dv[torch.isfinite(dv)] > 0).all())
    assert bool(torch.isnan(pc[0]).all()) and bool(torch.isfinite(pc[1:]).all())
    assert bool((torch.diagonal(pc[1:], dim1=1, dim2=2) > 0).all())
    assert torch.allclose(pc[1:], pc[1:].transpose(1, 2), rtol=1e-9, atol=0)
    # a direct evaluation on the last backend graph at the final state, with the last pass's BA arguments
    E = g.target.shape[1]
    a = g._last_ba
    assert (a["t0"], a["t1"], a["pose_damping"], a["pose_ep"]) == (1, n_kf, 1e-5, 1e-2)
    dv2, pc2, info = b.ba_marginals(g.target.view(E, -1, 2), g.weight.view(E, -1, 2), g.damping, g.ii, g.jj, **a)
    torch.cuda.synchronize()
    assert int(info[0]) == n_kf - 1 and int(info[1]) == int(src.sum()) * V
    dv2 = dv2[:n_kf * V].view(n_kf, V, 16, 64)
    m = torch.isfinite(dv)
    assert torch.equal(m, torch.isfinite(dv2))
    e_v = float(((dv2[m] - dv[m]).abs() / dv[m]).max())
    sd = torch.sqrt(torch.diagonal(pc[1:], dim1=1, dim2=2))
    e_c = float(((pc2[1:n_kf] - pc[1:]).abs() / (sd[:, :, None] * sd[:, None, :])).max())
    print(f"{what}: run output vs direct ba_marginals: disp_var {e_v:.3g}, pose_cov {e_c:.3g} relative; "
          f"variance {float(dv[m].min()):.3g} .. {float(dv[m].max()):.3g}")
    assert e_v <= 1e-3 and e_c <= 1e-3


def test_on_one_view(on_run, off_run):
    assert on_run["out"].keyframe_ids.tolist() == off_run["out"].keyframe_ids.tolist()
    check_run(on_run, 12, 1, "one view")


def test_on_two_view_rig(rig_run):
    check_run(rig_run, 10, 2, "two views")
