"""`KLTSparseTracks` on the device against the run of the same class driven by the float64 reference (the CPU test's
run), against ground truth, and inside `SLAMSystem.run` through `SLAMConfig(sparse_tracks="klt")`."""
import numpy as np
import pytest
import torch

import klt_reference as K

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def test_tracker_on_the_device_matches_the_reference_driven_run():
    kern = K.NumpyKernels()
    ref, _ = K.run_sequence(kern)
    got, _ = K.run_sequence(None, device=dev())
    torch.cuda.synchronize()
    _, _, warps = K.sequence_inputs()
    assert kern.excluded == 0  # no decision of the reference run is near a tie or a threshold: the runs must agree exactly
    ro, go = ref.observations[0], got.observations[0]
    assert len(go) == len(ro) == 6
    born, start, worst = {}, {}, 0.0
    for k, (a, b) in enumerate(zip(ro, go)):
        assert set(a) == set(b), f"frame {k}: other survivors or ids than the reference-driven run"
        for i in a:
            if i not in born:
                born[i], start[i] = k, a[i]
                assert np.array_equal(a[i], b[i])  # a new corner is a pixel
            else:
                err = np.abs(a[i] - b[i]).max() / ((k - born[i]) * K.TRACK_BOUND)  # one bound per tracked step
                worst = max(worst, err)
    print(f"device against reference-driven run: positions at most {worst:.3f} x (steps x TRACK_BOUND)")
    assert worst <= 1.0
    last = go[5]
    old = [i for i in last if born[i] < 5]
    truth = np.stack([warps[5].forward(warps[born[i]].inverse(start[i][None]))[0] for i in old])
    err = np.linalg.norm(np.stack([last[i] for i in old]) - truth, axis=1)
    print(f"{len(old)} tracks at the last frame, {np.mean(err < 0.15) * 100:.0f} % within 0.15 px of the truth (max {err.max():.3f})")
    assert len(old) >= 20 and np.mean(err < 0.15) >= 0.9


def _clip(H, W, T=8):
    from vipe_amd.slam.system import Frame
    frames, _ = K.make_sequence(T, H, W)
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    return [Frame(rgb=torch.from_numpy(f).to(dev()), intrinsics=intr) for f in frames]


def _config(**kw):
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.system import SLAMConfig
    return SLAMConfig(buffer=48, filter_thresh=0.0, frontend_backend_iters=(), frontend=FrontendArgs(keyframe_thresh=0.0),
                      infill=InfillArgs(infill_chunk_size=8), **kw)


def _count_klt_calls(monkeypatch):
    from vipe_amd.ext import klt_ext
    calls = dict(pyramid=0, detect=0, track=0)
    for name in calls:
        def wrapped(*a, _f=getattr(klt_ext, name), _n=name, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(klt_ext, name, wrapped)
    return calls


def test_slam_system_with_the_configured_tracker(monkeypatch):
    from vipe_amd.slam.sparse_tracks import KLTSparseTracks
    from vipe_amd.slam.system import SLAMSystem
    calls = _count_klt_calls(monkeypatch)
    sums = []
    inner = KLTSparseTracks.compute_dense_disp_target_weight

    def recording(self, *a, **k):
        target, weight = inner(self, *a, **k)
        sums.append(float(weight.sum()))
        return target, weight
    monkeypatch.setattr(KLTSparseTracks, "compute_dense_disp_target_weight", recording)
    frames = _clip(128, 512)
    torch.manual_seed(0)
    sysm = SLAMSystem(dev(), _config(sparse_tracks="klt"))
    out = sysm.run(frames)
    torch.cuda.synchronize()
    assert out.trajectory.data.shape == (8, 7) and bool(torch.isfinite(out.trajectory.data).all())
    tr = sysm.sparse_tracks
    assert isinstance(tr, KLTSparseTracks) and len(tr.observations[0]) == 8
    assert all(len(o) > 50 for o in tr.observations[0][1:])
    assert len(tr.get_correspondences(0, 0, 7)) > 20  # tracks live through the clip
    assert calls["pyramid"] == 8 and calls["detect"] == 8 and calls["track"] == 14
    assert sums and max(sums) > 0, "no BA received a track term"
    print(f"{len(sums)} BA calls with a track term, weight sums up to {max(sums):.1f}")


def test_slam_system_native_resolution_reports_at_slam_resolution():
    from vipe_amd.slam.ingest import StandardResize
    from vipe_amd.slam.system import SLAMSystem
    frames = _clip(270, 480)
    torch.manual_seed(0)
    sysm = SLAMSystem(dev(), _config(sparse_tracks="klt"))
    out = sysm.run(frames, native_resolution=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out.trajectory.data).all())
    H, W = StandardResize(270, 480).out_size
    obs = sysm.sparse_tracks.observations[0]
    assert len(obs) == 8 and all(len(o) > 50 for o in obs)
    uv = np.stack([p for o in obs for p in o.values()])
    assert uv[:, 0].min() >= 0 and uv[:, 0].max() <= W - 1 and uv[:, 1].min() >= 0 and uv[:, 1].max() <= H - 1
    assert uv[:, 0].max() > 480  # reported in the resized frame (584 wide), not in the native one


def test_slam_system_without_the_option_builds_and_calls_nothing(monkeypatch):
    from vipe_amd.slam.system import SLAMSystem
    calls = _count_klt_calls(monkeypatch)
    frames = _clip(128, 512)
    torch.manual_seed(0)
    sysm = SLAMSystem(dev(), _config())
    assert sysm.config.sparse_tracks is None
    out = sysm.run(frames)
    torch.cuda.synchronize()
    assert sysm.sparse_tracks is None and sysm.buffer.sparse_tracks is None and sysm.motion_filter.sparse_tracks is None
    assert calls == dict(pyramid=0, detect=0, track=0)
    assert out.trajectory.data.shape == (8, 7) and bool(torch.isfinite(out.trajectory.data).all())
