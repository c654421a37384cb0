"""The float64 references of the 360-degree panorama camera (tests/panorama_reference.py) checked on the CPU: the model
against central differences and against the reference's own convention, the Gauss-Newton solver against oracle/ba.py
with the pinhole camera plugged in, the fairness of every case the GPU tests use, and the argument errors."""
import os

import numpy as np
import pytest
import torch

import panorama_reference as R
from oracle import ba as oba
from oracle import geom as ogeom
from oracle import se3

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHARE_CAP = 0.005  # the cap tests/test_gpu_reproject.py uses for excluded pixels


# ---------------------------------------------------------------------------------------------- 1. the model

@pytest.mark.parametrize("ht,wd", [(8, 16), (12, 24), (7, 20)])
def test_projection_inverts_the_rays(ht, wd):
    b, u, v = R.rays(ht, wd)
    for s in (0.3, 1.0, 7.5):
        c, ok, _ = R.proj(b * s, ht, wd)
        assert ok.all()
        assert np.abs(c[..., 0] - u).max() < 1e-11 and np.abs(c[..., 1] - v).max() < 1e-11
    assert np.abs(np.linalg.norm(b, axis=-1) - 1).max() < 1e-15
    # the seam: column -0.5 is column wd - 0.5, and x is the principal value
    rng = np.random.default_rng(0)
    c, _, _ = R.proj(rng.normal(size=(4000, 3)), ht, wd)
    assert c[:, 0].min() >= -0.5 and c[:, 0].max() < wd - 0.5 and c[:, 1].min() >= -0.5 and c[:, 1].max() <= ht - 0.5
    c, _, _ = R.proj(np.array([[0.0, 0.3, -1.0], [-1e-9, 0.3, -1.0]]), ht, wd)
    assert c[0, 0] == -0.5 and abs(c[1, 0] + 0.5) < 1e-6


def test_projection_jacobian_matches_central_differences():
    rng = np.random.default_rng(1)
    X = rng.normal(size=(500, 3)) * np.array([1.0, 1.0, 1.0])
    X = X[np.hypot(X[:, 0], X[:, 2]) > 0.05]
    _, _, Jp = R.proj(X, 12, 24, jac=True)
    h = 1e-6
    num = np.zeros_like(Jp)
    for k in range(3):
        e = np.zeros(3)
        e[k] = h
        cp, _, _ = R.proj(X + e, 12, 24)
        cm, _, _ = R.proj(X - e, 12, 24)
        d = cp - cm
        d[:, 0] = R.wrap(d[:, 0], 24)
        num[:, :, k] = d / (2 * h)
    rel = np.abs(num - Jp).max() / np.abs(Jp).max()
    print(f"projection Jacobian against central differences: {rel:.2e} relative")
    assert rel < 1e-7


def test_term_jacobians_match_central_differences():
    """Ji, Jj, Jz of the whole term (poses on the left tangent, X <- Exp(dx) X; rig with a rotated second view)"""
    g, _, _ = R.case("g8x16_rig2")
    args = (g.pi, g.pj, g.qi, g.qj, g.di)
    poses, rig, disps = g.poses.astype(np.float64), g.rig.astype(np.float64), g.disps.astype(np.float64)
    out = R.reproject(poses, disps, rig, *args, jacobian=True)
    ok = out["valid"] & ~R.fairness_margins(out["X1"])
    h = 1e-6

    def coords(p, d):
        return R.reproject(p, d, rig, *args)["coords"]

    def diff(cp, cm):
        d = cp - cm
        d[..., 0] = R.wrap(d[..., 0], g.wd)
        return d / (2 * h)

    worst = 0.0
    for pose in (1, 2):
        for k in range(6):
            xi = np.zeros(6)
            xi[k] = h
            pp, pm = poses.copy(), poses.copy()
            pp[pose], pm[pose] = se3.se3_retr(poses[pose], xi), se3.se3_retr(poses[pose], -xi)
            num = diff(coords(pp, disps), coords(pm, disps))
            ana = np.where((g.pi == pose)[:, None, None, None], out["Ji"][..., k], 0.0) + \
                np.where((g.pj == pose)[:, None, None, None], out["Jj"][..., k], 0.0)
            worst = max(worst, np.abs(num - ana)[ok].max() / max(np.abs(ana)[ok].max(), 1.0))
    num = diff(coords(poses, disps + h), coords(poses, disps - h))
    worst = max(worst, np.abs(num - out["Jz"])[ok].max() / np.abs(out["Jz"])[ok].max())
    print(f"term Jacobians against central differences: {worst:.2e} relative")
    assert worst < 1e-6


# ---------------------------------------------------------------------------------------------- 2. the reference's convention

def test_convention_matches_the_reference():
    z = np.load(os.path.join(GOLDEN, "panorama_camera_reference.npz"))
    assert str(z["camera_type"]) == "panorama"
    from vipe_amd._lib import CAMERA_CODE
    assert CAMERA_CODE["panorama"] == 2
    ht, wd = 12, 24
    u, v = z["un"] * wd - 0.5, z["vn"] * ht - 0.5  # u_n = (u + 0.5) / wd
    b = R.ray_of(u, v, ht, wd)
    assert np.abs(b - z["xyzd"][:, :3]).max() < 1e-12
    assert np.array_equal(z["xyzd"][:, 3], z["disp"])  # the 4th component is the disparity, carried through
    c, ok, _ = R.proj(z["points"], ht, wd)
    assert ok.all()
    un = (c[:, 0] + 0.5) / wd
    dun = un - z["uvd"][:, 0]
    assert np.abs(dun - np.round(dun)).max() < 1e-12  # u_n = 1 is u_n = 0: the principal value may differ by a turn
    assert np.abs((c[:, 1] + 0.5) / ht - z["uvd"][:, 1]).max() < 1e-12
    assert np.abs(np.linalg.norm(z["points"], axis=-1) - z["uvd"][:, 2]).max() < 1e-12  # the depth it returns is the range


# ---------------------------------------------------------------------------------------------- 3. the solver

def test_solver_reproduces_the_oracle_with_the_pinhole_camera():
    from vipe_amd.synth import make_graph
    g = make_graph(n=4, height=48, width=64, radius=2, seed=3, depth_prior=True)
    pi, qi, di, pj, qj, _ = ogeom.expand_edge_multiview(g.ii, g.jj, 1)
    rig = se3.se3_identity(1, np.float64)
    kw = dict(t0=1, t1=4, pose_damping=1e-3, pose_ep=0.1)
    hist = R.gauss_newton(R.pinhole_camera(g.intrinsics), g.poses, g.disps, g.disps_sens, rig, g.target, g.weight, g.eta,
                          pi, qi, pj, qj, di, n_iters=3, **kw)
    E = len(g.ii)
    for it in range(3):
        op, od, _, _ = oba.bundle_adjustment(g.poses, g.disps[:, None], g.disps_sens[:, None], g.intrinsics, rig,
                                             g.target.reshape(E, -1, 2), g.weight.reshape(E, -1, 2), g.eta[:, None], g.ii,
                                             g.jj, n_iters=it + 1, **kw)
        ep, ed = np.abs(hist[it]["poses"] - op).max(), np.abs(hist[it]["disps"] - od[:, 0]).max()
        print(f"iteration {it + 1}: poses {ep:.1e}, disparities {ed:.1e}")
        assert ep < 1e-9 and ed < 1e-9


def test_solver_reproduces_the_oracle_on_a_rig():
    from vipe_amd.synth import make_rig_graph
    g = make_rig_graph(n=3, V=2, height=48, width=64, radius=1, seed=4)
    pi, qi, di, pj, qj, _ = ogeom.expand_edge_multiview(g.ii, g.jj, 2)
    kw = dict(t0=1, t1=3, pose_damping=1e-3, pose_ep=0.1, optimize_rig_rotation=True)
    M = len(pi)
    hist = R.gauss_newton(R.pinhole_camera(g.intrinsics), g.poses, g.disps.reshape(-1, g.ht, g.wd),
                          g.disps_sens.reshape(-1, g.ht, g.wd), g.rig, g.target, g.weight, g.eta.reshape(-1, g.ht, g.wd),
                          pi, qi, pj, qj, di, n_iters=2, **kw)
    op, od, _, orig = oba.bundle_adjustment(g.poses, g.disps, g.disps_sens, g.intrinsics, g.rig, g.target.reshape(M, -1, 2),
                                            g.weight.reshape(M, -1, 2), g.eta, g.ii, g.jj, n_iters=2, **kw)
    assert np.abs(hist[1]["poses"] - op).max() < 1e-9 and np.abs(hist[1]["rig"] - orig).max() < 1e-9
    assert np.abs(hist[1]["disps"].reshape(od.shape) - od).max() < 1e-9


# ---------------------------------------------------------------------------------------------- 4. / 5. the cases

@pytest.mark.parametrize("name", list(R.ba_cases()))
def test_cases_are_fair_and_do_what_they_claim(name):
    g, kw, hist = R.case(name)
    for it, h in enumerate(hist):
        share = R.fairness_margins(h["X1"]).mean()
        print(f"{name} iteration {it + 1}: {100 * share:.3f} % of the (term, pixel)s inside a decision margin")
        assert share < SHARE_CAP
    assert R.fairness_margins(hist[0]["X1"]).sum() == 0  # the seeds are picked so that the reprojection test excludes nothing
    first = R.reproject(g.poses, g.disps, g.rig, g.pi, g.pj, g.qi, g.qj, g.di)
    ok = first["valid"]
    dx = (first["coords"][..., 0] - g.target[..., 0])[ok]
    crossing = np.mean(np.abs(dx) > g.wd / 2)
    print(f"{name}: {100 * crossing:.1f} % of the valid terms cross the seam, {int((~ok).sum())} invalid")
    assert crossing >= 0.10
    assert np.median(np.abs(R.wrap(dx, g.wd))) < 0.5  # wrapped, the residuals are what the perturbation makes them
    assert ((g.target[..., 0] < -0.5) | (g.target[..., 0] >= g.wd - 0.5)).mean() > 0.05  # targets stored unwrapped
    assert ok.any() and (~ok).any()  # both validity branches
    front = (first["X1"][..., 2] > 0)[ok].mean()
    assert 0.25 < front < 0.75  # both hemispheres of the target camera carry terms
    # every term changes the pose error: the estimates start off the truth and the reference solver brings them closer
    e0, e4 = R.pose_error(g.poses, g.poses_gt), R.pose_error(hist[-1]["poses"], g.poses_gt)
    print(f"{name}: pose error {e0:.2e} -> {e4:.2e}")
    assert e4 < e0


def test_depth_filter_case_is_fair():
    g, thresh = R.depth_filter_case()
    count, tie = R.depth_filter(g.poses_gt, g.disps_gt, np.arange(g.n), thresh)
    print(f"depth filter: {100 * tie.mean():.2f} % of the pixels near a tie, counts {np.bincount(count.astype(int).ravel())}")
    assert tie.mean() < SHARE_CAP
    assert (count >= 2).mean() > 0.5 and (count == 0).any()  # one surface seen consistently, and pixels nothing confirms


def test_seam_case_discriminates():
    """Wrapped, the two-keyframe case converges; with the residual left unwrapped the same solver does not."""
    g = R.seam_case()
    args = (g.poses, g.disps, g.disps_sens, g.rig, g.target, g.weight, g.eta, g.pi, g.qi, g.pj, g.qj, g.di)
    kw = dict(t0=1, t1=2, n_iters=4, pose_damping=1e-3, pose_ep=0.1, motion_only=True)
    first = R.reproject(g.poses, g.disps, g.rig, g.pi, g.pj, g.qi, g.qj, g.di)
    dx = first["coords"][..., 0] - g.target[..., 0]
    assert np.mean(np.abs(dx) > g.wd / 2) > 0.3
    good = R.gauss_newton(R.panorama_camera(), *args, **kw)
    bad = R.gauss_newton(R.panorama_camera(wrap_seam=False), *args, **kw)
    e0 = R.pose_error(g.poses, g.poses_gt)
    eg, eb = R.pose_error(good[-1]["poses"], g.poses_gt), R.pose_error(bad[-1]["poses"], g.poses_gt)
    print(f"seam case: pose error {e0:.2e} -> wrapped {eg:.2e}, unwrapped {eb:.2e}")
    assert eg < 0.3 * e0 and eb > 3 * e0


# ---------------------------------------------------------------------------------------------- 6. argument errors

def test_camera_code_and_argument_errors_without_a_device():
    from vipe_amd._lib import CAMERA_CODE
    from vipe_amd.ext import slam_ext
    assert CAMERA_CODE == {"pinhole": 0, "mei": 1, "panorama": 2}
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "vipe_amd.h")).read()
    assert "#define VIPE_CAM_PANORAMA 2" in header
    for name in ("vipe_frame_distance_sphere", "vipe_depth_filter_sphere", "vipe_iproj_sphere"):
        assert f"int {name}(" in header
    t = torch.zeros(1)
    i = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="no intrinsics"):
        slam_ext.dense_ba(t, t, t, t, t, t, t, t, i, i, i, i, i, 0, 1, 1, 1e-3, 0.1, optimize_intrinsics=True, camera="panorama")
    with pytest.raises(ValueError, match="no intrinsics"):
        slam_ext.dense_ba_linearize(t, t, t, t, t, t, t, t, i, i, i, i, i, 0, 1, 1e-3, 0.1, optimize_intrinsics=True,
                                    camera="panorama")
    with pytest.raises(ValueError, match="unknown camera"):
        slam_ext.dense_ba(t, t, t, t, t, t, t, t, i, i, i, i, i, 0, 1, 1, 1e-3, 0.1, camera="fisheye")


def test_graph_buffer_refuses_pinhole_views_of_a_panorama():
    from vipe_amd.slam.buffer import GraphBuffer
    b = GraphBuffer(64, 128, n_views=1, buffer_size=4, camera_type="panorama", device=torch.device("cpu"))
    assert tuple(b.intrinsics.shape) == (1, 4) and not b.intrinsics.any()
    for what in (lambda: b.K, lambda: b.K_dense_disp, b._pinhole_intrinsics_8, lambda: b.update_disps_sens(object(), 0),
                 lambda: b.frame_distance_dense_disp(torch.tensor([0]), torch.tensor([1]), fused=False)):
        with pytest.raises(ValueError, match="panorama"):
            what()


def _system(**kw):
    from vipe_amd.slam.system import SLAMConfig, SLAMSystem
    cfg = SLAMConfig(**kw.pop("config", {}))
    return SLAMSystem(torch.device("cpu"), cfg, droid_net=object(), **kw)


def _frames(intr=None, T=2):
    from vipe_amd.slam.system import Frame
    return [Frame(rgb=torch.zeros(64, 128, 3), intrinsics=torch.zeros(4) if intr is None else intr) for _ in range(T)]


def test_slam_system_rejections_without_a_device():
    from vipe_amd.slam.backend import BackendArgs
    with pytest.raises(ValueError, match="native_resolution"):
        _system().run(_frames(), camera_type="panorama", native_resolution=True)
    with pytest.raises(ValueError, match="sparse-track"):
        _system(sparse_tracks=object()).run(_frames(), camera_type="panorama")
    with pytest.raises(ValueError, match="sparse-track"):
        _system(config=dict(sparse_tracks="klt")).run(_frames(), camera_type="panorama")
    with pytest.raises(ValueError, match="no intrinsics"):
        _system(config=dict(backend=BackendArgs(optimize_intrinsics=True))).run(_frames(), camera_type="panorama")
    with pytest.raises(ValueError, match="depth model"):
        _system(depth_model=object()).run(_frames(), camera_type="panorama")
    with pytest.raises(ValueError, match="all-zero"):
        _system().run(_frames(torch.tensor([100.0, 100.0, 64.0, 32.0])), camera_type="panorama")
    with pytest.raises(ValueError, match="all-zero"):
        _system().run(_frames(torch.zeros(5)), camera_type="panorama")
    with pytest.raises(ValueError, match="unknown camera_type"):
        _system().run(_frames(), camera_type="fisheye")
