"""The 360-degree panorama camera on the device against the float64 references of tests/panorama_reference.py (whose own
correctness, and the fairness of the cases, tests/test_panorama_reference.py establishes on the CPU): reprojection in its
three output layouts, the dense BA in every accumulate form, the seam case, marginals, frame distance, depth filter,
back-projection, a whole `SLAMSystem.run`, and the bits of the pinhole / MEI instantiations against the parent commit's."""
import os

import numpy as np
import pytest
import torch

import panorama_reference as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHARE_CAP = 0.005
EPS32 = float(np.finfo(np.float32).eps)
REPROJECT_CASES = ["g8x16_n5", "g12x24_n4", "g8x16_rig2"]


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev())


def term_args(g):
    return T(g.pi), T(g.qi), T(g.pj), T(g.qj), T(g.di)


# ---------------------------------------------------------------------------------------------- reprojection

_CONST = {}


def reproject_constant():
    """The constant of the per-pixel bound `constant x R.reproject_error_unit`: four times what a float32 NumPy restatement
    of the same formulas needs against float64 over the test's cases (the margin for the device's atan2f / sincosf and
    operation order).  Computed on the CPU; the device's output has no part in it."""
    if "k" not in _CONST:
        worst = 0.0
        for name in REPROJECT_CASES:
            g, _, _ = R.case(name)
            a = (g.pi, g.pj, g.qi, g.qj, g.di)
            r64 = R.reproject(g.poses, g.disps, g.rig, *a)
            r32 = R.reproject(g.poses, g.disps, g.rig, *a, dtype=np.float32)
            unit = R.reproject_error_unit(r64, g.poses, g.rig, g.disps, g.pi, g.pj, g.qi, g.qj, g.di, g.wd)
            keep = r64["valid"] & ~R.fairness_margins(r64["X1"])
            assert np.array_equal(r32["valid"][keep], r64["valid"][keep])
            d = r32["coords"].astype(np.float64) - r64["coords"]
            d[..., 0] = R.wrap(d[..., 0], g.wd)
            worst = max(worst, float((np.abs(d) / unit)[keep].max()))
        _CONST["k"] = 4.0 * worst
        print(f"float32 NumPy restatement needs {worst:.2f} units; the device is held to {4 * worst:.2f}")
    return _CONST["k"]


@pytest.mark.parametrize("name", REPROJECT_CASES)
def test_reproject_in_all_three_layouts(name):
    from vipe_amd.ext import slam_ext
    g, _, _ = R.case(name)
    ref = R.reproject(g.poses, g.disps, g.rig, g.pi, g.pj, g.qi, g.qj, g.di)
    unit = R.reproject_error_unit(ref, g.poses, g.rig, g.disps, g.pi, g.pj, g.qi, g.qj, g.di, g.wd)
    bound = reproject_constant() * unit
    margin = R.fairness_margins(ref["X1"])
    assert margin.mean() <= SHARE_CAP
    keep = ~margin
    state = (T(g.poses), T(g.disps), T(g.intrinsics), T(g.rig)) + term_args(g)
    coords, valid = slam_ext.reproject(*state, camera="panorama")
    coords, valid = coords.cpu().numpy(), valid.cpu().numpy()[..., 0]
    assert np.isfinite(coords).all()
    assert np.array_equal(valid[keep] > 0, ref["valid"][keep]) and set(np.unique(valid)) <= {0.0, 1.0}
    assert (valid == 0).any() and (valid == 1).any()
    _, u, v = R.rays(g.ht, g.wd, np.float32)
    bad = valid == 0
    assert np.array_equal(coords[bad], np.broadcast_to(np.stack([u, v], -1), coords.shape)[bad])  # an invalid pixel keeps its place
    assert coords[..., 0].min() >= -0.5 and coords[..., 0].max() < g.wd - 0.5  # the principal value
    d = coords.astype(np.float64) - ref["coords"]
    d[..., 0] = R.wrap(d[..., 0], g.wd)  # modulo wd
    ok = keep & ref["valid"]
    ratio = float((np.abs(d) / bound)[ok].max())
    print(f"{name}: coordinates at most {ratio:.3f} of the bound ({reproject_constant():.1f} units), "
          f"largest error {np.abs(d)[ok].max():.2e} px")
    assert ratio <= 1.0
    # the motion features: horizontal differences wrapped, compared modulo wd on the x channels
    want = R.motion_features(ref["coords"], g.target.astype(np.float64), g.ht, g.wd)  # [M,4,ht,wd]
    mb = np.stack([bound[..., 0], bound[..., 1], bound[..., 0], bound[..., 1]], 1) + EPS32 * (np.abs(want) + 1)
    okc = np.broadcast_to(ok[:, None], want.shape)
    tgt = T(g.target)
    c16, m16 = slam_ext.reproject_motion(*state, tgt, camera="panorama")
    c32, m32 = slam_ext.reproject_motion(*state, tgt, camera="panorama", motn_dtype=torch.float32)
    cnh, mnh = slam_ext.reproject_motion_nhwc(*state, tgt, camera="panorama")
    for c in (c16, c32, cnh):
        assert np.array_equal(c.cpu().numpy().view(np.uint32), coords.view(np.uint32))
    for tag, m, half in (("f32", m32, 0.0), ("f16", m16, 2.0 ** -11), ("nhwc f16", mnh.permute(0, 3, 1, 2), 2.0 ** -11)):
        got = m.float().cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all() and np.abs(got).max() <= 64
        dm = got - want
        dm[:, 0], dm[:, 2] = R.wrap(dm[:, 0], g.wd), R.wrap(dm[:, 2], g.wd)
        r = float((np.abs(dm) / (mb + half * (np.abs(want) + g.wd)))[okc].max())
        print(f"{name}: motion features {tag} at most {r:.3f} of the bound")
        assert r <= 1.0
        assert np.abs(got[:, [0, 2]])[okc[:, [0, 2]]].max() <= g.wd / 2 + 1e-3  # wrapped into [-wd/2, wd/2)


# ---------------------------------------------------------------------------------------------- dense BA

def run_ba(g, kw, n_iters, opts=0, t1=None):
    from vipe_amd.ext import slam_ext
    M = len(g.pi)
    poses, disps, rig, intr = T(g.poses).clone(), T(g.disps).clone(), T(g.rig).clone(), T(g.intrinsics).clone()
    info = slam_ext.dense_ba(poses, disps, T(g.disps_sens), intr, rig, T(g.target.reshape(M, -1, 2)),
                             T(g.weight.reshape(M, -1, 2)), T(g.eta), *term_args(g), t0=1, t1=g.n if t1 is None else t1,
                             n_iters=n_iters, camera="panorama", want_info=True, solver_options=opts, **kw)
    torch.cuda.synchronize()
    assert int(info[2]) == 0, "Cholesky must not fail"
    assert not intr.any()  # the row is never touched
    return poses.cpu().numpy(), disps.cpu().numpy(), rig.cpu().numpy()


def close_1e4(got, ref, what):
    """the project's 1e-4 form (tests/test_gpu_ba_edges.py:97-100)"""
    (p, d, r), (rp, rd, rr) = got, ref
    ep, ed, er = np.abs(p - rp).max(), np.abs(d - rd).max(), np.abs(r - rr).max()
    print(f"{what}: poses {ep:.2e} (of {1e-4 * max(1.0, np.abs(rp).max()):.1e}), disparities {ed:.2e} "
          f"(of {1e-4 * np.abs(rd).max():.1e}), rig {er:.2e} (of 1e-4)")
    assert ep <= 1e-4 * max(1.0, np.abs(rp).max()), what
    assert ed <= 1e-4 * np.abs(rd).max(), what
    assert er <= 1e-4, what


MONO = ["g8x16_n5", "g12x24_n4", "g8x16_motion_only", "g12x24_depth_prior"]
RIGS = ["g8x16_rig2", "g12x24_rig2"]


@pytest.mark.parametrize("name", MONO + RIGS)
def test_dense_ba_against_the_reference_solver(name):
    """after 1, 2 and 4 Gauss-Newton iterations, in every accumulate form the graph can take: the fused matrix-core kernel
    and the general walk + Schur pair for one view (they must also agree with each other), the rig walk with the rig
    rotations free for two"""
    from vipe_amd.ext import slam_ext
    g, kw, hist = R.case(name)
    forms = {"rig": 0} if name in RIGS else {"fused": 0, "general": slam_ext.BA_OPT_GENERAL_ACCUMULATE}
    for n_iters in (1, 2, 4):
        h = hist[n_iters - 1]
        ref = (h["poses"], h["disps"], h["rig"])
        got = {}
        for tag, opts in forms.items():
            got[tag] = run_ba(g, kw, n_iters, opts)
            close_1e4(got[tag], ref, f"{name} [{tag}] {n_iters} iterations")
        if len(got) == 2:
            close_1e4(got["fused"], got["general"], f"{name} fused against general, {n_iters} iterations")
    e0, e4 = R.pose_error(g.poses, g.poses_gt), R.pose_error(got[next(iter(forms))][0], g.poses_gt)
    print(f"{name}: pose error to the ground truth {e0:.2e} -> {e4:.2e}")
    assert e4 < e0
    if kw.get("motion_only"):
        assert np.array_equal(got["fused"][1], np.maximum(g.disps, 1e-3))
    if name in RIGS:
        assert np.abs(got["rig"][2] - g.rig).max() > 1e-4  # the rig rotations moved ...
        # ... and only they: view 0 is the gauge, and X <- Exp([0, phi]) X turns a baseline without changing its length
        assert np.array_equal(got["rig"][2][0], g.rig[0])
        assert np.abs(np.linalg.norm(got["rig"][2][:, :3], axis=-1) - np.linalg.norm(g.rig[:, :3], axis=-1)).max() < 1e-6


def test_seam_case_converges():
    """two keyframes half a turn apart, every flow across the seam (that the case discriminates - the same solver without
    the wrap diverges - is the CPU test's assertion)"""
    g = R.seam_case()
    kw = dict(pose_damping=1e-3, pose_ep=0.1, motion_only=True)
    ref = R.gauss_newton(R.panorama_camera(), g.poses, g.disps, g.disps_sens, g.rig, g.target, g.weight, g.eta, g.pi, g.qi,
                         g.pj, g.qj, g.di, t0=1, t1=2, n_iters=4, **kw)
    got = run_ba(g, kw, 4)
    close_1e4(got, (ref[-1]["poses"], ref[-1]["disps"], ref[-1]["rig"]), "seam case")
    e0, e4 = R.pose_error(g.poses, g.poses_gt), R.pose_error(got[0], g.poses_gt)
    print(f"seam case: pose error {e0:.2e} -> {e4:.2e}")
    assert e4 < 0.3 * e0


def test_linearize_and_marginals():
    from vipe_amd.ext import slam_ext
    g, kw, _ = R.case("g8x16_n5")
    M = len(g.pi)
    args = (T(g.poses), T(g.disps), T(g.disps_sens), T(g.intrinsics), T(g.rig), T(g.target.reshape(M, -1, 2)),
            T(g.weight.reshape(M, -1, 2)), T(g.eta)) + term_args(g)
    S, info, _ = slam_ext.dense_ba_linearize(*args, 1, g.n, camera="panorama", **kw)
    S = S.cpu().numpy()
    assert S.shape == (6 * (g.n - 1),) * 2 and np.isfinite(S).all() and np.array_equal(S, S.T)
    assert np.linalg.eigvalsh(S).min() > 0
    disp_var, pose_cov, _ = slam_ext.dense_ba_marginals(*args, 1, g.n, camera="panorama", **kw)
    disp_var, pose_cov = disp_var.cpu().numpy(), pose_cov.cpu().numpy()
    assert np.isfinite(disp_var).all() and (disp_var > 0).all()
    assert np.isnan(pose_cov[0]).all() and np.isfinite(pose_cov[1:]).all()  # keyframe 0 is the gauge
    for c in pose_cov[1:]:
        assert np.abs(c - c.T).max() <= 1e-12 * np.abs(c).max() and np.linalg.eigvalsh(0.5 * (c + c.T)).min() > 0


# ---------------------------------------------------------------------------------------------- frame operations

@pytest.mark.parametrize("name", ["g8x16_n5", "g12x24_rig2"])
@pytest.mark.parametrize("bidirectional", [True, False])
def test_frame_distance(name, bidirectional):
    """against float64, with a candidate that returns 1000: a third of one frame's disparities are NaN (an unusable frame),
    so fewer than 75 % of its pixels are valid"""
    from vipe_amd.ext import slam_ext
    g, _, _ = R.case(name)
    V, n = g.V, g.n
    disps = g.disps.copy()
    broken = (n - 1) * V
    disps[broken].reshape(-1)[::3] = np.nan
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    pi = np.repeat(np.array([p[0] for p in pairs], np.int64), V)
    pj = np.repeat(np.array([p[1] for p in pairs], np.int64), V)
    qi = np.tile(np.arange(V, dtype=np.int64), len(pairs))
    qj = (qi + (1 if V > 1 else 0)) % V
    beta = 0.3
    ref, shares = R.frame_distance(g.poses, g.rig, disps, pi, qi, pj, qj, beta, bidirectional)
    got = slam_ext.frame_distance_rig(T(g.poses), T(g.rig), T(disps), T(g.intrinsics), T(pi), T(qi), T(pj), T(qj), beta,
                                      bidirectional, camera="panorama").cpu().numpy()
    assert np.isfinite(got).all()
    far = ref >= 500
    assert far.any() and (~far).any()
    assert np.abs(shares - 0.75).min() > 1e-3  # no candidate near the 75 % decision
    assert np.array_equal(got >= 500, far)
    # a distance is a weighted mean of flow lengths: each within sqrt(2) of the reprojection bound (its largest value over
    # the frame is taken, for both flows), plus the float32 summation of P terms
    P = g.ht * g.wd
    worst = 0.0
    for m in np.flatnonzero(~far):
        dirs = [(pi[m], qi[m], pj[m], qj[m])] + ([(pj[m], qj[m], pi[m], qi[m])] if bidirectional else [])
        tol = 0.0
        for a, qa, b2, qb in dirs:
            idx = (np.array([a]), np.array([b2]), np.array([qa]), np.array([qb]), np.array([a * V + qa]))
            out = R.reproject(g.poses, disps, g.rig, *idx)
            unit = R.reproject_error_unit(out, g.poses, g.rig, disps, *idx, g.wd)
            tol += np.sqrt(2) * reproject_constant() * float(np.nanmax(np.where(out["valid"][..., None], unit, 0.0)))
        tol = tol / len(dirs) + P * EPS32 * ref[m]
        worst = max(worst, abs(got[m] - ref[m]) / tol)
    print(f"{name} bidirectional={bidirectional}: distances at most {worst:.3f} of the bound; "
          f"{int(far.sum())} of {len(ref)} candidates at 1000")
    assert worst <= 1.0
    assert np.allclose(got[far], ref[far], rtol=1e-4)


def test_depth_filter_sphere():
    from vipe_amd.ext import slam_ext
    g, thresh = R.depth_filter_case()
    want, tie = R.depth_filter(g.poses_gt, g.disps_gt, np.arange(g.n), thresh)
    assert tie.mean() < SHARE_CAP
    got = slam_ext.depth_filter(T(g.poses_gt), T(g.disps_gt), None, T(np.arange(g.n)), T(thresh.astype(np.float32)),
                                camera="panorama")
    got = got.cpu().numpy()
    print(f"depth filter: counts {np.bincount(got.astype(int).ravel())}, {int(tie.sum())} pixels excluded as ties, "
          f"{int((got != want)[tie].sum())} of them differ")
    assert np.array_equal(got[~tie], want[~tie])
    assert (want >= 2).mean() > 0.5 and (want == 0).any()


@pytest.mark.parametrize("name", ["g8x16_n5", "g12x24_n4"])
def test_iproj_sphere(name):
    from vipe_amd.ext import slam_ext
    from oracle import se3
    g, _, _ = R.case(name)
    c2w = se3.se3_inv(g.poses.astype(np.float64)).astype(np.float32)
    want = R.iproj(c2w, g.disps)
    got = slam_ext.iproj(T(c2w), T(g.disps), None, camera="panorama").cpu().numpy()
    # float32 rounding: the ray, the rotation and the sum are known to a few eps of |b| + |t| d, then divided by d
    scale = (1.0 + np.linalg.norm(c2w[:, :3], axis=-1)[:, None, None] * g.disps) / g.disps
    ratio = float((np.abs(got - want).max(-1) / (EPS32 * scale)).max())
    print(f"{name}: back-projected points within {ratio:.2f} eps32 (|b| + |t| d) / d")
    assert ratio <= 8.0
    # the points of the ground truth lie on one surface: the scene of the synthetic clip
    from vipe_amd.synth import _scene_range
    pts = R.iproj(se3.se3_inv(g.poses_gt.astype(np.float64)), g.disps_gt)
    dev_ = np.abs(np.linalg.norm(pts, axis=-1) - _scene_range(pts))
    assert np.median(dev_) < 1e-4


# ---------------------------------------------------------------------------------------------- the whole system

def test_slam_system_runs_a_panorama_clip():
    """an 8-frame 128 x 256 equirectangular clip through `SLAMSystem.run` with the default network"""
    import klt_reference as K
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.inner_filler import InfillArgs
    from vipe_amd.slam.system import Frame, SLAMConfig, SLAMSystem
    frames, _ = K.make_sequence(8, 128, 256)
    frames = [Frame(rgb=torch.from_numpy(f).to(dev()), intrinsics=torch.zeros(4)) for f in frames]
    cfg = SLAMConfig(buffer=48, filter_thresh=0.0, frontend_backend_iters=(), frontend=FrontendArgs(keyframe_thresh=0.0),
                     infill=InfillArgs(infill_chunk_size=8))
    torch.manual_seed(0)
    sysm = SLAMSystem(dev(), cfg)
    out = sysm.run(frames, camera_type="panorama")
    torch.cuda.synchronize()
    assert sysm.buffer.camera_type == "panorama"
    assert out.trajectory.data.shape == (8, 7) and bool(torch.isfinite(out.trajectory.data).all())
    assert not out.intrinsics.any()
    m = out.slam_map
    xyz = m.dense_disp_xyz
    assert xyz.shape[0] > 0 and bool(torch.isfinite(xyz).all())
    ids = [int(t) for t in out.keyframe_ids]
    assert ids == sorted(set(ids)) and set(ids) <= set(range(8)) and len(ids) == sysm.n_keyframes
    assert tuple(m.dense_disp_packinfo.shape) == (len(ids), 1, 2) and int(m.dense_disp_packinfo[:, :, 1].sum()) == xyz.shape[0]


# ---------------------------------------------------------------------------------------------- the other two cameras

@pytest.mark.parametrize("camera", ["pinhole", "mei"])
def test_pinhole_mei_bits_unchanged(camera):
    """tests/golden/panorama_parent_bits.npz holds what the parent commit's build computed on the device for one small graph
    (tests/golden/make_golden_panorama_parent.py).  The reprojection kernels are per-pixel arithmetic: same bits.  The BA
    sums through floating-point atomics and did not repeat its own bits on the parent (`ba_*_repeatable` is False there):
    it is held to the 1e-4 form instead."""
    import sys
    sys.path.insert(0, GOLD)
    import make_golden_panorama_parent as mk
    Z = np.load(os.path.join(GOLD, "panorama_parent_bits.npz"))
    got = mk.run_case(camera)
    for key in ("coords", "valid", "motn_f32", "coords_motion"):
        assert np.array_equal(got[key].view(np.uint32), Z[f"{camera}_{key}"].view(np.uint32)), key
    for key in ("motn_f16", "motn_nhwc"):
        assert np.array_equal(got[key], Z[f"{camera}_{key}"]), key
    for form in ("fused", "general"):
        p, d = got[f"ba_{form}_poses"], got[f"ba_{form}_disps"]
        rp, rd = Z[f"{camera}_ba_{form}_poses"], Z[f"{camera}_ba_{form}_disps"]
        if bool(Z[f"{camera}_ba_{form}_repeatable"]):
            assert np.array_equal(p.view(np.uint32), rp.view(np.uint32)) and np.array_equal(d.view(np.uint32), rd.view(np.uint32))
        assert np.abs(p - rp).max() <= 1e-4 * max(1.0, np.abs(rp).max()) and np.abs(d - rd).max() <= 1e-4 * np.abs(rd).max()
        print(f"{camera} BA [{form}]: poses {np.abs(p - rp).max():.1e}, disparities {np.abs(d - rd).max():.1e} from the parent's")
