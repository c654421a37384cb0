"""The references, inputs and bounds of the direct reprojection / Lie-group tests, proved without a GPU.

oracle/pose_cases.py builds the inputs, oracle/lie_groups.py and oracle/geom.py the float64 references and the bounds
that tests/test_gpu_reproject.py and tests/test_gpu_lie_groups.py hold the kernels to.  Here: the references against
hand-worked numbers and against scipy's matrix exponential; the properties of the inputs that make the GPU tests bite;
a list of wrong formulas that must leave the bound; and the library's HOST path (the same closed forms, libm) over the
Lie sets under half the bound."""

import numpy as np
import pytest
import torch

from oracle import geom, se3
from oracle import lie_groups as lg
from oracle import pose_cases as pc

CASES = [(g, cam) for g in pc.GRIDS for cam in ("pinhole", "mei")]
GROUPS = list(lg.GROUPS)


# ------------------------------------------------------------------------------------------------ hand-worked pins


def test_quarter_turn_about_z_by_hand():
    """phi = (0, 0, pi/2): q = (0, 0, sin 45, cos 45); R maps x -> y, y -> -x; W = [[2/pi, -2/pi, 0], [2/pi, 2/pi, 0], [0, 0, 1]]
    (A = (1 - cos t)/t^2 = 4/pi^2, B = (t - sin t)/t^3, C = 1), so tau = (1, 0, 0) lands at (2/pi, 2/pi, 0)."""
    r = np.sqrt(0.5)
    a = np.array([[1.0, 0, 0, 0, 0, np.pi / 2]])
    X = lg.exp("SE3", a, matrix_exponential=False)
    assert np.allclose(X, [[2 / np.pi, 2 / np.pi, 0, 0, 0, r, r]], atol=1e-15)
    q = X[:, 3:]
    assert np.allclose(se3.so3_adj(q, np.array([[1.0, 2, 3]])), [[-2, 1, 3]], atol=1e-15)
    assert np.allclose(se3.so3_adjT(q, np.array([[1.0, 2, 3]])), [[2, -1, 3]], atol=1e-15)
    assert np.allclose(se3.so3_act4(q, np.array([[1.0, 2, 3, 7]])), [[-2, 1, 3, 7]], atol=1e-15)
    M = se3.so3_matrix4(q)[0]
    assert np.allclose(M, [[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], atol=1e-15)
    P = se3.so3_projector(q)[0]  # 1/2 [[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]] and a zero column
    assert np.allclose(P, 0.5 * np.array([[r, r, 0, 0], [-r, r, 0, 0], [0, 0, r, 0], [0, 0, -r, 0]]), atol=1e-15)
    assert np.allclose(lg.log("SE3", X), a, atol=1e-15)
    assert np.allclose(lg.log("SO3", -q), [[0, 0, np.pi / 2]], atol=1e-15)  # -q: f < 0 times v < 0, the same rotation vector
    assert np.allclose(lg.adj("SE3", X, np.array([[0.0, 0, 0, 1, 0, 0]])), [[0, 0, 2 / np.pi, 0, 1, 0]],
                       atol=1e-15)  # [[t]x R e_x, R e_x] with t x e_y = (0, 0, t_x)


def test_pure_scaling_by_hand():
    """sigma = ln 2, no rotation: s = 2, W = (e^sigma - 1)/sigma I = I / ln 2; act doubles and shifts; inv halves."""
    ln2 = np.log(2.0)
    a = np.array([[ln2, 2 * ln2, -ln2, 0, 0, 0, ln2]])
    for mexp in (True, False):
        X = lg.exp("Sim3", a, matrix_exponential=mexp)
        assert np.allclose(X, [[1, 2, -1, 0, 0, 0, 1, 2]], atol=1e-15)
    assert np.allclose(lg.act("Sim3", X, np.array([[1.0, 1, 1]])), [[3, 4, 1]], atol=1e-15)
    assert np.allclose(lg.inv("Sim3", X), [[-0.5, -1, 0.5, 0, 0, 0, 1, 0.5]], atol=1e-15)
    assert np.allclose(lg.log("Sim3", X), a, atol=1e-15)
    assert np.allclose(lg.matrix("RxSO3", np.array([[0, 0, 0, 1.0, 2.0]]))[0], np.diag([2.0, 2, 2, 1]))
    assert np.allclose(lg.adj("Sim3", X, np.array([[0.0, 0, 0, 0, 0, 0, 1]])), [[-1, -2, 1, 0, 0, 0, 1]], atol=1e-15)
    assert np.allclose(lg.projector("Sim3", X)[0, :3, 6], [1, 2, -1]) and lg.projector("Sim3", X)[0, 7, 6] == 2.0


def test_one_pixel_through_a_two_view_mei_rig_by_hand():
    """Pixel (u, v) = (2, 1) of view 0 (fx = fy = 10, cx = 2, cy = 1, k1 = 0.5) -> the optical axis: X0 = (0, 0, 1), d = 0.5.
    Both poses are the identity, rig[0] = identity, rig[1] = a shift by (0.6, 0, 0): T = rig[1]^-1 moves points by (-0.6, 0, 0)
    x d: X1 = (-0.3, 0, 1).  View 1 (fx = fy = 20, cx = 3, cy = 2, k1 = 0.25): r = sqrt(1.09), x = 20 (-0.3) / (1 + 0.25 r) + 3."""
    poses = se3.se3_identity(2, np.float64)
    rig = se3.se3_identity(2, np.float64)
    rig[1, 0] = 0.6
    intr = np.array([[10.0, 10, 2, 1, 0.5], [20.0, 20, 3, 2, 0.25]])
    disps = np.full((4, 3, 4), 0.5)
    z, o = np.zeros(1, np.int64), np.ones(1, np.int64)
    out = geom.reproject(poses, disps, intr, rig, z, o, z, o, 3 * o, model="mei")
    want_x = 20 * -0.3 / (1 + 0.25 * np.sqrt(1.09)) + 3
    assert np.allclose(out["coords"][0, 1, 2], [want_x, 2.0], atol=1e-14) and out["valid"][0, 1, 2] == 1
    m32, m16 = geom.motion_features(np.float32([[[[70.0, -3.0]]]]), np.float32([[[[1.0, 1.0 + 2.0 ** -11]]]]), 1, 1)
    assert m32[0, :, 0, 0].tolist() == [64.0, -3.0, -64.0, 4.0 + 2.0 ** -11]
    assert m16[0, 3, 0, 0] == np.float16(4.0) and m16.dtype == np.float16  # 4 + 2^-11 is below the tie 4 + 2^-9


@pytest.mark.parametrize("group", ["SE3", "RxSO3", "Sim3"])
def test_references_match_the_matrix_exponential(group):
    """exp's matrix is scipy's expm(hat(a)) to 4e-14 of the matrix's size (expm's own accuracy: 1.6e-14 at |a| ~ 3, where
    the library's float64 path and the quadrature agree to 2e-15), log inverts exp, and adj is X hat(v) X^-1 - on the
    1000-row set with all its small angles and scales."""
    import scipy.linalg
    a = pc.tangents(group)
    E = scipy.linalg.expm(lg.hat(group, a))
    X = lg.exp(group, a)
    M = lg.matrix(group, X)
    size = np.abs(E).reshape(len(a), -1).max(1)[:, None, None]
    assert np.all(np.abs(M - E) <= 4e-14 * size)
    if lg.HAS_T[group]:
        Xe = lg.exp(group, a, matrix_exponential=True)
        assert np.all(np.abs(Xe - X) <= 4e-14 * np.maximum(1.0, np.abs(X)))
    back = lg.log(group, X)
    assert np.all(np.abs(back - a) <= 1e-13 * (1 + np.abs(a).max(1, keepdims=True)))
    v = pc.operands(group).a[:50]
    Av = lg.adj(group, X[:50], v)
    for i in range(50):
        assert np.allclose(lg.vee(group, M[i] @ lg.hat(group, v[i]) @ np.linalg.inv(M[i])), Av[i], atol=1e-11)
    w = pc.operands(group).p3[:50]
    assert np.allclose((lg.adjT(group, X[:50], v)[:, :3] * w).sum(-1), (v * lg.adj(group, X[:50], np.pad(w, ((0, 0), (0, lg.K[group] - 3))))).sum(-1), atol=1e-11)


# ------------------------------------------------------------------------------------------------ the reprojection inputs


def test_index_arrays_do_not_alias():
    arrs = {"pi": pc.RP_PI, "qi": pc.RP_QI, "pj": pc.RP_PJ, "qj": pc.RP_QJ, "di": pc.RP_DI}
    names = list(arrs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert not np.array_equal(arrs[a], arrs[b]), (a, b)
    assert (pc.RP_DI != pc.RP_PI * pc.V + pc.RP_QI).sum() >= 5 and (pc.RP_DI != pc.RP_PI).all()
    assert (pc.RP_QI != pc.RP_QJ).sum() >= 3 and (pc.RP_QI == pc.RP_QJ).sum() >= 2
    assert pc.RP_PI[pc.RP_SELF] == pc.RP_PJ[pc.RP_SELF] and pc.RP_QI[pc.RP_SELF] != pc.RP_QJ[pc.RP_SELF]
    assert len(pc.RP_PI) >= 7 and pc.RP_DI.max() < 2 * 8 and set(pc.FACTOR.values()) == {8.0, 5.0}
    c = pc.reproject_case(9, 29, "mei")
    ident = se3.se3_identity(1)[0]
    assert all(np.abs(row - ident).max() > 0.01 for row in c.rig)
    assert c.intr.shape == (2, 5) and c.intr[0, 4] != c.intr[1, 4] and 0.02 < c.intr[1, 0] / c.intr[0, 0] - 1 < 0.05
    assert pc.reproject_case(9, 29, "pinhole").intr.shape == (2, 4)


@pytest.mark.parametrize("grid,cam", CASES)
def test_depth_branches_margin_share_and_float32_within_a_quarter(grid, cam):
    """Both depth branches occur in the partial term, one term is entirely behind, at most 0.5 % of the pixels are left
    out, `valid` of the float32 and float64 runs agree on the kept ones, and the float32 run of the oracle stays within a
    quarter of the bound at every kept pixel.  On terms without a pixel behind the camera the bound is at most the
    2e-5 max|ref| of the existing tests."""
    c, r = pc.reproject_case(*grid, cam), pc.reproject_reference(*grid, cam)
    behind = (r.Z < geom.MIN_DEPTH).reshape(c.M, -1)
    assert 0.05 < behind[pc.RP_PARTIAL].mean() < 0.5 and behind[pc.RP_FAR].all()
    assert not behind[[0, 1, 2, 3, 6, 7]].any() and r.clean.sum() == 6
    assert (~r.keep).mean() <= pc.CAP
    o32 = pc.reproject_oracle(c, np.float32)
    assert np.array_equal(o32["valid"][r.keep], r.valid[r.keep]) and 0 < r.valid.mean() < 1
    frac = (np.abs(o32["coords"].astype(np.float64) - r.coords) / r.bound)[r.keep].max()
    print("float32 oracle / bound", grid, cam, frac)
    assert frac <= 0.25
    old = 2e-5 * np.abs(r.coords).reshape(c.M, -1).max(1)
    assert np.all(r.bound.reshape(c.M, -1).max(1)[r.clean] <= old[r.clean])


@pytest.mark.parametrize("grid,cam", CASES)
def test_motion_targets_reach_both_clamps_both_signs_and_ties(grid, cam):
    """Channels 2 / 3 (target - coords) hold +64, -64, both signs unclamped and exact fp16 ties on every case.  Channels
    0 / 1 (coords - grid) get +-64 from terms 4 and 5 wherever the camera can put a point 64 px outside the grid: always
    for the pinhole; for MEI |x - cx| < fx / k1, which is below 64 on all grids but (41, 73)."""
    c = pc.reproject_case(*grid, cam)
    c32 = pc.reproject_oracle(c, np.float32)["coords"]
    m32, m16 = geom.motion_features(c32, pc.motion_target(*grid, cam), *grid)
    assert m32.shape == (c.M, 4, *grid) and np.abs(m32).max() == 64.0
    for ch in range(4):
        v = m32[:, ch]
        if ch in pc.clamp_channels(grid, cam):
            assert (v == 64).sum() >= 4 and (v == -64).sum() >= 4, (ch, (v == 64).sum(), (v == -64).sum())
        assert ((v > 0) & (v < 64)).sum() >= 4 and ((v < 0) & (v > -64)).sum() >= 4
    ties = pc.count_fp16_ties(m32)
    assert ties[2] >= 8 and ties[3] >= 8, ties
    assert pc.clamp_channels((5, 7), "pinhole") == (0, 1, 2, 3) and pc.clamp_channels((41, 73), "mei") == (0, 1, 2, 3)


def _candidates(c, r):
    """the reference with one formula wrong -> coords (and, where named, something else)"""
    V = pc.V
    sw = lambda **k: pc.reproject_oracle(c, **k)["coords"]
    intr = pc.scaled_intr(c.intr, c.factor)
    out = {"rig order swapped": pc.reproject_oracle(c, rig=c.rig[::-1].copy())["coords"]}  # rig[qi] <-> rig[qj]
    out["intrinsics of qi / qj swapped"] = pc.reproject_oracle(c, intr=intr[::-1].copy())["coords"]
    out["di -> pi V + qi"] = sw(di=c.pi * V + c.qi)
    if c.cam == "mei":
        flat = np.concatenate([intr.ravel(), np.zeros(8)])  # row stride 4 over the 5-column rows
        out["intrinsics stride 4"] = sw(intr=np.stack([flat[0:5], flat[4:9]]))
        k = intr.copy()
        k[:, 4] /= c.factor
        out["k1 scaled by intr_factor"] = sw(intr=k)
    return out


@pytest.mark.parametrize("grid,cam", CASES)
def test_wrong_formulas_leave_the_bound(grid, cam):
    """Each candidate, applied to the float64 reference, is off by more than 100 bounds at some kept pixel of a term with
    nothing behind the camera (1e3 x the float32 run's own distance, which is held to a quarter)."""
    c, r = pc.reproject_case(*grid, cam), pc.reproject_reference(*grid, cam)
    keep = r.keep & r.clean[:, None, None]
    for name, coords in _candidates(c, r).items():
        frac = np.nan_to_num(np.abs(coords - r.coords) / r.bound, nan=np.inf)[keep].max()  # NaN: not even a number
        print(grid, cam, name, "off by", frac, "bounds")
        assert frac > 100, name
    # the feature-level candidates, on the float32 features
    c32 = pc.reproject_oracle(c, np.float32)["coords"]
    tgt = pc.motion_target(*grid, cam)
    m32, m16 = geom.motion_features(c32, tgt, *grid)
    nhwc = np.moveaxis(m16, 1, -1)
    assert not np.array_equal(nhwc, nhwc[..., ::-1]) and not np.array_equal(nhwc, np.moveaxis(m16[:, [2, 3, 0, 1]], 1, -1))
    u, v = geom.pixel_grid(*grid, np.float32)
    raw = np.moveaxis(np.concatenate([c32 - np.stack([u, v], -1), tgt - c32], -1), -1, 1)
    assert (np.abs(raw) > 64).sum() >= 8 and not np.array_equal(raw, m32)  # the clamp omitted
    Zc = np.where(r.Z < geom.MIN_DEPTH, 1.0, r.Z)
    wrong_valid = (Zc > geom.MIN_DEPTH).astype(np.float64)  # `valid` from the clamped Z: 1 everywhere
    assert (wrong_valid != r.valid)[r.keep].sum() >= grid[0] * grid[1]


# ------------------------------------------------------------------------------------------------ the Lie inputs


@pytest.mark.parametrize("group", GROUPS)
def test_every_branch_is_reached_in_both_precisions(group):
    need = 8
    for dt in (np.float32, np.float64):
        cen = pc.branch_census(group, dt)
        print(group, np.dtype(dt).name, cen)
        assert all(n >= need for n in cen.values()), (dt, cen)
    a = pc.tangents(group)
    theta = np.linalg.norm(lg.split_tangent(group, a)[1], axis=-1)
    assert theta.min() < 2e-9 and theta.max() > 3.0 and theta.max() < np.pi
    assert ((theta > 0.5e-6) & (theta < 1e-6)).sum() >= 90 and ((theta > 1e-6) & (theta < 1.5e-6)).sum() >= 90
    for lo in (1e-5, 1e-4, 1e-3):
        assert ((theta >= lo) & (theta < 10 * lo)).sum() >= 60  # every decade of the float32 cancellation zone
    X = pc.elements(group)
    o = 3 if lg.HAS_T[group] else 0
    nq = np.linalg.norm(X[:, o:o + 4], axis=-1)
    assert (np.abs(nq[pc.ROWS_UNNORM] - 1) > 0.01).sum() >= 24 and np.abs(np.delete(nq, np.r_[pc.ROWS_UNNORM]) - 1).max() < 1e-12


def test_big_set_needs_the_second_trip():
    b = pc.big_set()
    assert b.X.shape == (pc.BIG_ROWS, 7) and pc.BIG_ROWS == 2048 * 256 + 257 > 2048 * 256
    for a in (b.X, b.p, b.grad):
        assert np.array_equal(a[pc.BIG_HEAD:], a[:pc.BIG_TAIL]) and a.dtype == np.float32
    assert len(b.sample) == 4096 and (b.sample >= pc.BIG_HEAD).sum() == pc.BIG_TAIL and (b.sample < 1000).sum() >= 4
    assert b.X.nbytes < 16e6


# ------------------------------------------------------------------------------------------------ the host path


def _host_ops(group, dt):
    """op -> (library result on the host, float64 reference, the inputs for the bound)"""
    from vipe_amd.ext import lietorch_ext as B
    gid = lg.GROUPS[group]
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    o = pc.operands(group)
    a, X, Y, av, p3, p4 = (z.astype(dt) for z in (pc.tangents(group), pc.elements(group), o.Y, o.a, o.p3, o.p4))
    d = lambda z: z.astype(np.float64)
    n = len(a)
    return {
        "exp": (B.expm(gid, T(a)), lg.exp(group, d(a)), (d(a), None)),
        "log": (B.logm(gid, T(X)), lg.log(group, d(X)), (d(X), None)),
        "inv": (B.inv(gid, T(X)), lg.inv(group, d(X)), (d(X), None)),
        "mul": (B.mul(gid, T(X), T(Y)), lg.mul(group, d(X), d(Y)), (d(X), d(Y))),
        "adj": (B.adj(gid, T(X), T(av)), lg.adj(group, d(X), d(av)), (d(X), d(av))),
        "adjT": (B.adjT(gid, T(X), T(av)), lg.adjT(group, d(X), d(av)), (d(X), d(av))),
        "act": (B.act(gid, T(X), T(p3)), lg.act(group, d(X), d(p3)), (d(X), d(p3))),
        "act4": (B.act4(gid, T(X), T(p4)), lg.act4(group, d(X), d(p4)), (d(X), d(p4))),
        "matrix": (B.as_matrix(gid, T(X)).reshape(n, -1), lg.matrix(group, d(X)).reshape(n, -1), (d(X), None)),
        "vec": (B.projector(gid, T(X)).reshape(n, -1), lg.projector(group, d(X)).reshape(n, -1), (d(X), None)),
        "Jinv": (B.Jinv(gid, T(X), T(av)), lg.jinv(group, d(X), d(av)), (d(X), d(av))),
    }


def error_fractions(got, ref, bd):
    """|got - ref| / bound, [n, C]; a zero bound admits only a zero error"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bd = np.broadcast_to(bd if bd.ndim == 2 else bd[:, None], err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bd)


@pytest.mark.parametrize("dt", [np.float32, np.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("group", GROUPS)
def test_host_path_within_half_the_bound(group, dt):
    """the library's host loop (`dev = 0`: the kernels' closed forms, libm's functions) on the 1000-row sets: every
    element of every op within the host share of the bound (oracle/lie_groups.py: half of every rounding and cancellation
    term; the branch approximations and the lost c1 term whole)"""
    worst = {}
    for op, (got, ref, args) in _host_ops(group, dt).items():
        assert got.shape == ref.shape and np.isfinite(got.numpy()).all(), op
        worst[op] = float(error_fractions(got.numpy(), ref, lg.bound(group, op, dt, *args, share=lg.HOST)).max())
    print(group, np.dtype(dt).name, {k: round(v, 3) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


def test_cancellation_zone_of_float32_exp_is_what_the_bound_says():
    """SE3.exp in float32 on the host, rows 600-899 (angles 1e-5 .. 1e-2): the translation is off by far more than the
    2e-5 the older tests use - up to ~1e-4 |tau| - and every row stays within the c1 term + base.  Prints the largest
    fraction of the DEVICE bound per angle decade (recorded in DESIGN.md)."""
    from vipe_amd.ext import lietorch_ext as B
    for group in ("SE3", "Sim3"):
        a = pc.tangents(group).astype(np.float32)
        got = B.expm(lg.GROUPS[group], torch.from_numpy(a)).numpy()
        a64 = a.astype(np.float64)
        ref = lg.exp(group, a64)
        tau, phi, _ = lg.split_tangent(group, a64)
        theta = np.linalg.norm(phi, axis=-1)
        err = np.abs(got - ref)[:, :3].max(1)
        fr = error_fractions(got, ref, lg.bound(group, "exp", np.float32, a64))[:, :3].max(1)
        zone = slice(600, 900)
        if group == "SE3":  # Sim3 rows with sigma = O(1) take the general branch of calcW, which does not cancel here
            assert (err[zone] / np.linalg.norm(tau, axis=-1)[zone]).max() > 2e-5  # the old tolerance would fail here
        for lo in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2):
            m = (theta >= lo) & (theta < 10 * lo)
            print(group, "float32 exp, host, angle decade %.0e: worst error / device bound %.3f, worst |dt| / |tau| %.2e"
                  % (lo, fr[m].max(), (err[m] / np.linalg.norm(tau, axis=-1)[m]).max()))
        assert fr.max() <= 1.0
