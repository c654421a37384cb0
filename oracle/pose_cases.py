"""Inputs, float64 references and bounds for the direct tests of `reproject.hip` and `lie.hip`.

ORACLE (test infrastructure).  One place builds them, so that the CPU test that proves the inputs and the references
(tests/test_oracle_pose.py) and the GPU tests that feed them to the kernels (tests/test_gpu_reproject.py,
tests/test_gpu_lie_groups.py) look at the same numbers.  Everything is seeded and cached; nothing is modified after it
is built.
"""

import functools
from types import SimpleNamespace

import numpy as np

from . import frame_cases as fc
from . import geom, se3
from . import lie_groups as lg

GRIDS = fc.GRIDS
U32 = 2.0 ** -24

# ------------------------------------------------------------------------------------------------ reprojection
# Eight terms over 8 frames x 2 views.  Five index arrays that do not alias: the disparity map of a term is NOT the one
# of its source view (di != pi V + qi) except in terms 1, 5 and 7; source and target view differ in terms 1, 2, 4, 5, 6, 7.
# Term 4 looks at frame 6 (pushed back and far to the side: part of its pixels fall behind MIN_DEPTH, the rest land far
# outside the image), term 5 at frame 7 (100 units behind every source), term 7 is the self pair of keyframe 3's two views.
RP_PI = np.array([0, 1, 2, 5, 3, 4, 2, 3], dtype=np.int64)
RP_PJ = np.array([1, 0, 5, 2, 6, 7, 4, 3], dtype=np.int64)
RP_QI = np.array([0, 1, 0, 1, 1, 0, 1, 0], dtype=np.int64)
RP_QJ = np.array([0, 0, 1, 1, 0, 1, 0, 1], dtype=np.int64)
RP_DI = np.array([5, 3, 9, 2, 12, 8, 14, 6], dtype=np.int64)
RP_PARTIAL, RP_FAR, RP_SELF = 4, 5, 7
V = 2
FACTOR = {(41, 73): 8.0, (9, 29): 5.0, (16, 16): 8.0, (5, 7): 5.0}  # intr_factor: the hot loop's 8, and one that 1/f rounds
MEI_K1 = (0.30, 0.45)
# WAIVER: under MEI a point cannot land further than fx / k1 from the principal point (x - cx = fx X / (Z + k1 r), r >= |X|),
# which is 21 .. 87 grid pixels here, so channels 0 / 1 of the motion features (coords - grid) reach +-64 only on the
# (41, 73) grid; the pinhole cases reach both clamps in every channel on every grid (`clamp_channels`).  A k1 small enough
# to allow 64 px on a 7-pixel grid (< 0.1) would no longer separate the k1 candidates of tests/test_oracle_pose.py.
PARTIAL_T = (-30.0, 30.0, -1.5)
Z_MARGIN = 2e-5  # float32 Z carries ~1e-6 of rounding at these magnitudes (20 u x (|X0| + |Y0| + 1 + |t| d)); 20 x that
CAP = 0.005
# the offsets target - coords cycles through, by pixel index mod 8: both clamps, both signs unclamped, and four exact ties
# of the fp16 rounding (spacing 2^-10 in [1, 2), 2^-9 in [2, 4): odd multiples of half of it)
TIE_OFFSETS = (1.0 + 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 2.0 + 2.0 ** -10, -(3.0 + 3 * 2.0 ** -10))
OFFSETS = (100.0, -100.0, 7.3, -11.9) + TIE_OFFSETS


@functools.lru_cache(maxsize=None)
def reproject_case(ht, wd, cam):
    """everything `vipe_reproject*` reads, float32, on a (ht, wd) grid: 8 poses, 16 disparity maps, a two-view rig with no
    identity row, two intrinsics rows (full resolution = intr_factor x grid; MEI: 5 columns, two k1)"""
    g = fc.geom_case(ht, wd)
    c = SimpleNamespace(ht=ht, wd=wd, cam=cam, M=len(RP_PI), factor=FACTOR[(ht, wd)])
    c.poses = g.fd_poses.copy()  # frame 6 pushed back, frame 7 at z = -100 (oracle/frame_cases.py)
    c.poses[7, :2] = np.float32([40.0, -40.0])   # Z is replaced by 1 there: x = fx (X0 + 40 d) + cx straddles +64
    c.disps = np.ascontiguousarray(np.stack([g.g.disps, g.g.disps_gt], 1).reshape(2 * fc.N, ht, wd)).astype(np.float32)
    c.rig = se3.se3_exp(np.array([[0.05, -0.02, 0.01, 0.02, -0.03, 0.01],
                                  [0.30, 0.02, -0.01, 0.01, 0.20, -0.02]])).astype(np.float32)
    grid_intr = g.intr.astype(np.float64)  # [4] at grid scale
    rows = np.stack([grid_intr, 1.03 * grid_intr]) * c.factor
    if cam == "mei":
        rows = np.concatenate([rows, np.array(MEI_K1)[:, None]], 1)
    c.intr = rows.astype(np.float32)
    c.pi, c.qi, c.pj, c.qj, c.di = RP_PI, RP_QI, RP_PJ, RP_QJ, RP_DI
    # frame 6 is placed so that term 4's transform has the translation PARTIAL_T exactly (T.t is affine in t_6: T = R_qj^-1
    # G_6 G_pi^-1 R_qi): Z = (R X0)_z - 1.5 d falls below MIN_DEPTH for d > 0.6, a sixth of the pixels, and the 30 units
    # to the side clamp channels 0 / 1 at -64 / +64 on both sides of the depth branch
    p64, rig64 = c.poses.astype(np.float64), c.rig.astype(np.float64)
    p64[6, :3] = 0
    A = se3.se3_inv(rig64[RP_QJ[RP_PARTIAL]])
    rest = se3.se3_mul(se3.se3_inv(p64[RP_PI[RP_PARTIAL]]), rig64[RP_QI[RP_PARTIAL]])
    t0 = se3.se3_mul(se3.se3_mul(A, p64[6]), rest)[:3]
    c.poses[6, :3] = se3.so3_act(se3.so3_inv(A[3:]), np.array(PARTIAL_T) - t0).astype(np.float32)
    return c


def scaled_intr(intr, factor, dtype=np.float64):
    """[fx, fy, cx, cy] / factor, k1 untouched (cameras.py:212-213, :345-348)"""
    out = np.asarray(intr).astype(dtype).copy()
    out[:, :4] = out[:, :4] / dtype(factor)
    return out


def reproject_oracle(c, dtype=np.float64, **swap):
    """`oracle/geom.reproject` on the case; `swap` replaces inputs by name (the wrong-formula candidates of the CPU test)"""
    a = dict(poses=c.poses, disps=c.disps, intr=scaled_intr(c.intr, c.factor, dtype), rig=c.rig, pi=c.pi, pj=c.pj,
             qi=c.qi, qj=c.qj, di=c.di)
    a.update(swap)
    return geom.reproject(a["poses"].astype(dtype), a["disps"].astype(dtype), a["intr"].astype(dtype), a["rig"].astype(dtype),
                          a["pi"], a["pj"], a["qi"], a["qj"], a["di"], model=c.cam)


@functools.lru_cache(maxsize=None)
def reproject_reference(ht, wd, cam):
    """float64 coords / valid / Z of the case, the pixels kept in the comparison, and the per-pixel bound on float32
    coords.

    BOUND, u = 2^-24, from the roundings of the operation (all magnitudes from the float64 run):
      iproj    e0 = 4 u (|X0| + |cx| / fx): the scaling of the intrinsics row, one subtraction, one division.  MEI: X0 = ub h(r2)
               with h = factor / (factor - k1), whose own roundings are 8 u + 6 u factor / (factor - k1) (r2, the square
               root, two divisions, the difference) and which passes on the error of ub once more: 2 e0 + u |X0| (8 + 6 h).
      T X0     eP = eX0 + eY0 + 20 u (|X0| + |Y0| + 1) + 20 u |t|_sum d: a row of R (entries known to a few u after
               five quaternion products and the conversion) times X0, plus t d, where |t|_sum adds the translations that
               went into T (both poses, both rig rows, T itself).
      proj     x = fx (X / Z) + cx: fx eP (1 + |X / Z|) / Z + 6 u (|fx X / Z| + |cx|), Z the clamped depth: grows with
               1 / Z next to the clamp.  MEI: Z -> rb = Z + k1 r with e_rb = (1 + 2 k1) eP + 4 u rb.
    tests/test_oracle_pose.py holds the float32 run of the oracle to a QUARTER of it; the kernel gets the whole: it
    composes T through quaternions and a rotation matrix in another order than numpy does.  On terms with no pixel behind
    the camera the bound is cut to the 2e-5 max|ref| the suite already holds them to."""
    c = reproject_case(ht, wd, cam)
    o = reproject_oracle(c)
    f8 = np.float64
    intr = scaled_intr(c.intr, c.factor)
    Ii, Ij = intr[c.qi], intr[c.qj]
    X0, _ = geom.iproj_disp(c.disps[c.di].astype(f8), Ii, cam)
    poses, rig = c.poses.astype(f8), c.rig.astype(f8)
    T = se3.se3_mul(se3.se3_mul(se3.se3_inv(rig[c.qj]), se3.se3_mul(poses[c.pj], se3.se3_inv(poses[c.pi]))), rig[c.qi])
    X1 = se3.se3_act4(T[:, None, None, :], X0)
    X, Y, Z, d = X1[..., 0], X1[..., 1], X1[..., 2], X0[..., 3]
    nrm = lambda a: np.linalg.norm(a[:, :3], axis=-1)
    tsum = (nrm(poses[c.pi]) + nrm(poses[c.pj]) + nrm(rig[c.qi]) + nrm(rig[c.qj]) + nrm(T))[:, None, None]
    b = lambda a: a[:, None, None]
    u = U32
    e0x = 4 * u * (np.abs(X0[..., 0]) + b(np.abs(Ii[:, 2]) / Ii[:, 0]))
    e0y = 4 * u * (np.abs(X0[..., 1]) + b(np.abs(Ii[:, 3]) / Ii[:, 1]))
    if cam == "mei":
        k1 = b(Ii[:, 4])
        uu, vv = geom.pixel_grid(ht, wd, f8)
        r2 = ((uu - b(Ii[:, 2])) / b(Ii[:, 0])) ** 2 + ((vv - b(Ii[:, 3])) / b(Ii[:, 1])) ** 2
        factor = (k1 + np.sqrt(1 + (1 - k1 ** 2) * r2)) / (1 + r2)
        amp = u * (8 + 6 * factor / (factor - k1))
        e0x, e0y = 2 * e0x + amp * np.abs(X0[..., 0]), 2 * e0y + amp * np.abs(X0[..., 1])
    eP = (e0x + e0y) + 20 * u * (np.abs(X0[..., 0]) + np.abs(X0[..., 1]) + 1) + 20 * u * tsum * d
    Zc = np.where(Z < geom.MIN_DEPTH, 1.0, Z)
    fx, fy, cx, cy = (b(Ij[:, k]) for k in range(4))
    if cam == "mei":
        k1 = b(Ij[:, 4])
        rb = Zc + k1 * np.sqrt(X ** 2 + Y ** 2 + Zc ** 2)
        e_rb = (1 + 2 * k1) * eP + 4 * u * rb
        bx = fx * (eP / rb + np.abs(X) * e_rb / rb ** 2) + 6 * u * (np.abs(fx * X / rb) + np.abs(cx))
        by = fy * (eP / rb + np.abs(Y) * e_rb / rb ** 2) + 6 * u * (np.abs(fy * Y / rb) + np.abs(cy))
    else:
        bx = fx * eP * (1 + np.abs(X / Zc)) / Zc + 6 * u * (np.abs(fx * X / Zc) + np.abs(cx))
        by = fy * eP * (1 + np.abs(Y / Zc)) / Zc + 6 * u * (np.abs(fy * Y / Zc) + np.abs(cy))
    bound = np.stack([bx, by], -1)
    # never above what the suite already holds such terms to: 2e-5 max|ref| where no pixel of the term is behind the camera
    clean = ~(Z < geom.MIN_DEPTH).reshape(c.M, -1).any(1)
    old = 2e-5 * np.abs(o["coords"]).reshape(c.M, -1).max(1)
    bound = np.where(b(clean)[..., None], np.minimum(bound, b(old)[..., None]), bound)
    r = SimpleNamespace(coords=o["coords"], valid=o["valid"], Z=Z, bound=bound, clean=clean,
                        keep=np.abs(Z - geom.MIN_DEPTH) >= Z_MARGIN)
    return r


def clamp_channels(grid, cam):
    """the channels of the motion features that must hold both +64 and -64 on this case (see the waiver at MEI_K1)"""
    return (0, 1, 2, 3) if cam == "pinhole" or tuple(grid) == (41, 73) else (2, 3)


def target_from(coords32):
    """coords [M,ht,wd,2] float32 + OFFSETS[(pixel index + term) mod 8], channel 1 shifted by three pixels"""
    M, ht, wd, _ = coords32.shape
    k = (np.arange(ht * wd).reshape(1, ht, wd) + np.arange(M).reshape(-1, 1, 1)) % len(OFFSETS)
    off = np.asarray(OFFSETS, dtype=np.float32)[k]
    off = np.stack([off, np.roll(off, 3, axis=2)], -1)
    return (np.asarray(coords32, np.float32) + off).astype(np.float32)


def count_fp16_ties(m32):
    """per channel: how many unclamped float32 features lie exactly half way between two neighbouring halves"""
    v = np.asarray(m32, np.float32)
    h = v.astype(np.float16)
    inf = np.float16(np.inf)
    lo, hi = np.nextafter(h, -inf).astype(np.float64), np.nextafter(h, inf).astype(np.float64)
    v64, h64 = v.astype(np.float64), h.astype(np.float64)
    tie = (np.abs(v64) < 64) & (v64 != h64) & ((v64 == 0.5 * (h64 + lo)) | (v64 == 0.5 * (h64 + hi)))
    return tie.sum(axis=(0, 2, 3))


@functools.lru_cache(maxsize=None)
def motion_target(ht, wd, cam):
    """target [M,ht,wd,2] float32 = the oracle's float32 coordinates + OFFSETS[(pixel index + term) mod 8]: channels 2 / 3
    of the motion features then hold both clamps, both signs and exact fp16 ties (as far as the kernel's coordinates equal
    the oracle's float32 ones; channels 0 / 1 = coords - grid get their clamps from terms 4 and 5)."""
    c = reproject_case(ht, wd, cam)
    c32 = reproject_oracle(c, np.float32)["coords"]
    return target_from(c32)


# ------------------------------------------------------------------------------------------------ Lie groups
LIE_ROWS = 1000
BIG_HEAD, BIG_TAIL = 2048 * 256, 257  # the launch is capped at 2048 x 256 lanes: one row more needs the second trip
BIG_ROWS = BIG_HEAD + BIG_TAIL


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _loguniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


@functools.lru_cache(maxsize=None)
def tangents(group):
    """[1000, K] float64.  Rotation angles: rows 0-399 log-uniform in [1e-9, pi - 1e-3]; 400-599 dense on both sides of
    EPS = 1e-6 (0.5e-6 .. 1.5e-6); 600-899 log-uniform in [1e-5, 1e-2], the float32 cancellation zone of (1 - cos t) / t^2;
    900-999 the four (|sigma|, t) combinations of calcW below / just above EPS, 25 rows each.  tau ~ N(0, 1), sigma ~
    N(0, 0.5) outside rows 900-999."""
    rng = np.random.default_rng(1000 + lg.GROUPS[group])
    n = LIE_ROWS
    theta = np.concatenate([_loguniform(rng, 1e-9, np.pi - 1e-3, 400), 1e-6 * np.linspace(0.5, 1.5, 200),
                            _loguniform(rng, 1e-5, 1e-2, 300), np.zeros(100)])
    theta[0], theta[399] = 1e-9, np.pi - 1e-3  # both ends themselves
    sigma = 0.5 * rng.standard_normal(n)
    lo = lambda m: _loguniform(rng, 1e-9, 9e-7, m)
    hi = lambda m: _loguniform(rng, 1.1e-6, 1e-3, m)
    theta[900:] = np.concatenate([lo(25), lo(25), hi(25), hi(25)])
    sigma[900:] = np.concatenate([lo(25), hi(25), lo(25), hi(25)]) * rng.choice([-1.0, 1.0], 100)
    phi = theta[:, None] * _unit(rng, n)
    return lg.join_tangent(group, rng.standard_normal((n, 3)), phi, sigma)


# rows of `elements` that are replaced by explicit inputs of `log`
ROWS_W_SMALL, ROWS_SN_SMALL, ROWS_W_NEG, ROWS_UNNORM = slice(0, 16), slice(16, 32), slice(32, 64), slice(64, 96)


@functools.lru_cache(maxsize=None)
def elements(group):
    """[1000, N] float64: exp(tangents) by the reference, with rows 0-15 at |w| < 1e-6 (both signs; the rotation is pi to
    within 2e-6), 16-31 at x^2 + y^2 + z^2 < 1e-12 (w = +-1), 32-63 negated (w < 0 at ordinary angles), 64-95 scaled by
    0.5 .. 2 (not normalised: the kernels renormalise on load)"""
    rng = np.random.default_rng(2000 + lg.GROUPS[group])
    X = lg.exp(group, tangents(group))
    o = 3 if lg.HAS_T[group] else 0
    q = X[:, o:o + 4].copy()
    w = _loguniform(rng, 1e-8, 9e-7, 16) * np.tile([1.0, -1.0], 8)
    q[ROWS_W_SMALL] = np.concatenate([np.sqrt(1 - w ** 2)[:, None] * _unit(rng, 16), w[:, None]], 1)
    v = _loguniform(rng, 1e-9, 9e-7, 16)[:, None] * _unit(rng, 16)
    q[ROWS_SN_SMALL] = np.concatenate([v, np.tile([1.0, -1.0], 8)[:, None]], 1)
    q[ROWS_SN_SMALL] /= np.linalg.norm(q[ROWS_SN_SMALL], axis=-1, keepdims=True)
    q[ROWS_W_NEG] = np.where(q[ROWS_W_NEG, 3:4] > 0, -q[ROWS_W_NEG], q[ROWS_W_NEG])
    q[ROWS_UNNORM] *= rng.uniform(0.5, 2.0, (32, 1))
    X[:, o:o + 4] = q
    return X


@functools.lru_cache(maxsize=None)
def operands(group):
    """second operands [1000, .]: another element (for mul), a tangent, a point, a homogeneous point - O(1)"""
    rng = np.random.default_rng(3000 + lg.GROUPS[group])
    Y = lg.exp(group, 0.4 * rng.standard_normal((LIE_ROWS, lg.K[group])))
    return SimpleNamespace(Y=Y, a=rng.standard_normal((LIE_ROWS, lg.K[group])), p3=rng.standard_normal((LIE_ROWS, 3)),
                           p4=rng.standard_normal((LIE_ROWS, 4)))


def branch_census(group, dtype):
    """how many rows take each branch of exp (on `tangents`) and log (on `elements`), the predicates evaluated in `dtype`
    as the kernels do (after the normalisation on load)"""
    a = tangents(group).astype(dtype)
    _, phi, sigma = lg.split_tangent(group, a)
    theta = np.sqrt((phi * phi).sum(-1))
    eps = dtype(lg.EPS)
    out = {"exp_taylor": int((theta < eps).sum()), "exp_closed": int((theta >= eps).sum())}
    if lg.HAS_S[group]:
        for name, m in (("w_ss_ts", (np.abs(sigma) < eps) & (theta < eps)), ("w_ss_tl", (np.abs(sigma) < eps) & (theta >= eps)),
                        ("w_sl_ts", (np.abs(sigma) >= eps) & (theta < eps)), ("w_sl_tl", (np.abs(sigma) >= eps) & (theta >= eps))):
            out[name] = int(m.sum())
    X = elements(group).astype(dtype)
    o = 3 if lg.HAS_T[group] else 0
    q = X[:, o:o + 4]
    q = q * (dtype(1) / np.sqrt((q * q).sum(-1, keepdims=True)))
    sn, w = (q[:, :3] ** 2).sum(-1), q[:, 3]
    out["log_sn_small"] = int((sn < dtype(lg.EPS * lg.EPS)).sum())
    out["log_w_small_pos"] = int(((sn >= dtype(lg.EPS * lg.EPS)) & (np.abs(w) < eps) & (w > 0)).sum())
    out["log_w_small_neg"] = int(((sn >= dtype(lg.EPS * lg.EPS)) & (np.abs(w) < eps) & (w < 0)).sum())
    out["log_atan_w_neg"] = int(((sn >= dtype(lg.EPS * lg.EPS)) & (np.abs(w) >= eps) & (w < 0)).sum())
    out["log_atan_w_pos"] = int(((sn >= dtype(lg.EPS * lg.EPS)) & (np.abs(w) >= eps) & (w > 0)).sum())
    return out


@functools.lru_cache(maxsize=None)
def big_set():
    """SE3 elements [524 545, 7] float32, points [.., 3] and upstream gradients [.., 3]: row 524 288 + i equals row i for
    i < 257, so the second grid-stride trip must reproduce the head bit for bit.  `sample`: 4096 rows for the oracle,
    3839 spread over everything and the whole tail."""
    rng = np.random.default_rng(77)
    xi = rng.standard_normal((BIG_HEAD, 6)) * np.array([1, 1, 1, 0.5, 0.5, 0.5])
    X = lg.exp("SE3", xi, matrix_exponential=False).astype(np.float32)
    p = rng.standard_normal((BIG_HEAD, 3)).astype(np.float32)
    gr = rng.standard_normal((BIG_HEAD, 3)).astype(np.float32)
    rep = lambda a: np.ascontiguousarray(np.concatenate([a, a[:BIG_TAIL]]))
    sample = np.unique(np.concatenate([np.linspace(0, BIG_HEAD - 1, 4096 - BIG_TAIL).astype(np.int64),
                                       np.arange(BIG_HEAD, BIG_ROWS)]))
    return SimpleNamespace(X=rep(X), p=rep(p), grad=rep(gr), sample=sample)


# ------------------------------------------------------------------------------------------------ frontend_next_frame
@functools.lru_cache(maxsize=None)
def next_frame_case():
    """poses [8, 7] and disps [8, 2, 2993] float32 for `vipe_frontend_next_frame` at t1 = 6 (frames 6 and 7 hold
    sentinels the kernel must overwrite / leave alone), and the float64 constant-velocity pose
    Exp(1/2 Log(G_5 G_4^-1)) G_5 from the oracle's own operators"""
    rng = np.random.default_rng(91)
    c = SimpleNamespace(t1=6, V=2, P=41 * 73)
    poses = lg.exp("SE3", rng.standard_normal((8, 6)) * np.array([1, 1, 1, 0.3, 0.3, 0.3]), matrix_exponential=False)
    c.poses = poses.astype(np.float32)
    c.disps = rng.uniform(0.2, 1.0, (8, c.V, c.P)).astype(np.float32)
    p64 = c.poses.astype(np.float64)
    rel = lg.mul("SE3", p64[5:6], lg.inv("SE3", p64[4:5]))
    c.pose_ref = lg.mul("SE3", lg.exp("SE3", 0.5 * lg.log("SE3", rel), matrix_exponential=False), p64[5:6])[0]
    return c
