"""Marginal covariances of the dense BA's damped Gauss-Newton system, in numpy (dtype-generic: float64 is the yardstick,
float32 gives the distance delta32 the GPU test's tolerance is built from).

The reference project has no such function; the definition is linear algebra over the linearisation that `oracle.ba`
already pins.  `linearize` rebuilds H, E and C of ONE iteration exactly as `oracle/ba.py` (lines 48-162) does: poses,
per-view intrinsics with the 1/8 J_scale, rig blocks with -J, merged keys (pi == pj, qi == qj), the sensor prior, the LM
damping of the regular rows and the disparity damping 1e-7 + (0.2 eta + 1e-7).  tests/test_ba_marginals_reference.py ties
its S and C to the `debug` output of `oracle.ba.bundle_adjustment` to 1e-10.

    H = [[B, E], [E^T, C]]   C diagonal      S = B - E C^-1 E^T
    var_p = 1 / C_p + (e_p^T S^-1 e_p) / C_p^2       pose covariance = 6 x 6 diagonal block of S^-1

These are the covariances of the damped, weighted problem: the confidence weights act as inverse variances, without a
noise scale.
"""

from types import SimpleNamespace

import numpy as np

from oracle import geom
from oracle.ba import _merge


def linearize(poses, disps, disps_sens, intrinsics, rig, target, weight, disp_damping, ii, jj, t0, t1, pose_damping,
              pose_ep, motion_only=False, limited_disp=False, optimize_intrinsics=False, optimize_rig_rotation=False,
              model="pinhole", alpha=0.001, dtype=np.float64, weight_scale=0.001, intrinsics_factor=8.0, n_iters=None):
    """Arguments as `oracle.ba.bundle_adjustment` (n_iters is accepted and ignored).  -> namespace with the damped B as
    `B` [n,n], `E` {(block key, frame k): [dim,P]}, `C` {k: [P]} (damped), `off`, `blocks`, `free_pose`, `free_disp`."""
    dt = np.dtype(dtype)
    poses = np.array(poses, dtype=dt)
    disps = np.array(disps, dtype=dt)
    intrinsics = np.array(intrinsics, dtype=dt)
    rig = np.array(rig, dtype=dt)
    Nbuf, V, ht, wd = disps.shape
    P = ht * wd
    dflat = disps.reshape(Nbuf * V, P)
    eta = np.asarray(disp_damping, dtype=dt).reshape(Nbuf * V, P)
    ii = np.asarray(ii, dtype=np.int64)
    jj = np.asarray(jj, dtype=np.int64)
    pi, qi, di, pj, qj, _ = geom.expand_edge_multiview(ii, jj, V, None)
    M = len(pi)
    target = np.asarray(target, dtype=dt).reshape(M, P, 2)
    wgt = (np.asarray(weight, dtype=dt) * dt.type(weight_scale)).reshape(M, P, 2)
    D = intrinsics.shape[1] - 4

    # fixed sets (oracle/ba.py:67-85)
    pi_unique = np.unique(ii)
    if t0 < t1:
        fixed_pose, all_pose_fixed = set(pi_unique[(pi_unique < t0) | (pi_unique >= t1)].tolist()), False
    else:
        fixed_pose, all_pose_fixed = set(), True
    di_unique = np.unique(di)
    if motion_only:
        fixed_disp = set(di_unique.tolist())
    elif limited_disp:
        fixed_disp = set(di[(pi < t0) | (pi >= t1)].tolist())
    else:
        fixed_disp = set()
    free_disp = [int(k) for k in di_unique if int(k) not in fixed_disp]
    sens32 = np.asarray(disps_sens, dtype=np.float32).reshape(Nbuf * V, P)
    sens_frames = [k for k in free_disp if float(sens32[k].sum()) > 0.0]

    pose_ids = [] if all_pose_fixed else sorted(set(pi.tolist() + pj.tolist()) - fixed_pose)
    blocks = [("pose", p, 6) for p in pose_ids]
    if optimize_intrinsics:
        blocks += [("intr", q, 1 + D) for q in range(V)]
    if optimize_rig_rotation:
        blocks += [("rig", q, 6) for q in range(1, V)]
    off, n = {}, 0
    for kind, idx, dim in blocks:
        off[(kind, idx)] = (n, dim)
        n += dim

    intr8 = geom.scaled_intrinsics(intrinsics, 1.0 / intrinsics_factor, model)
    g = geom.reproject(poses, dflat.reshape(Nbuf * V, ht, wd), intr8, rig, pi, pj, qi, qj, di, model, jacobian=True,
                       jacobian_f=optimize_intrinsics)
    w = g["valid"].reshape(M, P, 1) * wgt
    Ji = g["Ji"].reshape(M, P, 2, 6)
    Jj = g["Jj"].reshape(M, P, 2, 6)
    Jz = g["Jz"].reshape(M, P, 2)

    H = np.zeros((n, n), dtype=dt)
    E = {}
    C = {k: np.zeros(P, dtype=dt) for k in free_disp}
    for e in range(M):
        loc = []
        if ("pose", int(pi[e])) in off:
            loc.append((("pose", int(pi[e])), Ji[e]))
        if ("pose", int(pj[e])) in off:
            loc.append((("pose", int(pj[e])), Jj[e]))
        if optimize_intrinsics:
            sc = dt.type(1.0 / intrinsics_factor)
            loc.append((("intr", int(qi[e])), g["Jfi"][e].reshape(P, 2, 1 + D) * sc))
            loc.append((("intr", int(qj[e])), g["Jfj"][e].reshape(P, 2, 1 + D) * sc))
        if optimize_rig_rotation:
            if ("rig", int(qi[e])) in off:
                loc.append((("rig", int(qi[e])), -Ji[e]))
            if ("rig", int(qj[e])) in off:
                loc.append((("rig", int(qj[e])), -Jj[e]))
        loc = _merge(loc)
        keys = list(loc.keys())
        for a in keys:
            oa, da = off[a]
            Ja_w = loc[a] * w[e][:, :, None]
            for b in keys:
                ob, db = off[b]
                H[oa:oa + da, ob:ob + db] += np.einsum("pcd,pcf->df", Ja_w, loc[b])
        k = int(di[e])
        if k in C:
            wz = w[e] * Jz[e]
            C[k] += np.sum(wz * Jz[e], axis=1)
            for a in keys:
                Eak = np.einsum("pcd,pc->dp", loc[a], wz)
                E[(a, k)] = E[(a, k)] + Eak if (a, k) in E else Eak
    for k in sens_frames:
        C[k] += dt.type(alpha)
    for kind, idx, dim in blocks:
        o, _d = off[(kind, idx)]
        lam, ep = {"pose": (pose_damping, pose_ep), "intr": (1e-6, 1e-6), "rig": (1e-4, 1e-4)}[kind]
        for a in range(o, o + dim):
            H[a, a] += dt.type(ep) + dt.type(lam) * H[a, a]
    for k in free_disp:
        C[k] += dt.type(1e-7) + (dt.type(0.2) * eta[k] + dt.type(1e-7))
    return SimpleNamespace(B=H, E=E, C=C, off=off, blocks=blocks, n=n, free_pose=pose_ids, free_disp=free_disp,
                           shape=(Nbuf, V, P), dtype=dt)


def frame_members(lin, k):
    """-> (global rows [r], E rows [r, P]) of disparity frame k: its column block of E"""
    rows, blocks = [], []
    for (a, kk), Eak in lin.E.items():
        if kk == k:
            oa, da = lin.off[a]
            rows.append(np.arange(oa, oa + da))
            blocks.append(Eak)
    if not rows:
        return np.zeros(0, np.int64), np.zeros((0, lin.shape[2]), lin.dtype)
    return np.concatenate(rows), np.concatenate(blocks, 0)


def reduced_system(lin):
    """S = B - E C^-1 E^T (oracle/ba.py:164-178)"""
    S = lin.B.copy()
    for k in lin.free_disp:
        rows, Ek = frame_members(lin, k)
        if len(rows):
            S[np.ix_(rows, rows)] -= (Ek / lin.C[k][None]) @ Ek.T
    return S


def marginals(*args, **kw):
    """`linearize` arguments -> namespace: `lin`, `S`, `Sinv`, `disp_var` [Nbuf*V, P] and `pose_cov` [Nbuf, 6, 6] (NaN where
    the frame / pose is not free), `pose_part` [Nbuf*V, P] = (var - 1/C) C = e^T S^-1 e / C (NaN likewise)."""
    lin = linearize(*args, **kw)
    dt = lin.dtype
    Nbuf, V, P = lin.shape
    S = reduced_system(lin)
    Sinv = np.linalg.inv(S) if lin.n else np.zeros((0, 0), dt)
    disp_var = np.full((Nbuf * V, P), np.nan, dt)
    pose_part = np.full((Nbuf * V, P), np.nan, dt)
    for k in lin.free_disp:
        rows, Ek = frame_members(lin, k)
        q = np.einsum("ap,ab,bp->p", Ek, Sinv[np.ix_(rows, rows)], Ek) if len(rows) else np.zeros(P, dt)
        ic = dt.type(1.0) / lin.C[k]
        disp_var[k] = ic + q * ic * ic
        pose_part[k] = q * ic
    pose_cov = np.full((Nbuf, 6, 6), np.nan, dt)
    for p in lin.free_pose:
        o, _ = lin.off[("pose", p)]
        pose_cov[p] = Sinv[o:o + 6, o:o + 6]
    return SimpleNamespace(lin=lin, S=S, Sinv=Sinv, disp_var=disp_var, pose_cov=pose_cov, pose_part=pose_part)


def full_inverse_variance(lin, k):
    """diagonal of the dense inverse of the full Hessian over (regular unknowns, disparities of frame k): what the Schur
    identity above must reproduce.  The other frames' disparities are eliminated exactly (their Schur complement onto B)."""
    n = lin.n
    P = lin.shape[2]
    Bk = lin.B.copy()
    for kk in lin.free_disp:
        if kk == k:
            continue
        rows, Ek = frame_members(lin, kk)
        if len(rows):
            Bk[np.ix_(rows, rows)] -= (Ek / lin.C[kk][None]) @ Ek.T
    rows, Ek = frame_members(lin, k)
    Hf = np.zeros((n + P, n + P), lin.dtype)
    Hf[:n, :n] = Bk
    Hf[rows, n:] = Ek
    Hf[n:, rows] = Ek.T
    Hf[n:, n:] = np.diag(lin.C[k])
    return np.diag(np.linalg.inv(Hf))[n:]


# ---- the cases of the GPU test (oracle/ba_cases.py), shared with the CPU test

CASES = {
    "ragged_plan": ("ragged_plan", {}),
    "ragged_plan_intr": ("ragged_plan", {"optimize_intrinsics": True}),
    "behind_mei": ("behind_mei", {}),
    "behind_pinhole": ("behind_pinhole", {}),  # 17 x 19: a second, partial tile
    "deg9_17": ("deg9_17", {}),
    "m4160": ("m4160", {}),
    "rig8_n129": ("rig8_n129", {}),
}
_CACHE = {}


def case_kwargs(tag):
    """oracle positional arguments and keyword arguments of a case, with the tag's overrides"""
    from oracle import ba_cases as bc
    name, over = CASES[tag]
    args, kw = bc.oracle_inputs(bc.case(name))
    kw = dict(kw, **over)
    return args, kw


def case_marginals(tag, dtype="float64"):
    """the reference on a case, computed once per (case, dtype) and not modified afterwards"""
    key = (tag, dtype)
    if key not in _CACHE:
        args, kw = case_kwargs(tag)
        _CACHE[key] = marginals(*args, dtype=np.dtype(dtype), **kw)
    return _CACHE[key]


def rel_err_var(got, ref):
    """largest |got - ref| / ref over the finite entries of ref (variances are > 0)"""
    m = np.isfinite(ref)
    if not m.any():
        return 0.0
    return float(np.nan_to_num(np.abs(got[m].astype(np.float64) - ref[m]) / ref[m], nan=np.inf).max())


def rel_err_cov(got, ref):
    """largest |got_ij - ref_ij| / sqrt(ref_ii ref_jj) over the free poses: each entry of a covariance block against its
    own scale (for a diagonal entry this is the plain relative error; an off-diagonal entry may pass through zero)"""
    free = np.isfinite(ref[:, 0, 0])
    if not free.any():
        return 0.0
    r = ref[free].astype(np.float64)
    sd = np.sqrt(np.einsum("nii->ni", r))
    e = np.abs(got[free].astype(np.float64) - r) / (sd[:, :, None] * sd[:, None, :])
    return float(np.nan_to_num(e, nan=np.inf).max())


def delta32(tag):
    """(disp_var, pose_cov): largest relative distance between the reference in float32 and in float64 on the case"""
    a, b = case_marginals(tag, "float32"), case_marginals(tag, "float64")
    return rel_err_var(a.disp_var, b.disp_var), rel_err_cov(a.pose_cov, b.pose_cov)


def bounds(tag):
    """the GPU test's tolerance per output: 4 x delta32, never looser than 1e-4 (the convention of
    `oracle.ba_cases.step_bounds`) -> ((delta32, bound) of disp_var, (delta32, bound) of pose_cov)"""
    return tuple((d, min(4 * d, 1e-4)) for d in delta32(tag))
