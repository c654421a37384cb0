"""Dense-BA problems off the smooth trajectory: validity, zero support, step rejection, ragged and large plans.

ORACLE (test infrastructure).  Pure numpy, seeded, CPU-only.  Every case starts from `vipe_amd.synth.make_graph` /
`make_rig_graph` and then edits what they return (new ground truth, edges, weights, targets); `synth.py` itself is what
the benchmark times and stays as it is.  One place builds the cases, so that the CPU test that proves what each one
reaches (tests/test_oracle_ba_cases.py), the fixture generator (tests/golden/make_golden.py:gen_ba_edges) and the GPU
test that feeds them to the kernels (tests/test_gpu_ba_edges.py) look at the same numbers.  Everything is cached;
nothing is modified after it is built.

A case is a namespace: `g` (a SyntheticGraph / SyntheticRigGraph: what `run_hip_ba` / `run_hip_ba_rig` of
tests/test_gpu_parity.py take), `cam`, `intr` (full resolution, with k1 for MEI), `bk` (the BA keyword arguments) and
`rig` (True for the multi-view case).

Grids: 13 x 17 = 221 pixels is one partial 256-pixel tile, 17 x 19 = 323 two tiles (the second partial), 4 x 6 = 24 for
the two large plans.
"""

import functools
from types import SimpleNamespace

import numpy as np

from vipe_amd.synth import _qexp, _qmul, _se3_inv, _se3_mul, expand_edges, make_graph, make_rig_graph, neighbourhood_edges

from . import ba, geom, se3

MONO = ("behind_pinhole", "behind_mei", "zero_support", "reject_and_clamp", "ragged_plan", "deg9_17", "m4160")
RIG = ("rig8_n129",)
ALL = MONO + RIG
BEHIND_K1 = 0.35
BEHIND_SEED = {"pinhole": 4414, "mei": 4104}  # chosen so that no (term, pixel) comes within 1e-3 of MIN_DEPTH (see the CPU test)
F8 = np.float64
F4 = np.float32


def _bk(t0, t1, n_iters=2, pose_damping=1e-3, pose_ep=0.1, **kw):
    out = dict(t0=t0, t1=t1, n_iters=n_iters, pose_damping=pose_damping, pose_ep=pose_ep, motion_only=False,
               limited_disp=False, optimize_intrinsics=False)
    out.update(kw)
    return out


def _coords(poses, disps, intr, rig, pi, qi, pj, qj, di, cam):
    """float64 reprojection of the given state through the oracle's geometry -> [M,ht,wd,2]"""
    intr8 = geom.scaled_intrinsics(np.asarray(intr, F8), 1.0 / 8.0, cam)
    return geom.reproject(np.asarray(poses, F8), np.asarray(disps, F8), intr8, np.asarray(rig, F8), pi, pj, qi, qj, di,
                          cam)["coords"]


def _retarget(g, intr, cam, rng, noise=0.5):
    """targets of a mono graph = reprojection of its ground truth + N(0, noise px), for the edges it holds now"""
    z = np.zeros_like(g.ii)
    c = _coords(g.poses_gt, g.disps_gt, intr, se3.se3_identity(1), g.ii, z, g.jj, z, g.ii, cam)
    g.target = (c + rng.normal(0, noise, c.shape)).astype(F4)


def _perturb(g, rng, pose_noise=0.003, disp_noise=0.05):
    """starting point = ground truth moved as make_graph moves it (pose 0 stays)"""
    n = g.n
    dT = np.concatenate([rng.normal(0, pose_noise, (n, 3)), _qexp(rng.normal(0, pose_noise, (n, 3)))], -1)
    dT[0] = [0, 0, 0, 0, 0, 0, 1]
    poses = _se3_mul(dT, g.poses_gt.astype(F8))
    poses[:, 3:] /= np.linalg.norm(poses[:, 3:], axis=-1, keepdims=True)
    g.poses = poses.astype(F4)
    g.disps = (g.disps_gt.astype(F8) * (1 + rng.normal(0, disp_noise, g.disps_gt.shape))).astype(F4)


def _mono(name, g, bk, cam="pinhole", intr=None):
    return SimpleNamespace(name=name, g=g, cam=cam, intr=g.intrinsics if intr is None else intr, bk=bk, rig=False)


# ------------------------------------------------------------------------------------------------ behind


def _behind(cam):
    """n = 5, radius 2, 17 x 19.  The camera moves FORWARD by 0.1 a frame and turns about y by 0.95 rad at frame 3 and
    once more at frame 4.  Frame 0 holds disparities up to 12: Z = 1 - 0.1 (j - i) d passes MIN_DEPTH and then zero in its
    terms 0 -> 1 and 0 -> 2.  The pairs 1 <-> 3, 2 <-> 3 and 3 <-> 4 (about 1 rad) put part of their pixels behind the target
    camera, 2 <-> 4 (2 rad) nearly all of them.  Frames 1 and 4 carry their quaternion with w < 0."""
    rng = np.random.default_rng(BEHIND_SEED[cam])
    g = make_graph(n=5, height=136, width=152, radius=2, seed=4100)
    n = g.n
    yaw = np.array([0.0, 0.03, -0.03, 0.95, 2.0])
    c2w_t = np.stack([0.02 * np.arange(n), np.zeros(n), 0.1 * np.arange(n)], -1) + rng.normal(0, 0.002, (n, 3))
    c2w_q = _qmul(_qexp(np.stack([np.zeros(n), yaw, np.zeros(n)], -1)), _qexp(rng.normal(0, 0.01, (n, 3))))
    c2w = np.concatenate([c2w_t, c2w_q], -1)
    c2w[0] = [0, 0, 0, 0, 0, 0, 1]
    gt = _se3_inv(c2w)
    gt[[1, 4]] *= np.array([1, 1, 1, -1, -1, -1, -1.0])  # the same rotations, w < 0
    g.poses_gt = gt.astype(F4)
    d = 1.0 / rng.uniform(1.0, 5.0, (n, g.ht, g.wd))
    # Z = 1 - 0.1 (j - i) d crosses MIN_DEPTH at d = 9 and 4.5: the three bands stay clear of both
    band = rng.integers(0, 3, (g.ht, g.wd))
    d[0] = rng.uniform(np.array([0.2, 4.9, 9.5])[band], np.array([4.1, 8.5, 12.0])[band])
    g.disps_gt = d.astype(F4)
    intr = g.intrinsics if cam == "pinhole" else np.concatenate([g.intrinsics, np.array([[BEHIND_K1]], F4)], 1)
    _perturb(g, rng, pose_noise=0.002, disp_noise=0.02)
    assert (g.poses[[1, 4], 6] < 0).all()
    _retarget(g, intr, cam, rng, noise=0.3)
    return _mono("behind_" + cam, g, _bk(1, 5), cam, intr)


# ------------------------------------------------------------------------------------------------ zero support

ZS_EDGE, ZS_FRAME = 3, 3  # the edge and the free source frame without any weight


def _zero_support():
    """n = 6, radius 2, 13 x 17: 30 % of the (edge, pixel) pairs without weight, 20 % with exactly one component at zero,
    edge ZS_EDGE all zero, no weight in any term whose source is frame ZS_FRAME, and eta = 0 there: C = 2e-7."""
    rng = np.random.default_rng(4201)
    g = make_graph(n=6, height=104, width=136, radius=2, seed=4200)
    w = g.weight.copy()
    E = len(g.ii)
    u = rng.random((E, g.ht, g.wd))
    w[u < 0.3] = 0
    one = (u >= 0.3) & (u < 0.5)
    which = rng.integers(0, 2, one.shape)
    w[..., 0][one & (which == 0)] = 0
    w[..., 1][one & (which == 1)] = 0
    w[ZS_EDGE] = 0
    w[g.ii == ZS_FRAME] = 0
    g.weight = w
    eta = g.eta.copy()
    eta[ZS_FRAME] = 0
    g.eta = eta
    return _mono("zero_support", g, _bk(1, 6))


# ------------------------------------------------------------------------------------------------ reject and clamp

RC_SHARE, RC_WEIGHT, RC_SHIFT = 0.05, 2e-3, 50.0


def reject_pixels():
    """[n, ht, wd] in {0, +1, -1}: the pixels of `reject_and_clamp` whose targets are moved, and to which side"""
    rng = np.random.default_rng(4302)
    g = make_graph(n=5, height=104, width=136, radius=2, seed=4300)
    hit = rng.random((g.n, g.ht, g.wd)) < RC_SHARE
    return hit * rng.choice([-1.0, 1.0], hit.shape)


def _reject_and_clamp():
    """n = 5, radius 2, 13 x 17.  5 % of the pixels of every frame: weight RC_WEIGHT in all their terms, eta = 0, and the
    target of every such term moved by +-50 px along d coords / d disparity (the epipolar direction), the same sign in
    every term of a pixel.  With |Jz| of 0.8 .. 1.7 px per unit disparity the step dz = -sum w Jz r / (sum w Jz^2 + 2e-7)
    is some +-30 .. 60: the positive ones are rejected, the negative ones are applied."""
    rng = np.random.default_rng(4301)
    g = make_graph(n=5, height=104, width=136, radius=2, seed=4300)
    sgn = reject_pixels()
    z = np.zeros_like(g.ii)
    intr8 = geom.scaled_intrinsics(g.intrinsics.astype(F8), 1.0 / 8.0, "pinhole")
    o = geom.reproject(g.poses.astype(F8), g.disps.astype(F8), intr8, se3.se3_identity(1), g.ii, g.jj, z, z, g.ii,
                       "pinhole", jacobian=True)
    Jz = o["Jz"]
    dirn = Jz / np.linalg.norm(Jz, axis=-1, keepdims=True)
    s = sgn[g.ii]  # [E,ht,wd]
    hit = s != 0
    tgt, w, eta = g.target.astype(F8), g.weight.copy(), g.eta.copy()
    # r = coords - target: a target moved by +s along Jz asks for dz = +s 50 / |Jz|
    tgt[hit] = (o["coords"] + RC_SHIFT * s[..., None] * dirn)[hit]
    w[hit] = RC_WEIGHT
    eta[sgn != 0] = 0
    g.target, g.weight, g.eta = tgt.astype(F4), w, eta
    del rng
    return _mono("reject_and_clamp", g, _bk(1, 5))


# ------------------------------------------------------------------------------------------------ ragged plan

RAGGED_UNUSED, RAGGED_TARGET_ONLY, RAGGED_DUPLICATES = 4, 7, 3


def _ragged_plan(duplicates=RAGGED_DUPLICATES):
    """n = 9, window [2, 6), 13 x 17, radius 2: every edge of pose 4 removed (a pose of the window without edges), every
    edge whose SOURCE is pose 7 removed (7 >= t1 is then only a target and stays free, buffer.py:462), poses 6 and 8 are
    sources >= t1 (fixed), 0 and 1 are sources below t0 with free targets (0 -> 2, 1 -> 2, 1 -> 3) and the pair 0 <-> 1 has
    both ends fixed; `duplicates` edges occur twice with data of their own; the list is shuffled."""
    rng = np.random.default_rng(4401)
    g = make_graph(n=9, height=104, width=136, radius=2, seed=4400)
    keep = (g.ii != RAGGED_UNUSED) & (g.jj != RAGGED_UNUSED) & (g.ii != RAGGED_TARGET_ONLY)
    ii, jj, tgt, w = g.ii[keep], g.jj[keep], g.target[keep], g.weight[keep]
    if duplicates:
        pick = np.array([np.flatnonzero((ii == a) & (jj == b))[0] for a, b in ((2, 3), (5, 7), (1, 2))][:duplicates])
        ii, jj = np.concatenate([ii, ii[pick]]), np.concatenate([jj, jj[pick]])
        tgt = np.concatenate([tgt, tgt[pick] + rng.normal(0, 0.5, tgt[pick].shape).astype(F4)])
        w = np.concatenate([w, rng.uniform(0, 1, w[pick].shape).astype(F4)])
    perm = rng.permutation(len(ii))
    g.ii, g.jj, g.target, g.weight = ii[perm], jj[perm], tgt[perm], w[perm]
    return _mono("ragged_plan", g, _bk(2, 6))


# ------------------------------------------------------------------------------------------------ degrees 7, 9, 17

DEG_WANT = {0: 17, 5: 9, 10: 7}


def _deg9_17():
    """n = 19, 13 x 17: the chain i <-> i + 1, and frames 0, 5 and 10 as sources of 17, 9 and 7 terms (the matrix-core
    accumulate kernel takes up to 6; the walk stages the transforms of 8 terms at a time: 7 = one partial chunk, 9 = one
    chunk and one term, 17 = two chunks and one term)"""
    rng = np.random.default_rng(4501)
    g = make_graph(n=19, height=104, width=136, radius=1, seed=4500)
    ii, jj = neighbourhood_edges(19, 1)
    have = set(zip(ii.tolist(), jj.tolist()))
    ei, ej = [], []
    for src, deg in DEG_WANT.items():
        cur = int((ii == src).sum())
        for j in sorted(range(19), key=lambda j: (abs(j - src), j)):
            if cur == deg:
                break
            if j != src and (src, j) not in have:
                have.add((src, j))
                ei.append(src)
                ej.append(j)
                cur += 1
    g.ii = np.concatenate([ii, np.asarray(ei, np.int64)])
    g.jj = np.concatenate([jj, np.asarray(ej, np.int64)])
    E = len(g.ii)
    g.weight = rng.uniform(0, 1, (E, g.ht, g.wd, 2)).astype(F4)
    _retarget(g, g.intrinsics, "pinhole", rng)
    return _mono("deg9_17", g, _bk(1, 19))


# ------------------------------------------------------------------------------------------------ M = 4160


def _m4160():
    """n = 65, all 4160 ordered pairs in random order, 4 x 6: the counting sort of the plan stages 4096 terms at a time, so
    the last 64 terms - of many source frames after the shuffle - come in its second chunk; 64 terms per source frame,
    384 unknowns."""
    rng = np.random.default_rng(4601)
    g = make_graph(n=65, height=32, width=48, radius=64, seed=4600)
    assert len(g.ii) == 4160
    perm = rng.permutation(4160)
    g.ii, g.jj, g.target, g.weight = g.ii[perm], g.jj[perm], g.target[perm], g.weight[perm]
    return _mono("m4160", g, _bk(1, 65))


# ------------------------------------------------------------------------------------------------ nF = 1032


def _rig8_n129():
    """8 views x 129 keyframes = 1032 disparity frames (one more trip of every 1024-lane loop of the plan, two entries per
    lane in its scans), radius 1 + cross-view self edges: 385 edges, 3080 terms, 4 x 6; rig rotation and per-view
    intrinsics on: 6 x 128 + 8 + 42 = 818 unknowns."""
    g = make_rig_graph(n=129, V=8, height=32, width=48, radius=1, seed=4700)
    # half a pixel of target noise is a tenth of a radian at this focal length (5.4 grid pixels): 0.05 px instead
    rng = np.random.default_rng(4701)
    pi, qi, di, pj, qj = expand_edges(g.ii, g.jj, g.V)
    c = _coords(g.poses_gt, g.disps_gt.reshape(g.n * g.V, g.ht, g.wd), g.intrinsics, g.rig_gt, pi, qi, pj, qj, di, "pinhole")
    g.target = (c + rng.normal(0, 0.05, c.shape)).astype(F4)
    bk = dict(t0=1, t1=129, n_iters=2, pose_damping=1e-3, pose_ep=0.1, optimize_intrinsics=True, optimize_rig_rotation=True)
    return SimpleNamespace(name="rig8_n129", g=g, cam="pinhole", intr=g.intrinsics, bk=bk, rig=True)


_BUILD = {"behind_pinhole": lambda: _behind("pinhole"), "behind_mei": lambda: _behind("mei"), "zero_support": _zero_support,
          "reject_and_clamp": _reject_and_clamp, "ragged_plan": _ragged_plan, "deg9_17": _deg9_17, "m4160": _m4160,
          "rig8_n129": _rig8_n129}


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name]()


def terms(c):
    """pi, qi, di, pj, qj of the case's terms"""
    g = c.g
    return expand_edges(g.ii, g.jj, g.V if c.rig else 1)


def oracle_inputs(c):
    """positional arguments of `oracle.ba.bundle_adjustment` for the case (up to jj) and its keyword arguments"""
    g = c.g
    M = g.target.shape[0]
    tgt, w = g.target.reshape(M, -1, 2), g.weight.reshape(M, -1, 2)
    if c.rig:
        return [g.poses, g.disps, g.disps_sens, c.intr, g.rig, tgt, w, g.eta, g.ii, g.jj], dict(c.bk)
    return ([g.poses, g.disps[:, None], g.disps_sens[:, None], c.intr, se3.se3_identity(1), tgt, w, g.eta[:, None], g.ii,
             g.jj], dict(c.bk, model=c.cam))


@functools.lru_cache(maxsize=None)
def oracle_run(name, dtype="float64", debug=False):
    """(poses, disps [n,V,ht,wd], intrinsics, rig[, debug]) of the oracle on the case, computed once"""
    args, kw = oracle_inputs(case(name))
    return ba.bundle_adjustment(*args, dtype=np.dtype(dtype), return_debug=debug, **kw)


def case_counts(c):
    """(free poses, free disparity frames, unknowns) of a case namespace from the oracle's sets: what the plan reports in
    info[0], [1], [3]"""
    g = c.g
    V = g.V if c.rig else 1
    pi, qi, di, pj, qj = terms(c)
    t0, t1 = c.bk["t0"], c.bk["t1"]
    src = np.unique(g.ii)
    fixed = set(src[(src < t0) | (src >= t1)].tolist())
    free = sorted(set(pi.tolist() + pj.tolist()) - fixed)
    D = c.intr.shape[1] - 4
    tail = (V * (1 + D) if c.bk.get("optimize_intrinsics") else 0) + (6 * (V - 1) if c.bk.get("optimize_rig_rotation") else 0)
    return len(free), len(np.unique(di)), 6 * len(free) + tail


def counts(name):
    """`case_counts` of the named case"""
    return case_counts(case(name))


OUTPUTS = ("poses", "disps", "intr", "rig")


def output_bounds(o64, o32, factor=4, ulps=0):
    """Per output of the oracle (poses, disps, intrinsics, rig): delta32 = the elementwise-maximum distance between its
    float32 run (the reference's arithmetic) and its float64 run (exact), and the bound min(factor x delta32, the suite's
    1e-4 form: 1e-4 max(1, |p|), 1e-4 max|d|, 1e-4 max|k|, 1e-4 for the rig), not below `ulps` units in the last place of
    the largest float32 value of the output.  Nothing but the oracle enters.  -> dict output -> (delta32, bound)"""
    old = (1e-4 * max(1.0, np.abs(o64[0]).max()), 1e-4 * np.abs(o64[1]).max(), 1e-4 * np.abs(o64[2]).max(), 1e-4)
    out = {}
    for key, a, b, lim in zip(OUTPUTS, o32, o64, old):
        d32 = float(np.abs(a.astype(F8) - b).max())
        out[key] = (d32, max(min(factor * d32, lim), ulps * 2.0 ** -23 * float(np.abs(b).max())))
    return out


def step_bounds(name):
    """The tolerance of the GPU test, relative to the step: per output, 4 x delta32 on this case and never looser than the
    suite's 1e-4 form (`output_bounds`).  -> dict output -> (delta32, bound), outputs in the order poses, disps, intr, rig."""
    return output_bounds(oracle_run(name, "float64"), oracle_run(name, "float32"))
