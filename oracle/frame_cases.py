"""Inputs for the slam_ext geometry kernels at grids beyond one 256-lane workgroup, with index arrays that do not alias.

ORACLE (test infrastructure).  One place builds them, so that the CPU test that checks the inputs themselves (valid-share
margins, shares of near-threshold pixels, the presence of both depth branches: tests/test_oracle_frame_ops.py) and the
GPU test that feeds them to the kernels (tests/test_gpu_geom_scatter.py) look at the same numbers.
"""

import functools
from types import SimpleNamespace

import numpy as np

from vipe_amd.synth import make_graph

from . import frame_ops, se3

# (ht, wd): ragged with ~12 trips per lane and a partial last workgroup / five pixels past one workgroup / exactly one
# workgroup / less than one wave
GRIDS = [(41, 73), (9, 29), (16, 16), (5, 7)]
BETA = 0.3
N = 8

# frame_distance: pose, disparity and intrinsics indices are five different arrays.  Pair 4 looks at frame 6 (pushed back
# by one unit: the pixels nearer than 4/3 fall behind MIN_DEPTH, the rest stay valid), pair 5 at frame 7 (far behind
# every source: < 75 % valid, the kernel's 1000)
FD_PI = np.array([0, 1, 2, 5, 3, 4, 2], dtype=np.int64)
FD_PJ = np.array([1, 0, 5, 2, 6, 7, 4], dtype=np.int64)
FD_DI = np.array([2, 1, 0, 3, 5, 4, 6], dtype=np.int64)
FD_QI = np.array([0, 1, 0, 1, 1, 0, 1], dtype=np.int64)
FD_QJ = np.array([0, 0, 1, 1, 0, 1, 0], dtype=np.int64)
FD_PARTIAL, FD_FAR = 4, 5

# depth_filter: a permuted subset (num != n) with the first and the last frame, one threshold each
DF_INDS = np.array([5, 0, 7, 2], dtype=np.int64)
DF_SCALE = np.array([2.0, 1.0, 3.0, 1.5], dtype=np.float32)

# projmap: edge 2 targets frame 3, which stands 1.5 units behind: target depths 1 - 1.5 d run from -0.5 to 0.7
PM_II = np.array([0, 1, 2, 5, 7, 3, 6], dtype=np.int64)
PM_JJ = np.array([1, 0, 3, 2, 4, 3, 3], dtype=np.int64)

# frame_distance_rig on a two-view rig: same-view and cross-view pairs, the self pair of a keyframe's two views
RIG_PI = np.array([0, 1, 2, 5, 7, 3, 6, 4], dtype=np.int64)
RIG_QI = np.array([0, 1, 0, 1, 1, 0, 1, 0], dtype=np.int64)
RIG_PJ = np.array([1, 0, 6, 2, 4, 3, 5, 7], dtype=np.int64)
RIG_QJ = np.array([0, 1, 1, 0, 1, 1, 0, 0], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def geom_case(ht, wd):
    """the inputs of every geometry kernel on a (ht, wd) grid of n = 8 frames (image = 8 x grid)"""
    g = make_graph(n=N, height=8 * ht, width=8 * wd, radius=2, seed=100 * ht + wd)
    intr8 = (g.intrinsics[0] / 8.0).astype(np.float32)
    c = SimpleNamespace(ht=ht, wd=wd, g=g, disps=g.disps)
    c.intr = intr8
    c.intr2 = np.stack([intr8, np.float32(1.03) * intr8]).astype(np.float32)  # two intrinsics rows for qi / qj to select
    c.fd_poses = g.poses.copy()
    c.fd_poses[6, 2] -= 1.0
    c.fd_poses[7, 2] = -100.0
    c.df_thresh = (DF_SCALE * np.float32(0.05 / g.disps.mean())).astype(np.float32)
    c.pm_poses = g.poses.copy()
    c.pm_poses[3, 2] -= 1.5
    return c


@functools.lru_cache(maxsize=None)
def rig_case(ht, wd):
    """a two-view rig over the same clip: disps [n * 2, ht, wd] (view 1 takes the ground-truth maps), full-resolution
    intrinsics [2, 4], and the per-view poses R_v^-1 G_n composed on the host in float64"""
    c = geom_case(ht, wd)
    g = c.g
    r = SimpleNamespace(ht=ht, wd=wd, poses=g.poses, V=2)
    r.rig = np.concatenate([se3.se3_identity(1, np.float64),
                            se3.se3_exp(np.array([[0.3, 0.02, -0.01, 0.01, 0.2, -0.02]]))]).astype(np.float32)
    r.disps = np.ascontiguousarray(np.stack([g.disps, g.disps_gt], 1).reshape(2 * N, ht, wd))
    r.intr_full = np.stack([g.intrinsics[0], np.float32(1.03) * g.intrinsics[0]]).astype(np.float32)
    rig64, poses64 = r.rig.astype(np.float64), g.poses.astype(np.float64)
    r.view_poses = se3.se3_mul(se3.se3_inv(rig64)[None, :], poses64[:, None]).reshape(2 * N, 7).astype(np.float32)
    r.intr8 = (r.intr_full / np.float32(8.0)).astype(np.float32)
    return r


def rig_reference(r, bidirectional):
    """frame_distance_rig through the plain `frame_distance` oracle on the host-composed per-view poses -> the
    distances [M] and the valid shares [1 or 2, M] of the directions that went into them"""
    si, sj = RIG_PI * r.V + RIG_QI, RIG_PJ * r.V + RIG_QJ
    d, share = frame_ops.frame_distance(r.view_poses, r.disps, r.intr8, si, sj, RIG_QI, RIG_QJ, si, BETA, with_share=True)
    if not bidirectional:
        return d, share[None]
    back, share_back = frame_ops.frame_distance(r.view_poses, r.disps, r.intr8, sj, si, RIG_QJ, RIG_QI, sj, BETA,
                                                with_share=True)
    return np.float32(0.5) * (d + back), np.stack([share, share_back])
