"""Writes geom_parent_bits.npz: what the eight frame geometry operations of geom_ops.hip - frame distance (plain and
fused over a rig), depth filter, projmap and back-projection for the pinhole family, frame distance, depth filter and
back-projection on the sphere - computed BEFORE the pinhole and the sphere kernels became two instantiations of one pixel
walk.  Run on the GPU with the parent commit's library (the C ABI is the same on both sides):

    VIPE_AMD_LIB=<parent's libvipe_amd.so> python tests/golden/make_golden_geom_parent.py --out tests/golden/geom_parent_bits.npz

tests/test_gpu_geom_scatter.py::test_frame_ops_bits_unchanged runs `run_case` on the current build and compares bits.  None
of these kernels uses atomics and every reduction has a fixed order, so every array repeats exactly.

Inputs: oracle/frame_cases.py for the pinhole family (two small grids for everything, the 41 x 73 grid for the two scalar
frame distances, the MEI intr_dim == 5 row once), tests/panorama_reference.py for the sphere (the frame-distance cases of
tests/test_gpu_panorama.py with their NaN disparities, the depth-filter case, one back-projection), and one input per
family that lands on exactly 75 % valid pixels, where the two families decide differently (`quarter_invalid_case`).
"""

import argparse
import os
import sys

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLD))
for p in (ROOT, os.path.dirname(GOLD)):
    if p not in sys.path:
        sys.path.insert(0, p)

SMALL_GRIDS = [(9, 29), (5, 7)]
LARGE_GRID = (41, 73)
SPHERE_FD_CASES = ["g8x16_n5", "g12x24_rig2"]


def sphere_graph(name):
    """the graph of a tests/panorama_reference.py case, without its float64 solver history"""
    import panorama_reference as R
    from vipe_amd.synth import make_panorama_graph
    return make_panorama_graph(**R.ba_cases()[name][0])


def sphere_frame_distance_case(name):
    """the inputs of tests/test_gpu_panorama.py::test_frame_distance: all ordered pairs, a third of one frame NaN"""
    g = sphere_graph(name)
    V, n = g.V, g.n
    disps = g.disps.copy()
    disps[(n - 1) * V].reshape(-1)[::3] = np.nan
    pairs = [(i, j) for i in range(n) for j in range(n) if i != j]
    pi = np.repeat(np.array([p[0] for p in pairs], np.int64), V)
    pj = np.repeat(np.array([p[1] for p in pairs], np.int64), V)
    qi = np.tile(np.arange(V, dtype=np.int64), len(pairs))
    qj = (qi + (1 if V > 1 else 0)) % V
    return g, disps, pi, qi, pj, qj


def quarter_invalid_case():
    """Two keyframes on the 8 x 16 grid, constant disparity, the last two of the eight rows NaN (unusable pixels, as in
    the sphere's frame-distance cases; the sphere has no `behind the camera` for a pose to push rows to), beta = 1: the
    weights are 1 and 0, so valid / total is 96 / 128 = 0.75 without rounding.  The pinhole family decides
    `vv / (tt + 1e-8) < 0.75` in double (true: 1000), the sphere in float (128 + 1e-8f == 128, false: the mean)."""
    poses = np.array([[0, 0, 0, 0, 0, 0, 1], [0.1, 0.02, -0.05, 0, 0, 0, 1]], np.float32)
    rig = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    disps = np.full((2, 8, 16), 0.5, np.float32)
    disps[:, 6:] = np.nan
    intr_full = np.array([[100.0, 100.0, 64.0, 32.0]], np.float32)
    z = np.zeros(1, np.int64)
    return poses, rig, disps, intr_full, z, z, z + 1, z


def run_case():
    """-> dict of float32 arrays computed by the device"""
    import torch

    import panorama_reference as R
    from oracle import frame_cases as fc
    from oracle import se3
    from vipe_amd.ext import slam_ext

    dev = torch.device("cuda:0")

    def T(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    out = {}

    def keep(key, t):
        out[key] = t.cpu().numpy()

    for grid in SMALL_GRIDS + [LARGE_GRID]:
        c, r, tag = fc.geom_case(*grid), fc.rig_case(*grid), "%dx%d" % grid
        keep(f"pinhole_frame_distance_{tag}",
             slam_ext.frame_distance(T(c.fd_poses), T(c.disps), T(c.intr2), T(fc.FD_PI), T(fc.FD_PJ), T(fc.FD_QI), T(fc.FD_QJ),
                                     T(fc.FD_DI), fc.BETA))
        rig_idx = (T(fc.RIG_PI), T(fc.RIG_QI), T(fc.RIG_PJ), T(fc.RIG_QJ))
        for bidir in (False, True):
            keep(f"pinhole_frame_distance_rig_{tag}_bidir{int(bidir)}",
                 slam_ext.frame_distance_rig(T(r.poses), T(r.rig), T(r.disps), T(r.intr_full), *rig_idx, fc.BETA,
                                             bidirectional=bidir))
        if grid == LARGE_GRID:
            continue
        keep(f"pinhole_depth_filter_{tag}",
             slam_ext.depth_filter(T(c.g.poses), T(c.disps), T(c.intr), T(fc.DF_INDS), T(c.df_thresh)))
        coords, valid = slam_ext.projmap(T(c.pm_poses), T(c.disps), T(c.intr), T(fc.PM_II), T(fc.PM_JJ))
        keep(f"pinhole_projmap_coords_{tag}", coords)
        keep(f"pinhole_projmap_valid_{tag}", valid)
        keep(f"pinhole_iproj_{tag}", slam_ext.iproj(T(c.g.poses), T(c.disps), T(c.intr)))
        if grid == SMALL_GRIDS[0]:  # the MEI row: f / (1 + k1) inside the kernel
            mei = np.concatenate([r.intr_full, np.array([[0.6], [0.4]], np.float32)], 1)
            keep(f"mei_frame_distance_rig_{tag}",
                 slam_ext.frame_distance_rig(T(r.poses), T(r.rig), T(r.disps), T(mei), *rig_idx, fc.BETA, camera="mei"))

    for name in SPHERE_FD_CASES:
        g, disps, pi, qi, pj, qj = sphere_frame_distance_case(name)
        for bidir in (False, True):
            keep(f"sphere_frame_distance_{name}_bidir{int(bidir)}",
                 slam_ext.frame_distance_rig(T(g.poses), T(g.rig), T(disps), None, T(pi), T(qi), T(pj), T(qj), 0.3, bidir,
                                             camera="panorama"))
    g, thresh = R.depth_filter_case()
    keep("sphere_depth_filter", slam_ext.depth_filter(T(g.poses_gt), T(g.disps_gt), None, T(np.arange(g.n)),
                                                      T(thresh.astype(np.float32)), camera="panorama"))
    g = sphere_graph("g12x24_n4")
    c2w = se3.se3_inv(g.poses.astype(np.float64)).astype(np.float32)
    keep("sphere_iproj", slam_ext.iproj(T(c2w), T(g.disps), None, camera="panorama"))

    poses, rig, disps, intr_full, *idx = quarter_invalid_case()
    for camera in ("pinhole", "panorama"):
        keep(f"{camera}_quarter_invalid", slam_ext.frame_distance_rig(T(poses), T(rig), T(disps), T(intr_full), *map(T, idx),
                                                                       1.0, bidirectional=False, camera=camera))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    arrays = run_case()
    again = run_case()
    for k, v in arrays.items():
        assert v.dtype == np.float32 and np.array_equal(v.view(np.uint32), again[k].view(np.uint32)), f"{k} does not repeat"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print("wrote", a.out, {k: v.shape for k, v in arrays.items()})
    print("exactly 75 % valid: pinhole", arrays["pinhole_quarter_invalid"], "sphere", arrays["panorama_quarter_invalid"])
