"""Writes panorama_parent_bits.npz: what the pinhole and MEI instantiations of the reprojection and dense-BA kernels
computed on one small seeded graph BEFORE the panorama camera became their third instantiation.  Run on the GPU with
the parent commit's library:

    python tests/golden/make_golden_panorama_parent.py --out tests/golden/panorama_parent_bits.npz

tests/test_gpu_panorama.py::test_pinhole_mei_bits_unchanged re-creates the inputs through `parent_case` below and compares
bits.  The reprojection kernels are plain per-pixel arithmetic and repeat exactly; the BA sums through floating-point
atomics, so it is run twice here and `ba_repeatable_<camera>` records whether the parent's own two runs agreed.
"""

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CAMERAS = ("pinhole", "mei")


def parent_case(camera):
    """The seeded inputs: a 4-keyframe 12 x 16 graph (P = 192: one ragged 256-lane tile), MEI with k1 = 0.6."""
    from vipe_amd.synth import make_graph

    g = make_graph(n=4, height=96, width=128, radius=2, seed=11)
    intr = g.intrinsics.copy()
    if camera == "mei":
        intr = np.concatenate([intr, np.full((1, 1), 0.6, np.float32)], 1)
    return g, np.ascontiguousarray(intr, dtype=np.float32)


def run_case(camera):
    """-> dict of arrays computed by the device for `camera`"""
    import torch

    from vipe_amd.ext import slam_ext

    dev = torch.device("cuda:0")
    g, intr = parent_case(camera)

    def T(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)

    E = len(g.ii)
    z = np.zeros_like(g.ii)
    rig = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    idx = (T(g.ii), T(z), T(g.jj), T(z), T(g.ii))
    out = {}
    coords, valid = slam_ext.reproject(T(g.poses), T(g.disps), T(intr), T(rig), *idx, camera=camera)
    out["coords"], out["valid"] = coords.cpu().numpy(), valid.cpu().numpy()
    tgt = T(g.target)
    c16, m16 = slam_ext.reproject_motion(T(g.poses), T(g.disps), T(intr), T(rig), *idx, tgt, camera=camera)
    c32, m32 = slam_ext.reproject_motion(T(g.poses), T(g.disps), T(intr), T(rig), *idx, tgt, camera=camera,
                                         motn_dtype=torch.float32)
    cnh, mnh = slam_ext.reproject_motion_nhwc(T(g.poses), T(g.disps), T(intr), T(rig), *idx, tgt, camera=camera)
    out["motn_f16"], out["motn_f32"], out["motn_nhwc"] = (m16.cpu().numpy().view(np.uint16), m32.cpu().numpy(),
                                                            mnh.cpu().numpy().view(np.uint16))
    out["coords_motion"] = np.stack([c16.cpu().numpy(), c32.cpu().numpy(), cnh.cpu().numpy()])
    for name, opt in (("fused", 0), ("general", slam_ext.BA_OPT_GENERAL_ACCUMULATE)):
        runs = []
        for _ in range(2):
            poses, disps, ii = T(g.poses).clone(), T(g.disps).clone(), T(intr).clone()
            slam_ext.dense_ba(poses, disps, T(g.disps_sens), ii, T(rig), T(g.target.reshape(E, -1, 2)),
                              T(g.weight.reshape(E, -1, 2)), T(g.eta), *idx, t0=1, t1=g.n, n_iters=2, pose_damping=1e-3,
                              pose_ep=0.1, camera=camera, solver_options=opt)
            runs.append((poses.cpu().numpy(), disps.cpu().numpy()))
        out[f"ba_{name}_poses"], out[f"ba_{name}_disps"] = runs[0]
        out[f"ba_{name}_repeatable"] = np.array(all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                                                    for a, b in zip(runs[0], runs[1])))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    arrays = {}
    for cam in CAMERAS:
        for k, v in run_case(cam).items():
            arrays[f"{cam}_{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print("wrote", a.out, {k: (v.shape, str(v.dtype)) for k, v in arrays.items()})
    print({k: bool(v) for k, v in arrays.items() if k.endswith("repeatable")})
