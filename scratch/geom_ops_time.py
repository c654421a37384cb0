"""geom_ops_time.py --parent LIB --change LIB [--rounds N] [--out FILE]: the frame geometry operations of geom_ops.hip,
event-timed under two builds of the library on one device.  The driver itself never opens the GPU: it starts one child
process per (library, round), parent and change alternating, each selecting its library through VIPE_AMD_LIB, and stops at
the first child that fails.  A child times every operation as the median of 5 batches of 100 back-to-back launches after 20
warm-up launches.

Sizes are the headline clip's (bench.py: 200 frames of 512 x 384, every frame a keyframe): the 48 x 64 grid; the
frontend's edge proposal asks for 5 x frontend_window = 125 candidate pairs per keyframe and its keyframe test for one
(frontend.py `_prefetch_proximity` / `_update`, both bidirectional); `extract_slam_map` filters and back-projects all 200
keyframes of the one view in one call each.  The output holds, per operation, the microseconds per launch of every round
under both libraries, the parent's own round-to-round spread (max - min), and whether the change's median lies at or
below the parent's slowest round."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HT, WD, KEYFRAMES, WINDOW, BETA = 48, 64, 200, 25, 0.3


def child():
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from vipe_amd.ext import slam_ext

    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    n = KEYFRAMES
    poses = np.zeros((n, 7), np.float32)  # a smooth trajectory: a few centimetres and a fraction of a degree per keyframe
    poses[:, 0] = 0.02 * np.arange(n)
    poses[:, 2] = 0.005 * np.arange(n)
    half = 0.002 * np.arange(n)
    poses[:, 4], poses[:, 6] = np.sin(half), np.cos(half)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    poses, rig = T(poses), T(np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32))
    disps = T((0.4 + 0.2 * rng.random((n, HT, WD))).astype(np.float32))
    intr_full = T(np.array([[400.0, 400.0, 256.0, 192.0]], np.float32))
    intr8 = (intr_full[0] / 8.0).contiguous()
    t = n - 1
    ii, jj = np.meshgrid(np.arange(t - 5, t, dtype=np.int64), np.arange(t - WINDOW, t, dtype=np.int64), indexing="ij")
    pi, pj = T(ii.reshape(-1)), T(jj.reshape(-1))
    z = torch.zeros_like(pi)
    one = (T(np.array([t - 3])), z[:1], T(np.array([t - 2])), z[:1])
    inds = torch.arange(n, device=dev)
    thresh = torch.full((n,), 0.05, device=dev)
    ops = {}
    for cam in ("pinhole", "panorama"):
        for bidir in (True, False):
            ops[f"frame_distance_rig_{cam}_M{pi.numel()}_bidir{int(bidir)}"] = (
                lambda cam=cam, bidir=bidir: slam_ext.frame_distance_rig(poses, rig, disps, intr_full, pi, z, pj, z, BETA, bidir,
                                                                         camera=cam))
        ops[f"frame_distance_rig_{cam}_M1_bidir1"] = (
            lambda cam=cam: slam_ext.frame_distance_rig(poses, rig, disps, intr_full, *one, BETA, True, camera=cam))
        ops[f"depth_filter_{cam}_n{n}"] = lambda cam=cam: slam_ext.depth_filter(poses, disps, intr8, inds, thresh, camera=cam)
        ops[f"iproj_{cam}_n{n}"] = lambda cam=cam: slam_ext.iproj(poses, disps, intr8, camera=cam)
    out = {}
    for name, op in ops.items():
        for _ in range(20):
            op()
        batches = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(100):
                r = op()
            e1.record()
            torch.cuda.synchronize()
            batches.append(e0.elapsed_time(e1) * 10.0)  # ms per 100 launches -> us per launch
        assert bool(torch.isfinite(r).all()), name
        out[name] = float(np.median(batches))
    print("RESULT " + json.dumps(out))


def driver(a):
    import statistics
    runs = {"parent": [], "change": []}
    for rnd in range(a.rounds):
        for tag, path in (("parent", a.parent), ("change", a.change)):
            env = dict(os.environ, VIPE_AMD_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                               timeout=180)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                sys.exit(f"child ({tag}, round {rnd}) exited with {r.returncode}: stopping")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            runs[tag].append(json.loads(line[7:]))
            print(tag, rnd, line[7:], flush=True)
    table = {}
    for name in runs["parent"][0]:
        p, c = [r[name] for r in runs["parent"]], [r[name] for r in runs["change"]]
        table[name] = {"parent_us": p, "change_us": c, "parent_spread_us": max(p) - min(p), "parent_median_us": statistics.median(p),
                       "change_median_us": statistics.median(c), "within_parent_spread": statistics.median(c) <= max(p)}
    res = {"grid": [HT, WD], "keyframes": KEYFRAMES, "rounds": a.rounds, "operations": table}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)
    print(json.dumps({k: (v["parent_median_us"], v["change_median_us"], v["parent_spread_us"], v["within_parent_spread"])
                      for k, v in table.items()}, indent=1))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--change")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    child() if a.child else driver(a)
