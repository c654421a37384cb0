"""panorama_time.py [--out FILE]: one Gauss-Newton iteration of the dense BA with the panorama camera against the pinhole
camera on the same graph shape (64 x 128 grid of BASELINE.json's 1024 x 512 configuration, N keyframes, radius-3 edges),
event-timed on one device: whole iterations (events around `calls` back-to-back dense_ba calls of `iters` iterations after
3 warm-up calls) and the accumulate launch alone (vipe_ba_params.profile_ev0 / ev1 around the last iteration's)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vipe_amd.ext import slam_ext  # noqa: E402
from vipe_amd.synth import make_graph, make_panorama_graph  # noqa: E402


def timed(camera, n, opts, calls, iters):
    dev = torch.device("cuda:0")
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    if camera == "panorama":
        g = make_panorama_graph(n=n, height=512, width=1024, radius=3, seed=1, step_length=0.1)
        pi, qi, pj, qj, di, intr = g.pi, g.qi, g.pj, g.qj, g.di, g.intrinsics
    else:
        g = make_graph(n=n, height=512, width=1024, radius=3, seed=1)
        z = np.zeros_like(g.ii)
        pi, qi, pj, qj, di, intr = g.ii, z, g.jj, z, g.ii, g.intrinsics
    M = len(pi)
    fixed = (T(g.disps_sens), T(intr), T(np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)), T(g.target.reshape(M, -1, 2)),
             T(g.weight.reshape(M, -1, 2)), T(g.eta), T(pi), T(qi), T(pj), T(qj), T(di))
    p0, d0 = T(g.poses), T(g.disps.reshape(-1, g.ht, g.wd))
    kw = dict(t0=1, t1=n, n_iters=iters, pose_damping=1e-3, pose_ep=0.1, camera=camera, solver_options=opts)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    for e in ev:
        e.record()
    acc = []
    for c in range(3 + calls):
        poses, disps = p0.clone(), d0.clone()
        if c == 3:
            ev[0].record()
        slam_ext.dense_ba(poses, disps, *fixed, **kw)
    ev[1].record()
    for _ in range(10):
        poses, disps = p0.clone(), d0.clone()
        slam_ext.dense_ba(poses, disps, *fixed, profile_events=(ev[2], ev[3]), **kw)
        torch.cuda.synchronize()
        acc.append(ev[2].elapsed_time(ev[3]))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(poses).all())
    return {"camera": camera, "form": "general" if opts else "fused", "keyframes": n, "terms": int(M), "grid": [g.ht, g.wd],
            "iteration_ms": ev[0].elapsed_time(ev[1]) / (calls * iters), "accumulate_ms_median": float(np.median(acc))}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--keyframes", type=int, default=12)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--iters", type=int, default=3)
    a = ap.parse_args()
    rows = [timed(cam, a.keyframes, opts, a.calls, a.iters) for opts in (0, slam_ext.BA_OPT_GENERAL_ACCUMULATE)
            for cam in ("pinhole", "panorama")]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        json.dump({"ba_iteration": rows}, open(a.out, "w"), indent=1)
