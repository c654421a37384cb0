"""The three stages of `slam_ext.dense_ba_marginals`, event-timed one by one, next to ONE Gauss-Newton iteration of
`dense_ba` on the same inputs: the headline graph (48 keyframes, 48 x 64, E = 276) and a 200-keyframe backend-sized graph.

    python scratch/ba_marginals_time.py [--iters 50] [--out FILE]

Stages: `vipe_dense_ba_linearize` (plan, sensor test, accumulate kernels, export of the damped S), the float64 inverse of
the reduced system in torch (`invert_reduced_system`: cholesky + cholesky_inverse, plumbing), `vipe_dense_ba_marginals`
(ba_disp_variance_kernel + the finish kernel that writes the pose blocks and zeroes S / Hd; the finish kernel is also timed
alone, the variance kernel is the difference).  Events around `--iters` back-to-back calls after 3 warm-up calls.

"bytes" of the variance kernel is what the algorithm has to move: per pixel of a free frame C, the 6 rows of E_kk when the
frame's own pose is free, 6 rows of E_j per term with a free target, the tail rows and the output, each once, against
8 TB/s.  The E rows of both shapes (24 MB / 105 MB) fit the 256 MiB Infinity Cache and in use the accumulate kernels have
just written them, so this is the figure of the real call, not an HBM-streaming figure."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import se3 as ose3  # noqa: E402
from vipe_amd._lib import lib, ptr, stream_ptr  # noqa: E402
from vipe_amd.ext import slam_ext  # noqa: E402
from vipe_amd.synth import make_graph  # noqa: E402

HBM_BPS = 8e12


def event_ms(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def measure(name, gk, bk, iters):
    dev = torch.device("cuda:0")
    g = make_graph(**gk)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    E = len(g.ii)
    z = np.zeros_like(g.ii)
    poses, disps = T(g.poses), T(g.disps)
    args = [poses, disps, T(g.disps_sens), T(g.intrinsics), T(ose3.se3_identity(1)), T(g.target.reshape(E, -1, 2)),
            T(g.weight.reshape(E, -1, 2)), T(g.eta), T(g.ii), T(z), T(g.jj), T(z), T(g.ii)]
    S, info, ctx = slam_ext.dense_ba_linearize(*args, **bk)
    p, ws, (n_poses, V, ht, wd) = ctx
    n = int(S.shape[0])
    Sinv = slam_ext.invert_reduced_system(S)
    dv, pc = slam_ext.dense_ba_marginals_apply(ctx, Sinv)
    L = lib()
    nmax = 6 * n_poses + 1
    Sbuf = torch.empty((nmax, nmax), dtype=torch.float64, device=dev)
    ibuf = torch.zeros(8, dtype=torch.int32, device=dev)
    st = stream_ptr(poses)

    def linearize():
        rc = L.vipe_dense_ba_linearize(ctypes.byref(p), *(ptr(a) for a in args), ptr(ws), ws.numel(), ptr(Sbuf), nmax, ptr(ibuf), st)
        assert rc == 0, rc

    def marg(with_var):
        rc = L.vipe_dense_ba_marginals(ctypes.byref(p), ptr(ws), ptr(Sinv), n, ptr(dv) if with_var else None, ptr(pc), st)
        assert rc == 0, rc

    t_lin = event_ms(linearize, iters)
    t_inv = event_ms(lambda: slam_ext.invert_reduced_system(S), iters)
    linearize()  # the marginals read what a linearize call left
    t_marg = event_ms(lambda: marg(True), iters)
    t_fin = event_ms(lambda: marg(False), iters)
    # one Gauss-Newton iteration of the solver on copies of the same state (in place: the state drifts over the calls, the
    # work per call does not)
    p2, d2 = poses.clone(), disps.clone()
    t_ba = event_ms(lambda: slam_ext.dense_ba(p2, d2, *args[2:], n_iters=1, **bk), iters)
    # algorithmic bytes of the variance kernel
    t0, t1 = bk["t0"], bk["t1"]
    src = np.unique(g.ii)
    fixed = set(src[(src < t0) | (src >= t1)].tolist())
    P = ht * wd
    rows = 0
    for k in src:
        rows += 2 + (0 if int(k) in fixed else 6) + 6 * int(np.sum([int(j) not in fixed for j in g.jj[g.ii == k]]))
    nbytes = 4 * P * rows
    t_var = t_marg - t_fin
    return {"graph": name, "keyframes": g.n, "grid": [ht, wd], "edges": E, "unknowns": n, "iters": iters,
            "linearize_ms": round(t_lin, 4), "torch_inverse_ms": round(t_inv, 4), "marginals_call_ms": round(t_marg, 4),
            "finish_kernel_ms": round(t_fin, 4), "disp_variance_kernel_ms": round(t_var, 4),
            "whole_ms": round(t_lin + t_inv + t_marg, 4), "dense_ba_one_iteration_ms": round(t_ba, 4),
            "variance_kernel_bytes": nbytes, "variance_kernel_GBps": round(nbytes / t_var / 1e6, 1),
            "share_of_8TBps": round(nbytes / (t_var * 1e-3) / HBM_BPS, 4),
            "max_degree": int(np.bincount(g.ii).max()), "var_min_max": [float(dv[torch.isfinite(dv)].min()), float(dv[torch.isfinite(dv)].max())]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bk = dict(pose_damping=1e-3, pose_ep=0.1)
    lines = [measure("headline", dict(n=48, height=384, width=512, radius=3, seed=1234, depth_prior=True), dict(bk, t0=1, t1=48), a.iters),
             measure("backend_200", dict(n=200, height=384, width=512, radius=3, seed=1234, depth_prior=True), dict(bk, t0=1, t1=200), a.iters)]
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        doc = {"what": "stages of slam_ext.dense_ba_marginals on one MI355X, next to one Gauss-Newton iteration of dense_ba on "
                       "the same inputs (the dense_ba kernels are the ones of the parent commit: this change adds entry points "
                       "and does not touch them)",
               "event_timing": lines,
               "event_timing_note": f"events around {a.iters} back-to-back calls after 3 warm-up calls; disp_variance_kernel_ms = "
                                    "marginals_call_ms - finish_kernel_ms; bytes = C, E_kk, E_j, tail and output of the free frames, "
                                    "each once, against the 8 TB/s HBM peak (the rows fit the 256 MiB Infinity Cache).  With "
                                    "SLAMConfig.disp_uncertainty the whole-clip cost is ONE such call per clip.",
               "commands": [f"python scratch/ba_marginals_time.py --iters {a.iters} --out ba_marginals_time.json"]}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
