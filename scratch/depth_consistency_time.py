"""`vipe_depth_consistency` for a 16-map batch, SLAM size 384 x 512 -> native 1080 x 1920, K = 4 neighbours, pinhole,
event-timed on the current stream next to a torch composition of the same function on the same inputs (F.pad(replicate)
+ F.interpolate for the blend and the source coordinates, the transforms as small matrix products, four index gathers
per neighbour, no custom kernel); and the cost of `SLAMConfig.frame_depth_conf` on the keep-every-4 clip of bench.py.

    python scratch/depth_consistency_time.py [--iters N] [--sets N] [--frames N] [--no-clip] [--no-kernel]
                                             [--variants depth,conf] [--out FILE]

Geometry as scratch/depth_export_time.py: (h1, w1) = (388, 518), top = 2, left = 3.  A buffer set is 24 rows of 384 x 512
(8 "keyframes" and the 16 source maps, 18.9 MB) and the 16 x 1080 x 1920 bytes written (33.2 MB); the timed loop rotates
over --sets of them (default 8: 0.42 GB) so that a set has left the 256 MiB Infinity Cache before it is used again.  The
scene is a slanted plane seen from cameras 0.05 units apart, so that nearly every pair is visible and takes all four taps.

"bytes" is what the algorithm has to move: each source map and its K neighbour maps once (N (1 + K) H W 4 B), the
output once (N H0 W0 B), against 8 TB/s of HBM.

Clip cost: `bench.make_clip_runner`'s clip with keep_every=4 (2 * --frames frames), `frame_depth` on, without ("depth")
and with ("conf") `frame_depth_conf`, alternating, two runs each after one warm-up clip per variant.  bench.py itself is
not changed: a variant hands it a SLAMConfig with the flags preset.  `--variants depth --no-kernel` runs on a tree that
does not have the flag (the parent commit's), for the alternation of that tree against this one on one library."""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

HBM_BPS = 8e12
PARAMS = (388, 518, 2, 3, 1080, 1920)
N, K, N_KF, H, W = 16, 4, 8, 384, 512
TOL = 0.05


def event_ms(fn, iters, warm=3):
    for i in range(warm):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def make_set(dev, seed):
    """24 slots on a line, 0.05 units apart, looking at the plane z = 4 + 0.3 x: exact disparities per slot, 2 % noise"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    R = N_KF + N
    fx = fy = 0.9 * W
    cx, cy = W / 2 - 0.3, H / 2 + 0.2
    intr = torch.tensor([[fx, fy, cx, cy]], device=dev)
    tx = 0.05 * (torch.arange(R, device=dev, dtype=torch.float32) - R / 2)
    poses = torch.zeros(R, 7, device=dev)
    poses[:, 0], poses[:, 6] = -tx, 1.0  # world -> camera of a camera at (tx, 0, 0)
    u = (torch.arange(W, device=dev, dtype=torch.float32) - cx) / fx
    # the ray (u, v, 1) s from (tx, 0, 0) meets z = 4 + 0.3 x at s = (4 + 0.3 tx) / (1 - 0.3 u)
    depth = (4 + 0.3 * tx)[:, None, None] / (1 - 0.3 * u)[None, None, :].expand(R, H, W)
    disp = (1.0 / depth) * (1 + 0.02 * torch.randn(R, H, W, device=dev, generator=gen))
    rows = torch.arange(N_KF, R, device=dev)
    nbr = torch.stack([torch.arange(N_KF, device=dev)[(i + torch.arange(K, device=dev)) % N_KF] for i in range(N)])
    rig = torch.tensor([[0, 0, 0, 0, 0, 0, 1.0]], device=dev)
    out = torch.empty(N, PARAMS[4], PARAMS[5], dtype=torch.uint8, device=dev)
    return dict(disp=disp.contiguous(), poses=poses, rig=rig, intr=intr, rows=rows, nbr=nbr.contiguous(), out=out)


def _rot(q):
    x, y, z, w = q.unbind(-1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                        2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                        2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).view(*q.shape[:-1], 3, 3)


def torch_composition(s):
    """the same bytes as torch operators (pinhole, one view, identity rig): -> [N,H0,W0] uint8"""
    h1, w1, top, left, H0, W0 = PARAMS
    disp, rows, nbr = s["disp"], s["rows"], s["nbr"]
    fx, fy, cx, cy = s["intr"][0]
    pad = (left, w1 - W - left, top, h1 - H - top)
    d = F.interpolate(F.pad(disp[rows][:, None], pad, mode="replicate"), size=(H0, W0), mode="bilinear", align_corners=False)[:, 0]
    gx = torch.arange(W, device=disp.device, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W)
    gy = torch.arange(H, device=disp.device, dtype=torch.float32).view(1, 1, H, 1).expand(1, 1, H, W)
    u = F.interpolate(F.pad(gx, pad, mode="replicate"), size=(H0, W0), mode="bilinear", align_corners=False)[0, 0]
    v = F.interpolate(F.pad(gy, pad, mode="replicate"), size=(H0, W0), mode="bilinear", align_corners=False)[0, 0]
    X0, Y0 = (u - cx) / fx, (v - cy) / fy
    Rw, tw = _rot(s["poses"][:, 3:]), s["poses"][:, :3]
    agree = torch.zeros(N, H0, W0, dtype=torch.uint8, device=disp.device)
    visible = torch.zeros_like(agree)
    flat = disp.view(disp.shape[0], -1)
    for k in range(K):
        q = nbr[:, k]
        Rq, Rr = Rw[q], Rw[rows]
        Rm = Rq @ Rr.transpose(1, 2)
        t = tw[q] - (Rm @ tw[rows][:, :, None])[:, :, 0]
        X = [Rm[:, i, 0, None, None] * X0 + Rm[:, i, 1, None, None] * Y0 + Rm[:, i, 2, None, None] + t[:, i, None, None] * d
             for i in range(3)]
        ok = (X[2] > 0.1) & (d > 0)
        Z = torch.where(X[2] < 0.1, torch.ones_like(X[2]), X[2])
        xp, yp = fx * (X[0] / Z) + cx, fy * (X[1] / Z) + cy
        dq = d / X[2]
        x0, y0 = torch.floor(xp), torch.floor(yp)
        vis = ok & (x0 >= 0) & (x0 <= W - 2) & (y0 >= 0) & (y0 <= H - 2)
        base = (torch.where(vis, y0, torch.zeros_like(y0)) * W + torch.where(vis, x0, torch.zeros_like(x0))).long()
        rowsq = flat[q]
        hit = torch.zeros_like(vis)
        for off in (0, 1, W, W + 1):
            tap = torch.gather(rowsq, 1, (base + off).view(N, -1)).view(N, H0, W0)
            hit |= (tap > 0) & ((dq - tap).abs() <= TOL * dq)
        visible += vis.to(torch.uint8)
        agree += (hit & vis).to(torch.uint8)
    return agree | (visible << 4)


def kernel_figures(args, dev):
    import depth_consistency_reference as cr
    from vipe_amd.slam.ingest import depth_consistency
    from vipe_amd.slam.interface import unpack_depth_conf
    sets = [make_set(dev, i) for i in range(args.sets)]

    def hip(s):
        return depth_consistency(s["disp"], s["poses"], s["rig"], s["intr"], "pinhole", PARAMS, s["rows"], s["nbr"], TOL, out=s["out"])

    t_hip = event_ms(lambda i: hip(sets[i % args.sets]), args.iters)
    t_hip_hot = event_ms(lambda i: hip(sets[0]), args.iters)
    t_torch = event_ms(lambda i: torch_composition(sets[i % args.sets]), max(5, args.iters // 20))
    s = sets[0]
    got = hip(s)
    tc = torch_composition(s)
    torch.cuda.synchronize()
    agree, visible = unpack_depth_conf(got)
    differ = float((got != tc).float().mean())
    # two maps against the float64 reference under the tests' criterion
    sub = dict(disp=s["disp"].cpu().numpy(), poses=s["poses"].cpu().numpy(), rig=s["rig"].cpu().numpy(),
               intrinsics=s["intr"].cpu().numpy(), camera="pinhole", params=PARAMS, rows=s["rows"][:2].cpu().numpy(),
               nbr=s["nbr"][:2].cpu().numpy(), tol=TOL)
    ref = cr.depth_consistency_ref(**sub)
    exact, loose = cr.compare(got[:2].cpu().numpy(), ref)
    nbytes = N * ((1 + K) * H * W * 4 + PARAMS[4] * PARAMS[5])
    return {"shape": {"N": N, "K": K, "R": N_KF + N, "H": H, "W": W, "params_h1_w1_top_left_H0_W0": list(PARAMS), "camera": "pinhole"},
            "iters": args.iters, "buffer_sets": args.sets, "hip_ms": round(t_hip, 5), "hip_ms_one_buffer_set": round(t_hip_hot, 5),
            "bytes": nbytes, "hip_GBps": round(nbytes / t_hip / 1e6, 1), "share_of_8TBps": round(nbytes / (t_hip * 1e-3) / HBM_BPS, 4),
            "share_of_8TBps_one_buffer_set": round(nbytes / (t_hip_hot * 1e-3) / HBM_BPS, 4),
            "torch_composition_ms": round(t_torch, 5), "torch_over_hip": round(t_torch / t_hip, 2),
            "mean_visible": round(float(visible.float().mean()), 3), "mean_agree": round(float(agree.float().mean()), 3),
            "share_of_bytes_differing_from_torch_f32": differ,
            "reference_2_maps": {"pixels_exact": exact, "pixels_with_undecided_pairs": loose, "pairs": cr.summary(ref)}}


def clip_figures(args, dev):
    import bench
    from vipe_amd.slam import system
    from vipe_amd.slam.factor_graph import warm_volume_pool
    real = system.SLAMConfig
    flags = {"depth": dict(frame_depth=True), "conf": dict(frame_depth=True, frame_depth_conf=True)}
    names = args.variants.split(",")
    runs = {}
    for name in names:
        system.SLAMConfig = functools.partial(real, **flags[name])
        try:
            runs[name] = bench.make_clip_runner(dev)
        finally:
            system.SLAMConfig = real

    from vipe_amd.slam import ingest
    launches = {"n": 0}
    real_conf = getattr(ingest, "depth_consistency", None)
    if real_conf is not None:
        def counted(*a, **k):
            launches["n"] += 1
            return real_conf(*a, **k)
        ingest.depth_consistency = counted

    def one(name, seed, n):
        launches["n"] = 0
        r = runs[name](seed=seed, n_frames=n, keep_every=4)
        r["conf_launches"] = launches["n"]
        return r

    for name in names:
        one(name, 10_000, 48)
    torch.cuda.empty_cache()
    warm_volume_pool(dev)
    one(names[0], 10_001, 2 * args.frames)  # the process has held the backend's memory before the timed clips
    res = {name: [] for name in names}
    for _ in range(2):
        for name in names:
            r = one(name, 1, 2 * args.frames)
            res[name].append({"frames_per_s": round(r["frames"] / r["seconds"], 2), "seconds": round(r["seconds"], 4),
                              "pass2_seconds": round(r["seconds_to_pass2_done"] - r["seconds_to_global_ba_done"], 4),
                              "keyframes": r["keyframes"], "frames": r["frames"], "state_finite": r["finite"],
                              "conf_launches": r["conf_launches"]})
    return {"runs": res, "frames_per_s_best": {k: max(x["frames_per_s"] for x in v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-clip", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--variants", default="depth,conf")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {}
    if not args.no_kernel:
        line["kernel"] = kernel_figures(args, dev)
        print(json.dumps(line), flush=True)
    if not args.no_clip:
        line["clip"] = clip_figures(args, dev)
        print(json.dumps({"clip": line["clip"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_depth_consistency, 16 maps 384 x 512 -> 1080 x 1920, K = 4, pinhole, one MI355X, next to a torch "
                       "composition of the same function on the same inputs; and the keep-every-4 clip of bench.py "
                       "(make_clip_runner, 384 x 512) with SLAMConfig.frame_depth on, frame_depth_conf off ('depth') / on ('conf')",
               "event_timing": line.get("kernel"),
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls, rotating over "
                                    f"{args.sets} buffer sets (52 MB each: a set leaves the 256 MiB Infinity Cache before it is "
                                    "used again); *_one_buffer_set: the same calls on one set, which the Infinity Cache holds - "
                                    "not an HBM figure.  bytes = source maps + K neighbour maps + output, each once; shares are "
                                    "of the 8 TB/s HBM peak.  The torch composition is timed over a twentieth of the calls",
               "clip": line.get("clip"),
               "clip_note": "frames / wall time of SLAMSystem.run, 2 runs per variant alternating after a warm-up clip per "
                            "variant and one full-length clip; maps at SLAM resolution kept on the device",
               "commands": [f"python scratch/depth_consistency_time.py --iters {args.iters} --sets {args.sets} --frames {args.frames} "
                            "--out profiles/depth_consistency_time.json"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
