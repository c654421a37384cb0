"""`vipe_depth_export` for a 16-map batch, SLAM size 384 x 512 -> native 1080 x 1920, fp16 out, event-timed on the current
stream next to the torch composition on the same inputs (F.pad(replicate) + F.interpolate(bilinear) + reciprocal +
.half()); and the cost of `SLAMConfig.frame_depth` on the keep-every-4 clip of bench.py.

    python scratch/depth_export_time.py [--iters N] [--sets N] [--frames N] [--no-clip] [--out FILE]

384 x 512 and 1080 x 1920 do not share an aspect ratio, so the maps are placed as a `StandardResize` would place them
with a crop band of 2 | 2 rows and 3 | 3 columns: (h1, w1) = (388, 518), top = 2, left = 3.

"bytes" is what the algorithm has to move: the disparities once (H*W*4 B per map), the output once (H0*W0*2 B per
map), against 8 TB/s of HBM.  One buffer set (12.6 MB in, 66.4 MB out) fits the 256 MiB Infinity Cache, so back-to-back
calls on ONE set are not an HBM figure: the timed loop rotates over enough sets (--sets, default 8: 0.63 GB) that a set
is evicted before it is used again.  The largest error / bound ratio against the float64 reference
(tests/depth_export_reference.py) is reported for a 2-map slice with fp32 output.

Clip cost: `bench.make_clip_runner`'s clip with keep_every=4 (2 * --frames frames, --frames default 200, as bench.py's
"keep_one_in_four"), `frame_depth` off and on, alternating, two runs each after one warm-up clip per variant.  bench.py
itself is not changed: the "on" variant hands it a SLAMConfig with the flag preset."""
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

import depth_export_reference as dr  # noqa: E402
from vipe_amd.slam.ingest import depth_export  # noqa: E402

HBM_BPS = 8e12
PARAMS = (388, 518, 2, 3, 1080, 1920)
N, H, W = 16, 384, 512


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


def kernel_figures(args, dev):
    gen = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(args.sets):
        disp = 1.0 / (1.0 + 4.0 * torch.rand(N, H, W, generator=gen, device=dev))
        sets.append((disp, torch.empty(N, PARAMS[4], PARAMS[5], dtype=torch.float16, device=dev)))
    t_hip = event_ms(lambda i: depth_export(sets[i % args.sets][0], PARAMS, out=sets[i % args.sets][1]), args.iters)
    t_hip_hot = event_ms(lambda i: depth_export(sets[0][0], PARAMS, out=sets[0][1]), args.iters)
    t_torch = event_ms(lambda i: dr.torch_composition(sets[i % args.sets][0], PARAMS).half(), max(10, args.iters // 10))
    disp, out = sets[0]
    depth_export(disp, PARAMS, out=out)
    f32 = depth_export(disp[:2], PARAMS, dtype=torch.float32)
    torch.cuda.synchronize()
    dn = disp[:2].cpu().numpy()
    ref, bound = dr.depth_export_ref(dn, PARAMS), dr.depth_bound(dn, PARAMS)
    ratio = float((np.abs(f32.cpu().numpy().astype(np.float64) - ref) / bound).max())
    tc = dr.torch_composition(disp, PARAMS)
    vs_torch = float(((out.float() - tc.half().float()).abs() / tc).max())
    nbytes = N * (H * W * 4 + PARAMS[4] * PARAMS[5] * 2)
    return {"shape": {"N": N, "H": H, "W": W, "params_h1_w1_top_left_H0_W0": list(PARAMS), "out": "float16"},
            "iters": args.iters, "buffer_sets": args.sets, "hip_ms": round(t_hip, 5),
            "hip_ms_one_buffer_set": round(t_hip_hot, 5), "bytes": nbytes, "hip_GBps": round(nbytes / t_hip / 1e6, 1),
            "share_of_8TBps": round(nbytes / (t_hip * 1e-3) / HBM_BPS, 4),
            "share_of_8TBps_one_buffer_set": round(nbytes / (t_hip_hot * 1e-3) / HBM_BPS, 4),
            "torch_composition_ms": round(t_torch, 5), "torch_over_hip": round(t_torch / t_hip, 2),
            "max_err_over_bound_f32": round(ratio, 4), "max_rel_diff_vs_torch_f16": vs_torch}


def clip_figures(args, dev):
    import bench
    from vipe_amd.slam import system
    from vipe_amd.slam.factor_graph import warm_volume_pool
    real = system.SLAMConfig
    runs = {}
    for name, cls in (("off", real), ("on", functools.partial(real, frame_depth=True))):
        system.SLAMConfig = cls
        try:
            runs[name] = bench.make_clip_runner(dev)
        finally:
            system.SLAMConfig = real

    from vipe_amd.slam import ingest
    launches = {"n": 0}
    real_export = ingest.depth_export

    def counted(*a, **k):
        launches["n"] += 1
        return real_export(*a, **k)
    ingest.depth_export = counted

    def one(name, seed, n):  # (make_clip_runner bound its SLAMConfig when it was made)
        launches["n"] = 0
        r = runs[name](seed=seed, n_frames=n, keep_every=4)
        r["export_launches"] = launches["n"]
        return r

    for name in ("off", "on"):
        one(name, 10_000, 48)
    torch.cuda.empty_cache()
    warm_volume_pool(dev)
    one("off", 10_001, 2 * args.frames)  # the process has held the backend's memory before the timed clips
    res = {"off": [], "on": []}
    for _ in range(2):
        for name in ("off", "on"):
            r = one(name, 1, 2 * args.frames)
            res[name].append({"frames_per_s": round(r["frames"] / r["seconds"], 2), "seconds": round(r["seconds"], 4),
                              "pass2_seconds": round(r["seconds_to_pass2_done"] - r["seconds_to_global_ba_done"], 4),
                              "keyframes": r["keyframes"], "frames": r["frames"], "state_finite": r["finite"],
                              "export_launches": r["export_launches"]})
    best = {k: max(x["frames_per_s"] for x in v) for k, v in res.items()}
    return {"runs": res, "frames_per_s_best": best, "on_over_off_seconds": round(best["off"] / best["on"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-clip", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {"kernel": kernel_figures(args, dev)}
    print(json.dumps(line), flush=True)
    if not args.no_clip:
        line["clip"] = clip_figures(args, dev)
        print(json.dumps({"clip": line["clip"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_depth_export, 16 maps 384 x 512 -> 1080 x 1920, fp16 out, one MI355X, next to the torch "
                       "composition (F.pad replicate + F.interpolate bilinear + reciprocal + .half()) on the same inputs; and "
                       "the keep-every-4 clip of bench.py (make_clip_runner, 384 x 512) with SLAMConfig.frame_depth off / on",
               "event_timing": line["kernel"],
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls, rotating over "
                                    f"{args.sets} buffer sets (79 MB each: a set leaves the 256 MiB Infinity Cache before it is "
                                    "used again); *_one_buffer_set: the same calls on one set, which the Infinity Cache holds - "
                                    "not an HBM figure.  bytes = disparities + output, each once; shares are of the 8 TB/s HBM "
                                    "peak.  The torch composition is timed over a tenth of the calls",
               "clip": line.get("clip"),
               "clip_note": "frames / wall time of SLAMSystem.run, 2 runs per variant alternating off / on after a warm-up "
                            "clip per variant and one full-length clip; 'on' = frame_depth (dense pass 2, upsampling of every "
                            "chunk, one export launch per chunk, fp16 maps at SLAM resolution kept on the device)",
               "commands": [f"python scratch/depth_export_time.py --iters {args.iters} --sets {args.sets} --frames {args.frames} "
                            "--out profiles/depth_export_time.json"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
