"""`vipe_cloud_fuse` for a 16-map batch, SLAM size 384 x 512 -> native 1080 x 1920, pinhole, the slanted-plane scene of
scratch/depth_consistency_time.py, event-timed on the current stream: the library's tile-aggregated form and the direct
form (the same source built with -DVIPE_CLOUD_FUSE_LDS_SLOTS=0 into scratch/lib/), strides 1 and 2, with and without
colour, next to a torch composition of the same function (back-projection of the blended maps, `unique`, `index_add`);
and the cost of `SLAMConfig.fused_cloud` on the keep-every-4 clip of bench.py.

    python scratch/cloud_fuse_time.py --build-direct                 (host only: compiles scratch/lib/libcloud_fuse_direct.so)
    python scratch/cloud_fuse_time.py [--iters N] [--sets N] [--frames N] [--no-clip] [--no-kernel]
                                      [--variants conf,cloud] [--out FILE]

A buffer set is the 24 rows of 384 x 512, the 16 x 1080 x 1920 confidence bytes and as many uint8 colour triples
(0.15 GB); the timed loop rotates over --sets of them.  All calls of a variant go into ONE table (2^22 slots, voxel 0.02):
after the warm-up calls every voxel has its slot, which is the state the kernel works in for all but the first frames of
a clip that revisits its scene; counts stay far below the saturation limit (200 calls x a few hundred points per voxel).

"atomic bytes" counts the direct form's global atomics, 4 bytes each: per point the count, the three offsets and - with
colour - three colour sums (zero addends are skipped, about 1 in 256 of the offsets); the guide's chip-wide rate for
shaped float atomics is 1.3 TB/s of added bytes, and it prices scattered one-lane atomics an order of magnitude lower.

Clip cost: `bench.make_clip_runner`'s clip with keep_every=4 (2 * --frames frames), `frame_depth` and `frame_depth_conf`
on, without ("conf") and with ("cloud") `fused_cloud`, alternating, two runs each after one warm-up clip per variant.
`--variants conf --no-kernel` runs on a tree that does not have the flag (the parent commit's)."""
import argparse
import ctypes
import functools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scratch"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import depth_consistency_time as dct  # noqa: E402  (scratch/: the scene and the event timer)

ATOMIC_BPS = 1.3e12
PARAMS, N, H, W = dct.PARAMS, dct.N, dct.H, dct.W
VOXEL, CAP, MIN_AGREE = 0.02, 1 << 22, 2
DIRECT_LIB = os.path.join(ROOT, "scratch", "lib", "libcloud_fuse_direct.so")


def build_direct():
    from vipe_amd import build
    os.makedirs(os.path.dirname(DIRECT_LIB), exist_ok=True)
    cmd = [build.HIPCC, *build.FLAGS, "-DVIPE_CLOUD_FUSE_LDS_SLOTS=0", "-shared", "-o", DIRECT_LIB,
           os.path.join(build.CSRC, "cloud_fuse.hip")]
    subprocess.run(cmd, check=True)
    print("built", DIRECT_LIB)


def make_set(dev, seed):
    from vipe_amd.slam.ingest import depth_consistency
    s = dct.make_set(dev, seed)
    s["conf"] = depth_consistency(s["disp"], s["poses"], s["rig"], s["intr"], "pinhole", PARAMS, s["rows"], s["nbr"], dct.TOL,
                                  out=s.pop("out"))
    gen = torch.Generator(device=dev).manual_seed(seed)
    s["rgb"] = torch.randint(0, 256, (N, PARAMS[4], PARAMS[5], 3), dtype=torch.uint8, device=dev, generator=gen)
    return s


def direct_fuse():
    """`ingest.cloud_fuse`'s call on the direct-form library -> callable(set, table, stride, colour)"""
    from vipe_amd._lib import check, parse_header, ptr, stream_ptr
    L = ctypes.CDLL(DIRECT_LIB)
    fn = L.vipe_cloud_fuse
    fn.restype, fn.argtypes = parse_header()["vipe_cloud_fuse"]
    h1, w1, top, left, H0, W0 = PARAMS

    def call(s, table, stride, colour):
        keys, acc, stats = table
        check(fn(ptr(s["disp"]), ptr(s["poses"]), ptr(s["rig"]), ptr(s["intr"]), 4, 0, ptr(s["rows"]), ptr(s["conf"]), MIN_AGREE,
                 ptr(s["rgb"]) if colour else None, 3, stride, 1.0 / VOXEL, ptr(keys), ptr(acc), keys.shape[0], ptr(stats), N,
                 s["disp"].shape[0], 1, H, W, h1, w1, top, left, H0, W0, stream_ptr(keys)), "vipe_cloud_fuse (direct form)")
    return call


def shipped_fuse(s, table, stride, colour):
    from vipe_amd.slam.ingest import cloud_fuse
    cloud_fuse(s["disp"], s["poses"], s["rig"], s["intr"], "pinhole", PARAMS, s["rows"], table, VOXEL, conf=s["conf"],
               min_agree=MIN_AGREE, rgb=s["rgb"] if colour else None, stride=stride)


def torch_composition(s, stride, colour):
    """the same cloud as torch operators (pinhole, one view, identity rotations): -> (keys, sums [K,7] int64)"""
    h1, w1, top, left, H0, W0 = PARAMS
    disp, rows = s["disp"], s["rows"]
    fx, fy, cx, cy = s["intr"][0]
    pad = (left, w1 - W - left, top, h1 - H - top)
    d = F.interpolate(F.pad(disp[rows][:, None], pad, mode="replicate"), size=(H0, W0), mode="bilinear", align_corners=False)[:, 0]
    gx = torch.arange(W, device=disp.device, dtype=torch.float32).view(1, 1, 1, W).expand(1, 1, H, W)
    gy = torch.arange(H, device=disp.device, dtype=torch.float32).view(1, 1, H, 1).expand(1, 1, H, W)
    u = F.interpolate(F.pad(gx, pad, mode="replicate"), size=(H0, W0), mode="bilinear", align_corners=False)[0, 0]
    v = F.interpolate(F.pad(gy, pad, mode="replicate"), size=(H0, W0), mode="bilinear", align_corners=False)[0, 0]
    keep = (d > 0) & ((s["conf"] & 15) >= MIN_AGREE)
    if stride > 1:
        grid = torch.zeros(H0, W0, dtype=torch.bool, device=disp.device)
        grid[::stride, ::stride] = True
        keep &= grid
    centre = -s["poses"][rows, :3]  # pure translations
    pts = torch.stack([(u - cx) / fx / d, (v - cy) / fy / d, 1.0 / d], -1) + centre[:, None, None, :]
    sv = pts[keep] * (1.0 / VOXEL)
    idx = torch.floor(sv)
    q = torch.clamp(((sv - idx) * 256.0).long(), max=255)
    ii = idx.long() + (1 << 20)
    key = ii[:, 0] | (ii[:, 1] << 21) | (ii[:, 2] << 42)
    keys, inv = torch.unique(key, return_inverse=True)
    vals = [torch.ones_like(q[:, :1]), q] + ([s["rgb"][keep].long()] if colour else [])
    vals = torch.cat(vals, 1)
    sums = torch.zeros(keys.shape[0], vals.shape[1], dtype=torch.int64, device=disp.device)
    sums.index_add_(0, inv, vals)
    return keys, sums


def kernel_figures(args, dev):
    import cloud_fuse_reference as cf
    from vipe_amd.slam.ingest import cloud_table
    sets = [make_set(dev, i) for i in range(args.sets)]
    forms = {"tile_aggregated": shipped_fuse}
    if os.path.exists(DIRECT_LIB):
        forms["direct"] = direct_fuse()
    out = {"shape": {"N": N, "R": sets[0]["disp"].shape[0], "H": H, "W": W, "params_h1_w1_top_left_H0_W0": list(PARAMS),
                     "camera": "pinhole", "voxel": VOXEL, "capacity": CAP, "min_agree": MIN_AGREE},
           "iters": args.iters, "buffer_sets": args.sets, "variants": {}}
    for stride in (1, 2):
        for colour in (True, False):
            name = f"stride{stride}_{'colour' if colour else 'no_colour'}"
            row = {}
            tables = {}
            for form, fn in forms.items():
                # one launch into a fresh table: what the forms must agree on, and the counts of the shape
                fresh = cloud_table(CAP, dev)
                fn(sets[0], fresh, stride, colour)
                torch.cuda.synchronize()
                tables[form] = tuple(x.cpu().numpy() for x in fresh)
                table = cloud_table(CAP, dev)
                row[f"{form}_ms"] = round(dct.event_ms(lambda i: fn(sets[i % args.sets], table, stride, colour), args.iters), 5)
                row[f"{form}_table_load_after_all_sets"] = round(float((table[0] != -1).float().mean()), 4)
            k, s_, _ = cf.table_rows(*tables["tile_aggregated"][:2])
            stats = [int(x) for x in tables["tile_aggregated"][2]]
            row.update(points_per_call=stats[0], voxels_per_call=int(k.shape[0]), counters_one_call=stats)
            if "direct" in tables:
                kd, sd, _ = cf.table_rows(*tables["direct"][:2])
                row["forms_leave_the_same_table"] = bool((k == kd).all() and (s_ == sd).all()
                                                         and stats == [int(x) for x in tables["direct"][2]])
                nbytes = stats[0] * (7 if colour else 4) * 4
                row["direct_atomic_bytes"] = nbytes
                row["direct_atomic_GBps"] = round(nbytes / row["direct_ms"] / 1e6, 1)
                row["direct_share_of_1.3TBps"] = round(nbytes / (row["direct_ms"] * 1e-3) / ATOMIC_BPS, 4)
                row["direct_over_tile_aggregated"] = round(row["direct_ms"] / row["tile_aggregated_ms"], 2)
            row["Mpoints_per_s"] = round(stats[0] / row["tile_aggregated_ms"] / 1e3, 1)
            t_torch = dct.event_ms(lambda i: torch_composition(sets[i % args.sets], stride, colour), max(3, args.iters // 40), warm=1)
            tk, ts = torch_composition(sets[0], stride, colour)
            row["torch_composition_ms"] = round(t_torch, 4)
            row["torch_over_hip"] = round(t_torch / row["tile_aggregated_ms"], 2)
            row["torch_voxels"] = int(tk.shape[0])  # float32 torch arithmetic rounds a few points into the neighbouring voxel
            out["variants"][name] = row
            print(json.dumps({name: row}), flush=True)
    return out


def clip_figures(args, dev):
    import bench
    from vipe_amd.slam import ingest, system
    from vipe_amd.slam.factor_graph import warm_volume_pool
    real = system.SLAMConfig
    base = dict(frame_depth=True, frame_depth_conf=True)
    flags = {"conf": base, "cloud": dict(base, fused_cloud=True)}
    names = args.variants.split(",")
    runs = {}
    for name in names:
        system.SLAMConfig = functools.partial(real, **flags[name])
        try:
            runs[name] = bench.make_clip_runner(dev)
        finally:
            system.SLAMConfig = real
    seen = {"fuse": 0, "cloud": None}
    real_fuse, real_extract = getattr(ingest, "cloud_fuse", None), getattr(ingest, "cloud_extract", None)
    if real_fuse is not None:
        def counted(*a, **k):
            seen["fuse"] += 1
            return real_fuse(*a, **k)

        def extract(table, *a, **k):
            res = real_extract(table, *a, **k)
            seen["cloud"] = dict(voxels_found=res[4], counters=table[2].tolist(), table_load=round(float((table[0] != -1).float().mean()), 4))
            return res
        ingest.cloud_fuse, ingest.cloud_extract = counted, extract

    def one(name, seed, n):
        seen["fuse"], seen["cloud"] = 0, None
        r = runs[name](seed=seed, n_frames=n, keep_every=4)
        r["fuse_launches"], r["cloud"] = seen["fuse"], seen["cloud"]
        return r

    for name in names:
        one(name, 10_000, 48)
    torch.cuda.empty_cache()
    warm_volume_pool(dev)
    one(names[0], 10_001, 2 * args.frames)
    res = {name: [] for name in names}
    for _ in range(2):
        for name in names:
            r = one(name, 1, 2 * args.frames)
            res[name].append({"frames_per_s": round(r["frames"] / r["seconds"], 2), "seconds": round(r["seconds"], 4),
                              "pass2_seconds": round(r["seconds_to_pass2_done"] - r["seconds_to_global_ba_done"], 4),
                              "keyframes": r["keyframes"], "frames": r["frames"], "state_finite": r["finite"],
                              "fuse_launches": r["fuse_launches"], "cloud": r["cloud"]})
    return {"runs": res, "frames_per_s_best": {k: max(x["frames_per_s"] for x in v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-clip", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--build-direct", action="store_true")
    ap.add_argument("--variants", default="conf,cloud")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.build_direct:
        return build_direct()
    dev = torch.device("cuda:0")
    line = {}
    if not args.no_kernel:
        line["kernel"] = kernel_figures(args, dev)
    if not args.no_clip:
        line["clip"] = clip_figures(args, dev)
        print(json.dumps({"clip": line["clip"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_cloud_fuse, 16 maps 384 x 512 -> 1080 x 1920, pinhole, gated by vipe_depth_consistency's bytes "
                       "(min_agree 2), voxel 0.02, 2^22 slots, one MI355X: the tile-aggregated form (the library's) and the "
                       "direct form, next to a torch composition; and the keep-every-4 clip of bench.py (make_clip_runner, "
                       "384 x 512) with frame_depth and frame_depth_conf on, fused_cloud off ('conf') / on ('cloud')",
               "event_timing": line.get("kernel"),
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls, rotating over "
                                    f"{args.sets} buffer sets, all into one table per variant and form; the torch composition "
                                    "is timed over a fortieth of the calls",
               "clip": line.get("clip"),
               "clip_note": "frames / wall time of SLAMSystem.run, 2 runs per variant alternating after a warm-up clip per "
                            "variant and one full-length clip; maps at SLAM resolution kept on the device; the clip's frames "
                            "are random images, so few pixels pass the gate",
               "commands": ["python scratch/cloud_fuse_time.py --build-direct",
                            f"python scratch/cloud_fuse_time.py --iters {args.iters} --sets {args.sets} --frames {args.frames} "
                            "--out profiles/cloud_fuse_time.json"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
