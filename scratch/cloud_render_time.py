"""`vipe_cloud_render` for the cloud scratch/cloud_fuse_time.py fuses (one 16-map call at stride 1 with colour: about
6.5e5 points of voxel 0.02) drawn into that call's 16 cameras at 1080 x 1920, event-timed on the current stream: the
library's form (a plain load in front of every atomic) and the always-atomic form (the same source built with
-DVIPE_CLOUD_RENDER_PRELOAD=0 into scratch/lib/), max_radius 0 and 2, next to a torch composition of the same function
(projection in torch, packed int64 keys, one `scatter_reduce_(amin)` per footprint offset); `vipe_cloud_resolve`; and the
cost of `SLAMConfig.fused_depth` on the keep-every-4 clip of bench.py.

    python scratch/cloud_render_time.py --build-always               (host only: compiles scratch/lib/libcloud_render_always.so)
    python scratch/cloud_render_time.py [--iters N] [--sets N] [--frames N] [--no-clip] [--no-kernel]
                                        [--variants cloud,depth] [--out FILE]

A render starts from an EMPTY z-buffer - a filled one lets the library's form skip nearly every atomic - so a timed
call is `fill_(-1)` + render, rotating over --sets z-buffers of 16 x 1080 x 1920 x 8 B (0.27 GB each); the fill alone is
timed the same way and subtracted ("render_ms").  "atomics" counts the (point, image, footprint pixel) triples, 8 bytes
each: what the always-atomic form issues; DESIGN.md section 18 measured 82-96 GB/s for scattered one-lane 4-byte
atomics.

Clip cost: `bench.make_clip_runner`'s clip with keep_every=4 (2 * --frames frames), `frame_depth`, `frame_depth_conf` and
`fused_cloud` on, without ("cloud") and with ("depth") `fused_depth`, alternating, two runs each after one warm-up clip
per variant.  `--variants cloud --no-kernel` runs on a tree that does not have the flag (the parent commit's)."""
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

import cloud_fuse_time as cft  # noqa: E402  (scratch/: the scene, its cloud)
import depth_consistency_time as dct  # noqa: E402  (scratch/: the event timer)

PARAMS, N, H, W = dct.PARAMS, dct.N, dct.H, dct.W
GEOM = (H, W, *PARAMS)
VOXEL = cft.VOXEL
ALWAYS_LIB = os.path.join(ROOT, "scratch", "lib", "libcloud_render_always.so")


def build_always():
    from vipe_amd import build
    os.makedirs(os.path.dirname(ALWAYS_LIB), exist_ok=True)
    cmd = [build.HIPCC, *build.FLAGS, "-DVIPE_CLOUD_RENDER_PRELOAD=0", "-shared", "-o", ALWAYS_LIB,
           os.path.join(build.CSRC, "cloud_render.hip")]
    subprocess.run(cmd, check=True)
    print("built", ALWAYS_LIB)


def make_scene(dev):
    """the cloud of one `cloud_fuse` call of scratch/cloud_fuse_time.py and the 16 cameras of its maps"""
    from vipe_amd.slam.ingest import cloud_extract, cloud_table
    s = cft.make_set(dev, 0)
    table = cloud_table(cft.CAP, dev)
    cft.shipped_fuse(s, table, 1, True)
    xyz, rgb, _, key, _ = cloud_extract(table, VOXEL, min_count=1)
    order = torch.argsort(key)
    return dict(xyz=xyz[order].contiguous(), rgb=rgb[order].contiguous(), cams=s["poses"][s["rows"]].contiguous(),
                intr=s["intr"].expand(N, -1).contiguous())


def always_render():
    """`ingest.cloud_render`'s call on the always-atomic library -> callable(scene, zbuf, stats, max_radius)"""
    from vipe_amd._lib import check, parse_header, ptr, stream_ptr
    fn = ctypes.CDLL(ALWAYS_LIB).vipe_cloud_render
    fn.restype, fn.argtypes = parse_header()["vipe_cloud_render"]

    def call(sc, zbuf, stats, max_radius):
        check(fn(ptr(sc["xyz"]), sc["xyz"].shape[0], 0, ptr(sc["cams"]), ptr(sc["intr"]), 4, 0, N, *GEOM, VOXEL, max_radius,
                 ptr(zbuf), ptr(stats), stream_ptr(zbuf)), "vipe_cloud_render (always-atomic form)")
    return call


def shipped_render(sc, zbuf, stats, max_radius):
    from vipe_amd.slam.ingest import cloud_render
    cloud_render(sc["xyz"], sc["cams"], sc["intr"], "pinhole", GEOM, zbuf, VOXEL, max_radius=max_radius, stats=stats)


def torch_composition(sc, max_radius):
    """the same z-buffer as torch operators (pinhole, pure translations) -> (zbuf int64 [N,H0,W0], footprint pixels written)"""
    h1, w1, top, left, H0, W0 = PARAMS
    xyz, dev = sc["xyz"], sc["xyz"].device
    fx, fy, cx, cy = sc["intr"][0]
    sx, sy = w1 / W0, h1 / H0
    Xc = xyz[None] + sc["cams"][:, None, :3]
    z = Xc[..., 2]
    ok = z > 0.1
    zs = torch.where(ok, z, torch.ones_like(z))
    px = torch.floor((fx * (Xc[..., 0] / zs) + cx + left + 0.5) / sx)
    py = torch.floor((fy * (Xc[..., 1] / zs) + cy + top + 0.5) / sy)
    r = torch.clamp((0.5 * VOXEL * (fx / sx) / zs).long(), max=max_radius)
    ok &= (px >= -max_radius - 1) & (px <= W0 + max_radius) & (py >= -max_radius - 1) & (py <= H0 + max_radius)
    px, py = px.long(), py.long()
    key = (zs.view(torch.int32).long() << 32) | torch.arange(xyz.shape[0], device=dev)[None]
    base = torch.arange(N, device=dev)[:, None] * (H0 * W0)
    out = torch.full((N * H0 * W0,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
    written = 0
    for dy in range(-max_radius, max_radius + 1):
        for dx in range(-max_radius, max_radius + 1):
            x, y = px + dx, py + dy
            m = ok & (r >= max(abs(dx), abs(dy))) & (x >= 0) & (x < W0) & (y >= 0) & (y < H0)
            out.scatter_reduce_(0, (base + y * W0 + x)[m], key[m], reduce="amin")
            written += int(m.sum())
    out = torch.where(out == torch.iinfo(torch.int64).max, torch.full_like(out, -1), out)
    return out.view(N, H0, W0), written


def kernel_figures(args, dev):
    from vipe_amd.slam.ingest import cloud_resolve, cloud_zbuffer
    sc = make_scene(dev)
    H0, W0 = PARAMS[4:]
    forms = {"preload": shipped_render}
    if os.path.exists(ALWAYS_LIB):
        forms["always_atomic"] = always_render()
    zbufs = [cloud_zbuffer(N, H0, W0, dev) for _ in range(args.sets)]
    out = {"shape": {"points": int(sc["xyz"].shape[0]), "images": N, "H": H, "W": W, "params_h1_w1_top_left_H0_W0": list(PARAMS),
                     "camera": "pinhole", "point_size": VOXEL},
           "iters": args.iters, "buffer_sets": args.sets, "variants": {}}
    fill_ms = dct.event_ms(lambda i: zbufs[i % args.sets].fill_(-1), args.iters)
    out["zbuffer_fill_ms"] = round(fill_ms, 5)
    for max_radius in (0, 2):
        row, result = {}, {}
        for form, fn in forms.items():
            stats = torch.zeros(3, dtype=torch.int64, device=dev)
            z = cloud_zbuffer(N, H0, W0, dev)
            fn(sc, z, stats, max_radius)
            torch.cuda.synchronize()
            result[form] = (z, stats.tolist())
            scratch_stats = torch.zeros(3, dtype=torch.int64, device=dev)

            def call(i, fn=fn):
                zb = zbufs[i % args.sets]
                zb.fill_(-1)
                fn(sc, zb, scratch_stats, max_radius)
            total = dct.event_ms(call, args.iters)
            row[f"{form}_fill_plus_render_ms"] = round(total, 5)
            row[f"{form}_render_ms"] = round(total - fill_ms, 5)
            row[f"{form}_render_into_a_filled_buffer_ms"] = round(
                dct.event_ms(lambda i, fn=fn: fn(sc, zbufs[i % args.sets], scratch_stats, max_radius), args.iters), 5)
        z, stats = result["preload"]
        row.update(counters_one_call=stats, pixels_drawn=int((z != -1).sum()))
        t_torch = dct.event_ms(lambda i: torch_composition(sc, max_radius), max(3, args.iters // 40), warm=1)
        tz, written = torch_composition(sc, max_radius)
        row["atomics"] = written
        row["torch_composition_ms"] = round(t_torch, 4)
        row["torch_over_hip"] = round(t_torch / row["preload_render_ms"], 2)
        row["torch_pixels_that_differ"] = int((tz != z).sum())  # float32 torch arithmetic rounds a few points over a pixel border
        row["Mpairs_per_s"] = round(sc["xyz"].shape[0] * N / row["preload_render_ms"] / 1e3, 1)
        if "always_atomic" in result:
            za, sa = result["always_atomic"]
            row["forms_leave_the_same_buffer"] = bool(torch.equal(z, za) and stats == sa)
            row["always_atomic_GBps"] = round(written * 8 / row["always_atomic_render_ms"] / 1e6, 1)
            row["always_atomic_over_preload"] = round(row["always_atomic_render_ms"] / row["preload_render_ms"], 2)
        out["variants"][f"max_radius{max_radius}"] = row
        print(json.dumps({f"max_radius{max_radius}": row}), flush=True)
    z = result["preload"][0]
    for dtype, colour in ((torch.float16, False), (torch.float16, True), (torch.float32, True)):
        name = f"resolve_{'f16' if dtype == torch.float16 else 'f32'}{'_colour' if colour else ''}_ms"
        out[name] = round(dct.event_ms(lambda i: cloud_resolve(z, sc["rgb"] if colour else None, dtype=dtype), args.iters), 5)
    return out


def clip_figures(args, dev):
    import bench
    from vipe_amd.slam import ingest, system
    from vipe_amd.slam.factor_graph import warm_volume_pool
    real = system.SLAMConfig
    base = dict(frame_depth=True, frame_depth_conf=True, fused_cloud=True)
    flags = {"cloud": base, "depth": dict(base, fused_depth=True)}
    names = args.variants.split(",")
    runs = {}
    for name in names:
        system.SLAMConfig = functools.partial(real, **flags[name])
        try:
            runs[name] = bench.make_clip_runner(dev)
        finally:
            system.SLAMConfig = real
    seen = {"render": 0, "points": None}
    real_render = getattr(ingest, "cloud_render", None)
    if real_render is not None:
        def counted(xyz, *a, **k):
            seen["render"] += 1
            seen["points"] = int(xyz.shape[0])
            return real_render(xyz, *a, **k)
        ingest.cloud_render = counted

    def one(name, seed, n):
        seen["render"], seen["points"] = 0, None
        r = runs[name](seed=seed, n_frames=n, keep_every=4)
        r["render_launches"], r["cloud_points"] = seen["render"], seen["points"]
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
                              "keyframes": r["keyframes"], "frames": r["frames"], "state_finite": r["finite"],
                              "render_launches": r["render_launches"], "cloud_points": r["cloud_points"]})
    return {"runs": res, "frames_per_s_best": {k: max(x["frames_per_s"] for x in v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-clip", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--build-always", action="store_true")
    ap.add_argument("--variants", default="cloud,depth")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.build_always:
        return build_always()
    dev = torch.device("cuda:0")
    line = {}
    if not args.no_kernel:
        line["kernel"] = kernel_figures(args, dev)
        print(json.dumps({"kernel": {k: v for k, v in line["kernel"].items() if k != "variants"}}), flush=True)
    if not args.no_clip:
        line["clip"] = clip_figures(args, dev)
        print(json.dumps({"clip": line["clip"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_cloud_render: the cloud of one vipe_cloud_fuse call of scratch/cloud_fuse_time.py (voxel 0.02) drawn "
                       "into 16 pinhole cameras at 1080 x 1920 (export geometry 384 x 512 -> 1080 x 1920), one MI355X: the "
                       "library's form (a plain load in front of the atomic) and the always-atomic form, next to a torch "
                       "composition; vipe_cloud_resolve; and the keep-every-4 clip of bench.py (make_clip_runner, 384 x 512) "
                       "with frame_depth, frame_depth_conf and fused_cloud on, fused_depth off ('cloud') / on ('depth')",
               "event_timing": line.get("kernel"),
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls; a call is fill_(-1) of "
                                    f"one of {args.sets} rotating z-buffers plus the render, render_ms is that less the fill "
                                    "timed alone; the torch composition is timed over a fortieth of the calls",
               "clip": line.get("clip"),
               "clip_note": "frames / wall time of SLAMSystem.run, 2 runs per variant alternating after a warm-up clip per "
                            "variant and one full-length clip; maps at SLAM resolution kept on the device; the clip's frames "
                            "are random images, so few pixels pass the gate and the cloud is small",
               "commands": ["python scratch/cloud_render_time.py --build-always",
                            f"python scratch/cloud_render_time.py --iters {args.iters} --sets {args.sets} --frames {args.frames} "
                            "--out profiles/cloud_render_time.json"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
