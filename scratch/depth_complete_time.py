"""`vipe_depth_anchor_bits` + `vipe_depth_complete` event-timed on the current stream, next to what they replace, and the
cost of `SLAMConfig.complete_depth` on the keep-every-4 clip of bench.py.

    python scratch/depth_complete_time.py [--iters N] [--frames N] [--no-clip] [--no-kernel] [--composition]
                                          [--variants depth,complete] [--out FILE]

(a) Kernel.  The 16 maps of 1080 x 1920 of one render call of scratch/cloud_render_time.py (its cloud drawn into its 16
cameras at max_radius 2, resolved to f16) as anchors, the same chunk's `depth_export` maps (f16) as predictions, K = 5,
R = 32, depth domain; events around --iters calls after 3 warm-up calls, the bits pass and the main pass timed separately
(through the library handle, as `ingest.depth_complete` calls them) and together (the wrapper).  The anchor density and
the unreached share are recorded.

(b) Against what it replaces, on the device: `nonzero` + `utils_ext.nearest_neighbours` + batched `torch.linalg.lstsq`
on the reference's construction (rows scaled by w / sum w, w = 1 / dist), for ONE 384 x 512 image of the same data (the
top-left 384 x 512 window of the first map: the brute-force search cannot do 1080p).  Only with --composition: on the
first device run this part (1 warm-up and 5 timed calls, about 20 000 least-squares problems of 5 x 2 each) did not
finish within the job's 400 s limit and was ended there, so no ratio is recorded.

(c) Clip: `bench.make_clip_runner`'s clip with keep_every=4 (2 * --frames frames), `frame_depth`, `frame_depth_conf`,
`fused_cloud` and `fused_depth` on, without ("depth") and with ("complete") `complete_depth`, alternating, two runs each
after one warm-up clip per variant.  `--variants depth --no-kernel` runs on a tree that does not have the flag."""
import argparse
import functools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scratch"))
import torch  # noqa: E402

import cloud_fuse_time as cft  # noqa: E402  (scratch/: the scene)
import cloud_render_time as crt  # noqa: E402  (scratch/: its cloud, the render)
import depth_consistency_time as dct  # noqa: E402  (scratch/: the event timer)

PARAMS, N = dct.PARAMS, dct.N
K, R = 5, 32


def make_maps(dev):
    """-> (fused [16,1080,1920] f16, frame [16,1080,1920] f16): one render call of cloud_render_time and its chunk's export"""
    from vipe_amd.slam.ingest import cloud_resolve, cloud_zbuffer, depth_export
    sc = crt.make_scene(dev)
    zbuf = cloud_zbuffer(N, PARAMS[4], PARAMS[5], dev)
    crt.shipped_render(sc, zbuf, torch.zeros(3, dtype=torch.int64, device=dev), 2)
    fused = cloud_resolve(zbuf, None, dtype=torch.float16)[0]
    s = cft.make_set(dev, 0)
    frame = depth_export(s["disp"], PARAMS, rows=s["rows"], dtype=torch.float16)
    return fused, frame


def kernel_figures(args, dev):
    from vipe_amd._lib import F16, check, lib, ptr, stream_ptr
    from vipe_amd.slam import ingest
    fused, frame = make_maps(dev)
    B, H, W = fused.shape
    out, _, _, _, stats = ingest.depth_complete(fused, frame, K=K, radius=R)
    torch.cuda.synchronize()
    st = stats.tolist()
    anchors = int(((fused > 0) & (frame > 0)).sum())
    targets = sum(st)
    bits = ingest._anchor_bits(B * H * ((W + 63) // 64), dev)
    scratch = torch.zeros(4, dtype=torch.int64, device=dev)

    def bits_pass(i):
        check(lib().vipe_depth_anchor_bits(ptr(fused), ptr(frame), F16, B, H, W, ptr(bits), stream_ptr(fused)), "bits")

    def main_pass(i):
        check(lib().vipe_depth_complete(ptr(fused), ptr(frame), F16, None, ptr(bits), B, H, W, 1, K, R, 0, ptr(out), None, None,
                                        None, ptr(scratch), stream_ptr(fused)), "complete")

    res = {"shape": {"images": B, "H": H, "W": W, "dtype": "f16", "K": K, "radius": R, "domain": "depth"},
           "iters": args.iters, "anchors": anchors, "anchor_density": round(anchors / (B * H * W), 4), "targets": targets,
           "counters_affine_scale_unreached_rejected": st, "unreached_share_of_targets": round(st[2] / max(targets, 1), 4),
           "bits_ms": round(dct.event_ms(bits_pass, args.iters), 5), "complete_ms": round(dct.event_ms(main_pass, args.iters), 5),
           "wrapper_both_ms": round(dct.event_ms(lambda i: ingest.depth_complete(fused, frame, K=K, radius=R, out=out, stats=scratch),
                                                 args.iters), 5)}
    res["bytes_read_written_once"] = B * H * W * 2 * 3
    res["complete_GBps_of_that"] = round(res["bytes_read_written_once"] / res["complete_ms"] / 1e6, 1)
    print(json.dumps({"kernel": res}), flush=True)
    if not args.composition:
        return res
    # (b) one 384 x 512 image: the composition the reference runs, on the device
    from vipe_amd.ext import utils_ext
    sp, pr = fused[0, :384, :512].float().contiguous(), frame[0, :384, :512].float().contiguous()
    sp_d, pr_d = torch.where(sp > 0, 1.0 / sp, sp), 1.0 / pr  # disparities, as `kss_completer` takes them

    def composition(i=0):
        smask = sp_d > 0
        tree = torch.nonzero(smask)[:, [1, 0]].float().contiguous()
        query = torch.nonzero(~smask)[:, [1, 0]].float().contiguous()
        _, idx = utils_ext.nearest_neighbours(query, tree, K)
        idx = idx.long()
        ks, kp = sp_d[smask][idx], pr_d[smask][idx]
        dist = (query[:, None] - tree[idx]).norm(dim=2)
        w = 1.0 / dist
        w = w / w.sum(1, keepdim=True)
        X = torch.stack([kp, torch.ones_like(kp)], 2) * w[..., None]
        sol = torch.linalg.lstsq(X, (ks * w)[..., None]).solution[..., 0]
        res_ = torch.zeros_like(sp_d)
        res_[~smask] = pr_d[~smask] * sol[:, 0] + sol[:, 1]
        res_[smask] = sp_d[smask]
        return res_

    small_out = torch.empty_like(sp)
    ours = dct.event_ms(lambda i: ingest.depth_complete(sp[None], pr[None], K=K, radius=R, out=small_out[None], stats=scratch),
                        args.iters)
    a = int((sp > 0).sum())
    row = {"anchors": a, "queries": 384 * 512 - a, "hip_bits_plus_complete_ms": round(ours, 5)}
    try:
        theirs = dct.event_ms(composition, max(3, args.iters // 20), warm=1)
        row.update(nonzero_knn_lstsq_ms=round(theirs, 4), composition_over_hip=round(theirs / ours, 1))
    except Exception as e:  # noqa: BLE001 - a batched lstsq the device build of torch cannot do is a finding, not a failure
        row["composition_failed"] = f"{type(e).__name__}: {e}"[:300]
    res["against_composition_384x512"] = row
    print(json.dumps({"against_composition_384x512": res["against_composition_384x512"]}), flush=True)
    return res


def clip_figures(args, dev):
    import bench
    from vipe_amd.slam import ingest, system
    from vipe_amd.slam.factor_graph import warm_volume_pool
    real = system.SLAMConfig
    base = dict(frame_depth=True, frame_depth_conf=True, fused_cloud=True, fused_depth=True)
    flags = {"depth": base, "complete": dict(base, complete_depth=True)}
    names = args.variants.split(",")
    runs = {}
    for name in names:
        system.SLAMConfig = functools.partial(real, **flags[name])
        try:
            runs[name] = bench.make_clip_runner(dev)
        finally:
            system.SLAMConfig = real
    seen = {"complete": 0}
    real_complete = getattr(ingest, "depth_complete", None)
    if real_complete is not None:
        def counted(*a, **k):
            seen["complete"] += 1
            return real_complete(*a, **k)
        ingest.depth_complete = counted

    def one(name, seed, n):
        seen["complete"] = 0
        r = runs[name](seed=seed, n_frames=n, keep_every=4)
        r["complete_calls"] = seen["complete"]
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
                              "complete_calls": r["complete_calls"]})
    return {"runs": res, "frames_per_s_best": {k: max(x["frames_per_s"] for x in v) for k, v in res.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--no-clip", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    ap.add_argument("--composition", action="store_true", help="(b): did not finish within 400 s on the first device run")
    ap.add_argument("--variants", default="depth,complete")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    line = {}
    if not args.no_kernel:
        line["kernel"] = kernel_figures(args, dev)
    if not args.no_clip:
        line["clip"] = clip_figures(args, dev)
        print(json.dumps({"clip": line["clip"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_depth_anchor_bits + vipe_depth_complete, one MI355X: 16 maps of 1080 x 1920 (f16) of one render call "
                       "of scratch/cloud_render_time.py as anchors, the chunk's depth_export maps as predictions, K = 5, R = 32; "
                       "one 384 x 512 window of them against nonzero + utils_ext.nearest_neighbours + torch.linalg.lstsq on the "
                       "device; and the keep-every-4 clip of bench.py (make_clip_runner, 384 x 512) with frame_depth, "
                       "frame_depth_conf, fused_cloud and fused_depth on, complete_depth off ('depth') / on ('complete')",
               "event_timing": line.get("kernel"),
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls; the composition is timed "
                                    "over a twentieth of the calls after 1 warm-up call",
               "clip": line.get("clip"),
               "clip_note": "frames / wall time of SLAMSystem.run, 2 runs per variant alternating after a warm-up clip per "
                            "variant and one full-length clip; maps at SLAM resolution kept on the device",
               "commands": [f"python scratch/depth_complete_time.py --iters {args.iters} --frames {args.frames} "
                            "--out profiles/depth_complete_time.json"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
