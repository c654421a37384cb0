"""The sparse tracker (klt_track.hip) at 384 x 512 and 1080 x 1920 with every cell occupied: the three entry points
event-timed on the current stream, a whole `KLTSparseTracks.track_image` (wall clock: it ends with the host waiting for
the tracker's event and building the dictionaries), and pass 1 of one `SLAMSystem.run` on a synthetic clip with
`SLAMConfig.sparse_tracks` None and "klt".

    python scratch/klt_time.py [--iters N] [--clip-frames T] [--out FILE]

Frames are the analytic texture of tests/klt_reference.py (rendered on the device), frame k seen through k steps of its
warp, so the tracker has real work: every cell holds a corner and nearly every point survives."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import klt_reference as K  # noqa: E402
from vipe_amd.ext import klt_ext  # noqa: E402
from vipe_amd.slam.sparse_tracks import KLTSparseTracks  # noqa: E402


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


def render(tex, H, W, warp, dev):
    """tests/klt_reference.render on the device -> rgb [H,W,3] float32 in 0-1"""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev),
                            indexing="ij")
    p = torch.stack([xx, yy], -1).reshape(-1, 2)
    Minv = torch.from_numpy(np.linalg.inv(warp.M)).to(dev)
    p = (p - torch.from_numpy(warp.c + warp.t).to(dev)) @ Minv.T + torch.from_numpy(warp.c).to(dev)
    s = torch.zeros(H * W, dtype=torch.float64, device=dev)
    for fx, fy, ph, a in zip(tex.fx, tex.fy, tex.ph, tex.amp):
        s += a * torch.cos(2 * np.pi * (fx * p[:, 0] + fy * p[:, 1]) + ph)
    g = torch.clamp(127.5 + 127.5 * s / (3 * tex.sigma), 0.0, 255.0).reshape(H, W)
    return (g / 255.0).float()[..., None].repeat(1, 1, 3).contiguous()


def entry_points(H, W, iters, dev):
    from vipe_amd.slam.system import Frame
    tex = K.Texture(0)
    frames = [render(tex, H, W, K.Warp(H, W, steps=k), dev) for k in range(4)]
    u8 = [(f * 255).round().to(torch.uint8) for f in frames]
    tr = KLTSparseTracks(1, device=dev)
    L, prm, cell = tr._levels_for(H, W), tr.params, tr.cell
    n_cells = -(-H // cell) * -(-W // cell)
    pyr = [klt_ext.pyramid(f, L) for f in frames]
    cells = klt_ext.detect(pyr[0][:H * W].view(H, W), cell, prm["border"], prm["min_eig"])
    pts = cells[cells[:, 0] >= 0, :2].contiguous()
    fwd, status, _ = klt_ext.track(pyr[0], pyr[1], H, W, L, pts, **prm)
    busy = torch.zeros(n_cells, dtype=torch.uint8, device=dev)
    out = {"H": H, "W": W, "levels": L, "cell": cell, "cells": n_cells, "points": int(pts.shape[0]),
           "launches_per_track_image": L + 4, "iters": iters}
    out["pyramid_f32_ms"] = round(event_ms(lambda i: klt_ext.pyramid(frames[i % 4], L, out=pyr[i % 4]), iters), 5)
    out["pyramid_u8_ms"] = round(event_ms(lambda i: klt_ext.pyramid(u8[i % 4], L, out=pyr[i % 4]), iters), 5)
    pyr = [klt_ext.pyramid(f, L) for f in frames]
    out["detect_all_cells_free_ms"] = round(event_ms(lambda i: klt_ext.detect(pyr[i % 4][:H * W].view(H, W), cell, prm["border"], prm["min_eig"], out=cells), iters), 5)
    out["track_forward_ms"] = round(event_ms(lambda i: klt_ext.track(pyr[0], pyr[1], H, W, L, pts, **prm), iters), 5)
    out["track_backward_ms"] = round(event_ms(lambda i: klt_ext.track(pyr[1], pyr[0], H, W, L, fwd, fb_ref=pts, status=status, cell=cell, cell_busy=busy, **prm), iters), 5)
    # a whole track_image, frames cycling forwards and backwards through the warp so that points survive
    order = [0, 1, 2, 3, 2, 1]
    fr = [[Frame(rgb=f)] for f in frames]
    for i in range(6):
        tr.track_image(fr[order[i % 6]])
    tr.observations[0].clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(iters):
        tr.track_image(fr[order[i % 6]])
    torch.cuda.synchronize()
    out["track_image_wall_ms"] = round((time.perf_counter() - t0) / iters * 1e3, 4)
    out["track_image_live_points"] = int(np.mean([len(o) for o in tr.observations[0]]))
    return out


def pass1(H, W, T, dev):
    """pass-1 seconds per frame of one SLAMSystem.run on the warped-texture clip, tracker off and on (second of two runs
    each: the first one pays for lazy initialisation)"""
    from vipe_amd.slam.frontend import FrontendArgs
    from vipe_amd.slam.system import Frame, SLAMConfig, SLAMSystem
    tex = K.Texture(0)
    intr = torch.tensor([0.9 * W, 0.9 * W, W / 2.0, H / 2.0])
    frames = [Frame(rgb=render(tex, H, W, K.Warp(H, W, steps=k), dev), intrinsics=intr) for k in range(T)]
    res = {"H": H, "W": W, "frames": T}
    for name in (None, "klt"):
        for rep in range(2):
            torch.manual_seed(0)
            # every frame a keyframe: the tracker's score must not change WHICH frames pass 1 works on, or the two runs
            # measure different work
            sysm = SLAMSystem(dev, SLAMConfig(buffer=max(64, T + 8), filter_thresh=0.0, frontend_backend_iters=(),
                                              frontend=FrontendArgs(keyframe_thresh=0.0), sparse_tracks=name))
            spent, term, parts = [0.0], [0.0], {"launch": 0.0, "collect": 0.0}
            if name:
                inner, inner_w = KLTSparseTracks.track_image, KLTSparseTracks.compute_dense_disp_target_weight

                def timed_w(self, *a, _inner=inner_w, **k):
                    t0 = time.perf_counter()
                    r = _inner(self, *a, **k)
                    term[0] += time.perf_counter() - t0
                    return r
                KLTSparseTracks.compute_dense_disp_target_weight = timed_w

                inner_l, inner_c = KLTSparseTracks._launch, KLTSparseTracks._collect

                def timed_l(self, *a, _inner=inner_l):
                    t0 = time.perf_counter()
                    r = _inner(self, *a)
                    parts["launch"] += time.perf_counter() - t0
                    return r

                def timed_c(self, *a, _inner=inner_c):
                    t0 = time.perf_counter()
                    _inner(self, *a)
                    parts["collect"] += time.perf_counter() - t0
                KLTSparseTracks._launch, KLTSparseTracks._collect = timed_l, timed_c

                def timed(self, frames, _inner=inner):
                    t0 = time.perf_counter()
                    _inner(self, frames)
                    spent[0] += time.perf_counter() - t0
                KLTSparseTracks.track_image = timed
            try:
                sysm.run(frames)
            finally:
                if name:
                    KLTSparseTracks.track_image, KLTSparseTracks.compute_dense_disp_target_weight = inner, inner_w
                    KLTSparseTracks._launch, KLTSparseTracks._collect = inner_l, inner_c
            torch.cuda.synchronize()
        key = "klt" if name else "off"
        res[f"pass1_ms_per_frame_{key}"] = round(sysm.timings["pass1_seconds"] / T * 1e3, 3)
        res[f"keyframes_{key}"] = int(sysm.n_keyframes)
        if name:
            res["track_image_ms_per_frame_in_run"] = round(spent[0] / T * 1e3, 3)
            res["track_image_parts_ms_per_frame"] = {
                "host_launches": round(parts["launch"] / T * 1e3, 3), "host_dictionaries": round(parts["collect"] / T * 1e3, 3),
                "event_wait": round((spent[0] - parts["launch"] - parts["collect"]) / T * 1e3, 3)}
            res["tracker_share_of_pass1_frame"] = round(spent[0] / sysm.timings["pass1_seconds"], 4)
            res["tracker_over_baseline_pass1_frame"] = round(spent[0] / T * 1e3 / res["pass1_ms_per_frame_off"], 4)
            res["track_term_host_ms_per_frame_pass1_and_backend"] = round(term[0] / T * 1e3, 3)
            res["live_points_last_frame"] = len(sysm.sparse_tracks.observations[0][-1])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--clip-frames", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"what": "sparse tracker (klt_track.hip) on one MI355X: entry points and KLTSparseTracks.track_image at 384 x 512 "
                   "and 1080 x 1920 with every cell occupied; pass 1 of SLAMSystem.run with the tracker off and on",
           "entry_points": [entry_points(384, 512, args.iters, dev), entry_points(1080, 1920, args.iters, dev)],
           "pass1": pass1(384, 512, args.clip_frames, dev),
           "note": f"*_ms: events around {args.iters} back-to-back calls after 3 warm-up calls (pyramids rotate over 4 frames); "
                   "track_image_wall_ms: wall clock per call, host wait and dictionaries included; pass 1: "
                   "SLAMSystem.timings['pass1_seconds'] / frames, every frame a keyframe in both runs; tracker share = time inside track_image / pass-1 time; track_term_host_ms: host time inside compute_dense_disp_target_weight (the per-edge dictionary walk, not part of this change) over the whole run, per frame",
           "commands": [f"python scratch/klt_time.py --iters {args.iters} --clip-frames {args.clip_frames} --out klt_time.json"]}
    print(json.dumps(doc), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
