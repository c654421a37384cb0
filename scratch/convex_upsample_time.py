"""`vipe_convex_upsample` at N = 48 keyframes on the 48 x 64 grid, C = 1 (fp16 mask as the operator writes it),
event-timed on the current stream next to DROID-SLAM's torch composition (softmax + F.unfold + sum) on the same inputs.

    python scratch/convex_upsample_time.py [--iters N] [--out FILE]

"bytes" is what the algorithm has to move: the mask once (1152 B per coarse pixel), the data once, the output once
(256 * C B per coarse pixel), against 8 TB/s of HBM.  The 170 MB mask + 38 MB output of this shape fit the 256 MiB
Infinity Cache, so back-to-back calls on ONE buffer are not an HBM figure: the timed loop rotates over enough
buffer sets that a set is evicted before it is used again (--sets, default 4: 0.8 GB in rotation).  The largest
error / bound ratio against the float64 reference (tests/cvx_reference.py) is reported for a 4-keyframe slice."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import cvx_reference as cr  # noqa: E402
from vipe_amd.ext import droid_net_ext  # noqa: E402

HBM_BPS = 8e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    N, h, w, C = 48, 48, 64, 1
    gen = torch.Generator(device=dev).manual_seed(0)
    sets = []
    for _ in range(args.sets):
        mask = (torch.randn(N, h, w, 576, generator=gen, device=dev) * 3.0).half()
        data = torch.rand(N, h, w, C, generator=gen, device=dev) + 0.5
        out = torch.empty(N, 8 * h, 8 * w, C, device=dev)
        sets.append((data, mask, out))
    t_hip = event_ms(lambda i: droid_net_ext.cvx_upsample(*sets[i % args.sets][:2], out=sets[i % args.sets][2]), args.iters)
    t_hip_hot = event_ms(lambda i: droid_net_ext.cvx_upsample(*sets[0][:2], out=sets[0][2]), args.iters)
    t_torch = event_ms(lambda i: cr.torch_composition(sets[i % args.sets][0], sets[i % args.sets][1].float()),
                       max(10, args.iters // 10))
    t_torch_f16 = event_ms(lambda i: cr.torch_composition(sets[i % args.sets][0].half(), sets[i % args.sets][1]),
                           max(10, args.iters // 10))
    data, mask, out = sets[0]
    droid_net_ext.cvx_upsample(data, mask, out=out)
    torch.cuda.synchronize()
    dn, mn = data[:4].cpu().numpy(), mask[:4].cpu().numpy()
    ref, bound = cr.cvx_upsample_ref(dn, mn), cr.cvx_bound(dn)
    ratio = float((np.abs(out[:4].cpu().numpy().astype(np.float64) - ref) / bound).max())
    vs_torch = (out - cr.torch_composition(data, mask.float())).abs().max().item()
    nbytes = N * h * w * (576 * 2 + 4 * C + 64 * C * 4)
    line = {"shape": {"N": N, "h": h, "w": w, "C": C, "mask": "float16"}, "iters": args.iters, "buffer_sets": args.sets,
            "hip_ms": round(t_hip, 5), "hip_ms_one_buffer_set": round(t_hip_hot, 5), "bytes": nbytes,
            "hip_GBps": round(nbytes / t_hip / 1e6, 1), "share_of_8TBps": round(nbytes / (t_hip * 1e-3) / HBM_BPS, 4),
            "share_of_8TBps_one_buffer_set": round(nbytes / (t_hip_hot * 1e-3) / HBM_BPS, 4),
            "torch_composition_f32_ms": round(t_torch, 5), "torch_over_hip": round(t_torch / t_hip, 2),
            "torch_composition_f16_ms": round(t_torch_f16, 5), "torch_f16_over_hip": round(t_torch_f16 / t_hip, 2),
            "max_err_over_bound": round(ratio, 4), "c_bound": cr.C_BOUND, "max_abs_diff_vs_torch_f32": vs_torch}
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_convex_upsample at N = 48 keyframes, 48 x 64 grid, C = 1, fp16 mask, one MI355X; next to DROID-SLAM's "
                       "torch composition (softmax over the 9 taps, F.unfold, sum, permute) on the same inputs",
               "event_timing": line,
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls, rotating over "
                                    f"{args.sets} buffer sets (208 MB each: a set leaves the 256 MiB Infinity Cache before it "
                                    "is used again); *_one_buffer_set: the same calls on one set, which the Infinity Cache "
                                    "holds - not an HBM figure.  bytes = mask + data + out, each once; shares are of the "
                                    "8 TB/s HBM peak (about 6.3 TB/s is achievable)",
               "commands": [f"python scratch/convex_upsample_time.py --iters {args.iters} --out convex_upsample_time.json"]}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
