"""`vipe_frame_ingest` at native 1080 x 1920 and 720 x 1280 (fp32 and uint8 frames, with and without mask + depth),
event-timed on the current stream next to what a caller has to run today on the same GPU to hand `SLAMSystem.run` a frame
at SLAM resolution: F.interpolate x 3 (rgb, mask, depth), the crops, the permute, the 1/8 mask resample, the [3::8, 3::8]
slice + where, then `vipe_enc_prep`.

    python scratch/ingest_time.py [--iters N] [--out FILE] [--unfused-src]     one JSON line per (size, dtype, inputs)

--out writes {"what", "event_timing": [those lines], "event_timing_note", "unfused_src"}: the shape of
profiles/ingest_time.json, whose "kernel_trace" part is added by hand from the statistics `rocprofv3 --kernel-trace
--stats` prints for this script.  --unfused-src also resamples the 1080p frame in torch with the kernel's arithmetic but
`src` as a separately rounded product and difference, and reports how far that is from F.interpolate: the reason for
the one fused multiply-add in make_tap (frame_ingest.hip).

"bytes" counts what the kernel has to move: the source rows and columns its taps touch (every source pixel once when
downscaling by less than 2, else two rows / columns per output row / column) plus the outputs, against 8 TB/s of HBM."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vipe_amd.slam.encoders import normalize_images  # noqa: E402
from vipe_amd.slam.ingest import StandardResize, frame_ingest  # noqa: E402

HBM_BPS = 8e12


def event_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def compose(rgb, mask, depth, r):
    """The caller's side today: the reference's VideoFrame.resize / crop, _precompute_features, _add_keyframe lines."""
    (h1, w1), (top, _, left, _), (H, W) = r.size, r.crop, r.out_size
    x = rgb.float() / 255.0 if rgb.dtype == torch.uint8 else rgb
    images = F.interpolate(x.permute(2, 0, 1)[None], (h1, w1), mode="bilinear")[:, :, top:top + H, left:left + W].contiguous()
    x4 = normalize_images(images)
    m8 = ds = None
    if mask is not None:
        m = F.interpolate(mask[None, None].float(), (h1, w1), mode="bilinear")[0, 0] > 0.9
        m = m[top:top + H, left:left + W]
        m8 = ~(F.interpolate(m[None, None].float(), (H // 8, W // 8), mode="bilinear")[0, 0] > 0.9)
    if depth is not None:
        d = F.interpolate(depth[None, None], (h1, w1), mode="bilinear")[0, 0][top:top + H, left:left + W][3::8, 3::8]
        ds = torch.where(d > 0, d.reciprocal(), d)
    return images, x4, m8, ds


def unfused_resample(x, h1, w1):
    """x [C,H0,W0] f32 -> [C,h1,w1]: frame_ingest.hip's taps and blend as torch tensor operations (each rounded on its
    own), with src = scale * (dst + 0.5) - 0.5 as two operations instead of the kernel's one."""
    def taps(n_in, n_out):
        scale = torch.tensor(n_in, dtype=torch.float32, device=x.device) / torch.tensor(n_out, dtype=torch.float32, device=x.device)
        src = ((torch.arange(n_out, device=x.device, dtype=torch.float32) + 0.5) * scale - 0.5).clamp_min(0.0)
        i0 = src.to(torch.int64).clamp_max(n_in - 1)
        l1 = src - i0.float()
        return i0, (i0 + 1).clamp_max(n_in - 1), 1.0 - l1, l1
    y0, y1, h0, h1w = taps(x.shape[1], h1)
    x0, x1, w0, w1w = taps(x.shape[2], w1)
    r0, r1 = x[:, y0], x[:, y1]
    top = w0 * r0[:, :, x0] + w1w * r0[:, :, x1]
    bot = w0 * r1[:, :, x0] + w1w * r1[:, :, x1]
    return h0[:, None] * top + h1w[:, None] * bot


def kernel_bytes(r, rgb_elem, with_aux):
    (H0, W0), (h1, w1), (H, W) = r.native_size, r.size, r.out_size
    rows = min(H0, 2 * H) if H0 > h1 else H0
    cols = min(W0, 2 * W) if W0 > w1 else W0
    n = rows * cols * 3 * rgb_elem + H * W * (3 * 4 + 4 * 2)
    if with_aux:  # four mask pixels (four taps each) and one depth pixel (four taps) per 1/8 cell, one byte + one float out
        n += (H // 8) * (W // 8) * (16 * 1 + 4 * 4 + 1 + 4)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--unfused-src", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    lines, unfused = [], None
    for H0, W0 in ((1080, 1920), (720, 1280)):
        r = StandardResize(H0, W0)
        H, W = r.out_size
        rgb32 = torch.rand(H0, W0, 3, generator=gen, device=dev)
        depth = 0.5 + 9.5 * torch.rand(H0, W0, generator=gen, device=dev)
        mask = torch.rand(H0 // 40, W0 // 40, generator=gen, device=dev).repeat_interleave(40, 0).repeat_interleave(40, 1) > 0.1
        images = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        x4 = torch.empty((H, W, 4), dtype=torch.float16, device=dev)
        m8 = torch.empty((H // 8, W // 8), dtype=torch.bool, device=dev)
        ds = torch.empty((H // 8, W // 8), dtype=torch.float32, device=dev)
        if args.unfused_src and unfused is None:
            want = F.interpolate(rgb32.permute(2, 0, 1)[None], r.size, mode="bilinear")[0]
            d = (unfused_resample(rgb32.permute(2, 0, 1), *r.size) - want).abs()
            c, y, x = (int(v) for v in torch.unravel_index(d.argmax(), d.shape))
            unfused = {"native": [H0, W0], "resized": list(r.size), "max_abs_diff_vs_F_interpolate": d.max().item(),
                       "at_channel_row_column": [c, y, x]}
            print(json.dumps({"unfused_src": unfused}), flush=True)
        for rgb in (rgb32, (rgb32 * 255).round().to(torch.uint8)):
            for aux in (True, False):
                mk, dp = (mask, depth) if aux else (None, None)
                t_hip = event_ms(lambda: frame_ingest(rgb, r, images, x4, mk, m8 if aux else None, dp, ds if aux else None), args.iters)
                t_torch = event_ms(lambda: compose(rgb, mk, dp, r), args.iters)
                ref = compose(rgb, mk, dp, r)
                err = (images - ref[0][0]).abs().max().item()
                nbytes = kernel_bytes(r, rgb.element_size(), aux)
                lines.append({"native": [H0, W0], "out": [H, W], "rgb": str(rgb.dtype).replace("torch.", ""),
                              "mask_and_depth": aux, "hip_ms": round(t_hip, 4), "torch_composition_ms": round(t_torch, 4),
                              "speedup": round(t_torch / t_hip, 2), "bytes": nbytes, "hip_GBps": round(nbytes / t_hip / 1e6, 1),
                              "share_of_8TBps": round(nbytes / t_hip / 1e-3 / HBM_BPS, 4),
                              "max_abs_diff_images_vs_torch": err,
                              "mask8_equal": bool(torch.equal(m8, ref[2])) if aux else None})
                print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        doc = {"what": "vipe_frame_ingest at native 1080 x 1920 and 720 x 1280 (both -> 328 x 584), fp32 and uint8 frames, "
                       "with and without mask + depth, one MI355X; next to the torch composition a caller runs today "
                       "(F.interpolate x 3, crops, 1/8 mask resample, [3::8,3::8] + where, vipe_enc_prep)",
               "event_timing": lines,
               "event_timing_note": f"events around {args.iters} back-to-back calls after 3 warm-up calls: at 10-13 us per call "
                                    "this is the launch rate of one small kernel from Python, not the kernel's duration; "
                                    "hip_GBps / share_of_8TBps are bytes over that call time",
               "unfused_src": unfused}
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
