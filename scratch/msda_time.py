"""grounding_dino_ext.ms_deform_attn_{forward,backward} at GroundingDINO's shapes (8 heads x 32 channels, 4 levels x 4
points, 16:9 video at a short side of 800: levels 94x167, 47x84, 24x42, 12x21), event-timed on the current stream next
to the torch grid_sample composition (multi_scale_deformable_attn_pytorch) on the same GPU, fp32.

    python scratch/msda_time.py [--iters N]      one JSON line per (shape, path)

encoder: Lq = Lv = 20906 queries; decoder: Lq = 900.  "gathered" counts the corner bytes the forward reads
(Lq * heads * L * P * 4 corners * C * 4 B); the backward adds as many atomically added bytes to grad_value."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vipe_amd.ext import grounding_dino_ext as gd  # noqa: E402

LEVELS = [(94, 167), (47, 84), (24, 42), (12, 21)]
HEADS, C, P = 8, 32, 4


def compose(value, shapes, loc, attn):
    bs, _, heads, ch = value.shape
    _, Lq, _, L, P_, _ = loc.shape
    vals = value.split([h * w for h, w in shapes], dim=1)
    grids = 2 * loc - 1
    sampled = []
    for lvl, (h, w) in enumerate(shapes):
        v = vals[lvl].flatten(2).transpose(1, 2).reshape(bs * heads, ch, h, w)
        g = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(v, g, mode="bilinear", padding_mode="zeros", align_corners=False))
    a = attn.transpose(1, 2).reshape(bs * heads, 1, Lq, L * P_)
    return (torch.stack(sampled, dim=-2).flatten(-2) * a).sum(-1).view(bs, heads * ch, Lq).transpose(1, 2).contiguous()


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    ss = torch.tensor(LEVELS, dtype=torch.int64, device=dev)
    areas = ss[:, 0] * ss[:, 1]
    lsi = torch.cat([areas.new_zeros(1), areas.cumsum(0)[:-1]])
    Lv = sum(h * w for h, w in LEVELS)
    value = torch.randn(1, Lv, HEADS, C, generator=g).to(dev)
    for name, Lq in (("encoder", Lv), ("decoder", 900)):
        # reference points in [0, 1] plus offsets of a few pixels, as the layers produce them
        loc = (torch.rand(1, Lq, 1, 1, 1, 2, generator=g) + torch.randn(1, Lq, HEADS, 4, P, 2, generator=g) * 0.02)
        loc = loc.to(dev).contiguous()
        attn = torch.softmax(torch.randn(1, Lq, HEADS, 4 * P, generator=g), -1).view(1, Lq, HEADS, 4, P).to(dev)
        gout = torch.randn(1, Lq, HEADS * C, generator=g).to(dev)
        gathered = Lq * HEADS * 4 * P * 4 * C * 4
        fwd = event_ms(lambda: gd.ms_deform_attn_forward(value, ss, lsi, loc, attn, 64), args.iters)
        bwd = event_ms(lambda: gd.ms_deform_attn_backward(value, ss, lsi, loc, attn, gout, 64), args.iters)
        vr, lr, ar = (t.clone().requires_grad_() for t in (value, loc, attn))
        t_fwd = event_ms(lambda: compose(value, LEVELS, loc, attn), args.iters)

        def torch_fb():
            out = compose(vr, LEVELS, lr, ar)
            torch.autograd.grad(out, (vr, lr, ar), gout)

        t_fb = event_ms(torch_fb, args.iters)
        ref = compose(value, LEVELS, loc, attn)
        err = (gd.ms_deform_attn_forward(value, ss, lsi, loc, attn, 64) - ref).abs().max().item()
        print(json.dumps({"shape": name, "Lq": Lq, "Lv": Lv, "hip_forward_ms": round(fwd, 4),
                          "hip_backward_ms": round(bwd, 4), "torch_forward_ms": round(t_fwd, 4),
                          "torch_forward_backward_ms": round(t_fb, 4), "gathered_bytes": gathered,
                          "forward_gathered_TBps": round(gathered / fwd / 1e9, 3),
                          "backward_atomic_TBps": round(gathered / bwd / 1e9, 3),
                          "max_abs_diff_vs_torch": err}), flush=True)


if __name__ == "__main__":
    main()
