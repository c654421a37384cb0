"""Writes fused_lookup_parent_bits.npz: the output of the fused lookup + 1x1 convolution (`corr_lookup_conv_kernel`)
computed BEFORE the kernel became half-CU workgroups of 64 pixels with the next group's rows loading under the current
group's arithmetic.  Run on the GPU from a checkout of the parent commit (copy this file into its tests/golden/: the
parent's library lacks `vipe_corr_lookup_conv1x1_ex`, so the current Python package does not load it):

    python tests/golden/make_golden_fused_lookup_parent.py --out tests/golden/fused_lookup_parent_bits.npz

tests/test_gpu_fused_lookup_resident.py::test_bits_unchanged_from_parent runs `run_case` on the current build and compares
bits.  The kernel has no atomics and a fixed accumulation order, so every array repeats exactly (checked below).

Inputs: seeded feature maps, the correlation encoder's first layer of `UpdateModule` under `torch.manual_seed(0)`, ReLU;
E = 2 on the 8 x 64 grid in both pyramid layouts (one array in the file: the parent writes the same bits from either, which
is asserted before it is saved) and on the 9 x 18 grid in the padded blocked layout; coordinates anywhere in
[-3, w + 6) x [-3, h + 6), one row of pixels at -50 (windows wholly outside the map).
"""

import argparse
import os
import sys

import numpy as np

GOLD = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(GOLD))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CASES = [("reference_8x64", 8, 64, False), ("blocked_8x64", 8, 64, True), ("blocked_9x18", 9, 18, True)]
E = 2
GOLDEN_KEY = {"reference_8x64": "8x64", "blocked_8x64": "8x64", "blocked_9x18": "blocked_9x18"}  # case -> array of the file


def case_inputs(h, w, blocked, dev):
    """-> (levels, coords, grid) of one case, on the device"""
    import torch
    from vipe_amd.ext import droid_net_ext
    g = torch.Generator().manual_seed(1000 * h + w)
    f1 = torch.randn(E, 128, h, w, generator=g).half().to(dev)
    f2 = torch.randn(E, 128, h, w, generator=g).half().to(dev)
    levels = droid_net_ext.corr_pyramid_build(f1, f2, 4)
    if blocked:
        levels = droid_net_ext.pyramid_to_blocked(levels, h, w)
    coords = torch.rand(E, h, w, 2, generator=g) * torch.tensor([w + 9.0, h + 9.0]) - 3.0
    coords[1, h // 2] = -50.0
    return levels, coords.to(dev).contiguous(), (h, w)


def run_case(**launch):
    """-> dict of uint16 arrays [E,h,w,128] computed by the device; `launch`: keyword arguments of the current build's
    `corr_lookup_conv1x1` (the parent's has none of them)"""
    import torch
    from vipe_amd.ext import droid_net_ext
    from vipe_amd.slam.networks import UpdateModule
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    eng = UpdateModule().eval().engine(dev)
    out = {}
    for name, h, w, blocked in CASES:
        levels, coords, grid = case_inputs(h, w, blocked, dev)
        o = torch.zeros(E, h, w, 128, dtype=torch.float16, device=dev)
        droid_net_ext.corr_lookup_conv1x1(levels, coords, eng.corr0.packed, eng.corr0.bias, o, act="relu", grid=grid, **launch)
        out[name] = o.cpu().numpy().view(np.uint16)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    arrays = run_case()
    again = run_case()
    for k, v in arrays.items():
        assert v.dtype == np.uint16 and np.array_equal(v, again[k]), f"{k} does not repeat"
        assert np.count_nonzero(v) > v.size // 8, f"{k} is mostly zero"
    # the two layouts hold the same pyramid and the kernel reads the same values from either: one copy serves both
    assert np.array_equal(arrays["reference_8x64"], arrays["blocked_8x64"]), "the layouts disagree on the parent"
    arrays = {GOLDEN_KEY[k]: v for k, v in arrays.items()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print("wrote", a.out, {k: v.shape for k, v in arrays.items()}, os.path.getsize(a.out), "bytes")
