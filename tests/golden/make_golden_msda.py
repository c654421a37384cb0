"""Generate the multi-scale deformable attention fixture from the reference's own Python file (build container only).

Run:  python tests/golden/make_golden_msda.py  REFERENCE_ROOT   (a checkout of the reference)

groundingdino/models/main/ms_deform_attn.py is loaded by path with `vipe`, `vipe.ext` and `vipe.ext.grounding_dino_ext`
stubbed as empty modules (the technique of make_golden.py); its `multi_scale_deformable_attn_pytorch` (:92-134, the
grid_sample composition) then runs on the CPU in float64 under autograd.  Each case stores its inputs, the output and
the three gradients for a fixed grad_output.  Only DATA is written: ms_deform_attn_reference.npz next to this script.
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None
MSDA = "vipe/priors/track_anything/groundingdino/models/main/ms_deform_attn.py"

# name: (bs, heads, C, level shapes (H, W), Lq, P)
CASES = {
    "multi_level": (2, 8, 8, [(5, 6), (3, 4), (1, 4), (2, 1)], 6, 4),
    "one_head_c32": (2, 1, 32, [(5, 7), (1, 1), (3, 2)], 6, 1),
    "c32_heads8": (2, 8, 32, [(3, 4), (1, 2), (2, 1)], 4, 4),
    "single_level_p1": (2, 8, 8, [(4, 5)], 9, 1),
}


def load_reference():
    for name in ["vipe", "vipe.ext"]:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    gd = types.ModuleType("vipe.ext.grounding_dino_ext")
    sys.modules["vipe.ext.grounding_dino_ext"] = gd
    sys.modules["vipe.ext"].grounding_dino_ext = gd
    spec = importlib.util.spec_from_file_location("ref_ms_deform_attn", os.path.join(REF, MSDA))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(fn, seed, bs, heads, C, shapes, Lq, P):
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    ss = torch.tensor(shapes, dtype=torch.int64)
    areas = ss[:, 0] * ss[:, 1]
    lsi = torch.cat([torch.zeros(1, dtype=torch.int64), areas.cumsum(0)[:-1]])
    Lv = int(areas.sum())
    value = torch.randn(bs, Lv, heads, C, generator=g, dtype=torch.float64).requires_grad_()
    loc = (torch.rand(bs, Lq, heads, L, P, 2, generator=g, dtype=torch.float64) * 1.2 - 0.1).requires_grad_()
    attn = torch.rand(bs, Lq, heads, L, P, generator=g, dtype=torch.float64)
    attn = (attn / attn.sum((-1, -2), keepdim=True)).detach().requires_grad_()
    out = fn(value, ss, loc, attn)
    grad_output = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(grad_output)
    arr = lambda t: t.detach().numpy().copy()  # noqa: E731
    return {"value": arr(value), "spatial_shapes": arr(ss), "level_start_index": arr(lsi), "sampling_loc": arr(loc),
            "attn_weight": arr(attn), "output": arr(out), "grad_output": arr(grad_output), "grad_value": arr(value.grad),
            "grad_sampling_loc": arr(loc.grad), "grad_attn_weight": arr(attn.grad)}


def main():
    if REF is None:
        sys.exit(__doc__)
    mod = load_reference()
    data = {}
    for i, (name, spec) in enumerate(CASES.items()):
        for k, v in make_case(mod.multi_scale_deformable_attn_pytorch, 100 + i, *spec).items():
            data[f"{name}/{k}"] = v
    data["cases"] = np.array(list(CASES))
    path = os.path.join(HERE, "ms_deform_attn_reference.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
