"""Generate the native-resolution frame-ingest fixture from the reference's own Python files (build container only).

Run:  python tests/golden/make_golden_ingest.py  REFERENCE_ROOT   (a checkout of the reference)

vipe/streams/base.py (`VideoFrame.resize` / `crop`) and vipe/slam/system.py (`StandardResizeStreamProcessor`,
`SLAMSystem._precompute_features`, the sensor-disparity lines of `_add_keyframe`) are loaded by path; everything they
import for type annotations, logging or the rest of the SLAM system (`rerun`, `omegaconf`, `vipe.ext.lietorch`,
`vipe.priors.depth`, `vipe.utils.*`, the sibling component modules) is a stand-in module whose attributes are empty
classes - the technique of make_golden.py.  Only DATA is written: frame_ingest_reference.npz next to this script.

(a) policy/*: for every native size of SIZES what `_compute_frame_size_crop` decides - (h1, w1), the four crops,
    fac_x, fac_y, scx, scy - and a pinhole and a 5-element MEI intrinsics row carried through
    `VideoFrame.resize(...).crop(...)` (K_fwd) and back through `recover_intrinsics` (K_rec).
(b) <case>/*: `VideoFrame.resize(size).crop(...)` at explicit small sizes on random rgb, a blob mask and depth with a zero
    patch: the inputs, the cropped rgb, the cropped thresholded mask, the 1/8 INVALID mask of `_precompute_features` on
    it, and `metric_depth[3::8, 3::8]` after `d > 0 ? 1/d : d`.

Two conditions are asserted here so that the tests can demand exact mask equality: no resized-mask value lies within
1e-3 of the 0.9 threshold before thresholding (another seed is tried when one does), and every stored 1/8 mask has both
True and False cells."""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None

SIZES = [(1080, 1920), (720, 1280), (2160, 3840), (480, 640), (384, 512), (328, 584),
         (1920, 1080), (1280, 720), (3840, 2160), (640, 480), (854, 480),                    # portrait
         (1024, 1024), (600, 800), (768, 1024), (1200, 1600), (1440, 2560), (540, 960), (360, 640), (480, 854),
         (1088, 1920), (2048, 2048), (720, 960), (576, 720), (486, 720), (1556, 2048), (3000, 4000), (1080, 2560),
         (405, 720), (721, 1283), (333, 777), (777, 333), (1000, 1500), (1234, 2345),
         (240, 320), (120, 160), (96, 160), (100, 100), (200, 300), (64, 64), (50, 75), (160, 96)]  # upscaling

# name: (native (H0, W0), resize (h1, w1), crop (top, bottom, left, right))
CASES = {
    "downscale": ((37, 53), (29, 43), (2, 3, 1, 2)),       # -> 24 x 40
    "upscale": ((19, 23), (43, 61), (1, 2, 2, 3)),         # -> 40 x 56
    "identity": ((24, 40), (24, 40), (0, 0, 0, 0)),        # -> 24 x 40
    "mixed_ratio": ((31, 70), (45, 50), (2, 3, 1, 1)),     # rows up, columns down -> 40 x 48
}

K_PINHOLE = [1234.5, 1240.25, 961.75, 543.5]
K_MEI = [820.0, 815.5, 640.25, 355.75, 0.875]


class _Stub(types.ModuleType):
    """A module every attribute of which is an empty class (annotations and base classes evaluate; nothing runs)."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        cls = type(name, (), {})
        setattr(self, name, cls)
        return cls


def _stub(name, **attrs):
    m = _Stub(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, child = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], child, m)
    return m


def _load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    for name in ["vipe", "vipe.ext", "vipe.ext.lietorch", "vipe.utils", "vipe.utils.cameras", "vipe.utils.logging",
                 "vipe.utils.misc", "vipe.priors", "vipe.priors.depth", "vipe.priors.depth.base", "vipe.streams",
                 "vipe.slam", "vipe.slam.components", "vipe.slam.components.backend", "vipe.slam.components.buffer",
                 "vipe.slam.components.frontend", "vipe.slam.components.inner_filler",
                 "vipe.slam.components.motion_filter", "vipe.slam.components.sparse_tracks", "vipe.slam.interface",
                 "vipe.slam.networks", "vipe.slam.networks.droid_net", "rerun"]:
        _stub(name)
    sys.modules["vipe.utils.cameras"].CameraType = type("CameraType", (), {"PINHOLE": 0, "MEI": 1})  # a default reads it
    for name, attrs in (("omegaconf", {}), ("einops", {"rearrange": lambda x, pattern: x.permute(0, 3, 1, 2)})):
        try:
            importlib.import_module(name)
        except ImportError:
            _stub(name, **attrs)
    base = _load("vipe.streams.base", "vipe/streams/base.py")
    sys.modules["vipe.streams"].base = base
    system = _load("vipe.slam.system", "vipe/slam/system.py")
    return base, system


def policy_table(base, system):
    rows_i, rows_f, k_fwd, k_rec = [], [], [], []
    for h0, w0 in SIZES:
        proc = system.StandardResizeStreamProcessor()
        (h1, w1), crops = proc._compute_frame_size_crop((h0, w0))
        rows_i.append([h0, w0, h1, w1, *crops, proc.scx, proc.scy])
        rows_f.append([proc.fac_x, proc.fac_y])
        fwd, rec = [], []
        for K in (K_PINHOLE, K_MEI):
            # the intrinsics go the frame's own way: VideoFrame.resize -> crop (a one-pixel-high stand-in for the image
            # would change size(); the frame is real, its content irrelevant)
            frame = base.VideoFrame(raw_frame_idx=0, rgb=torch.zeros(h0, w0, 3), intrinsics=torch.tensor(K, dtype=torch.float64))
            out = proc(0, frame)
            assert out.size() == proc.update_frame_size((h0, w0)) and out.size()[0] % 8 == 0 and out.size()[1] % 8 == 0
            fwd.append(np.pad(out.intrinsics.numpy(), (0, 5 - len(K))))
            rec.append(np.pad(proc.recover_intrinsics(out.intrinsics).numpy(), (0, 5 - len(K))))
        k_fwd.append(fwd)
        k_rec.append(rec)
    ints = np.array(rows_i, dtype=np.int64)
    assert ((ints[:, 2] % 8) % 2 == 1).any() and ((ints[:, 3] % 8) % 2 == 1).any(), "no unequal crop halves in SIZES"
    assert (ints[:, 2] > ints[:, 0]).any() and (ints[:, 2] < ints[:, 0]).any(), "SIZES must scale both ways"
    return {"policy/ints": ints, "policy/factors": np.array(rows_f, dtype=np.float64),
            "policy/K_in": np.array([np.pad(K_PINHOLE, (0, 1)), K_MEI], dtype=np.float64),
            "policy/K_fwd": np.array(k_fwd, dtype=np.float64), "policy/K_rec": np.array(k_rec, dtype=np.float64)}


def make_case(base, system, seed, native, size, crops):
    g = torch.Generator().manual_seed(seed)
    H0, W0 = native
    rgb = torch.rand(H0, W0, 3, generator=g)
    depth = 0.5 + 9.5 * torch.rand(H0, W0, generator=g)
    py, px = int(torch.randint(0, H0 - H0 // 3, (1,), generator=g)), int(torch.randint(0, W0 - W0 // 3, (1,), generator=g))
    depth[py:py + H0 // 3, px:px + W0 // 3] = 0.0  # a patch without sensor depth
    yy, xx = torch.meshgrid(torch.arange(H0).float(), torch.arange(W0).float(), indexing="ij")
    cy, cx = (0.3 + 0.4 * torch.rand(2, generator=g)) * torch.tensor([H0, W0])
    ry, rx = (0.18 + 0.12 * torch.rand(2, generator=g)) * torch.tensor([H0, W0])
    mask = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 > 1.0  # True = usable pixel; the blob is not
    soft = torch.nn.functional.interpolate(mask[None, None].float(), size, mode="bilinear")[0, 0]
    if bool(((soft - 0.9).abs() < 1e-3).any()):
        return None
    frame = base.VideoFrame(raw_frame_idx=0, rgb=rgb, mask=mask, metric_depth=depth)
    top, bottom, left, right = crops
    out = frame.resize(size).crop(top=top, bottom=bottom, left=left, right=right)
    assert out.size()[0] % 8 == 0 and out.size()[1] % 8 == 0
    _, masks = system.SLAMSystem._precompute_features(None, [out])
    d = out.metric_depth[3::8, 3::8]
    disps = torch.where(d > 0, d.reciprocal(), d)  # system.py:153-154
    if not (bool(masks.any()) and not bool(masks.all())):
        return None
    return {"rgb": rgb.numpy(), "mask": mask.numpy(), "depth": depth.numpy(), "geometry": np.array([*size, *crops]),
            "rgb_out": out.rgb.contiguous().numpy(), "mask_out": out.mask.contiguous().numpy(),
            "mask8": masks[0].numpy(), "disps_sens": disps.contiguous().numpy()}


def main():
    if REF is None:
        sys.exit(__doc__)
    base, system = load_reference()
    data = policy_table(base, system)
    for i, (name, spec) in enumerate(CASES.items()):
        for attempt in range(50):
            case = make_case(base, system, 1000 * (i + 1) + attempt, *spec)
            if case is not None:
                break
        assert case is not None, name
        m8 = case["mask8"]
        assert m8.any() and not m8.all(), name
        for k, v in case.items():
            data[f"{name}/{k}"] = v
        print(name, "seed", 1000 * (i + 1) + attempt, "out", case["rgb_out"].shape, "invalid cells", int(m8.sum()), "of", m8.size)
    data["cases"] = np.array(list(CASES))
    path = os.path.join(HERE, "frame_ingest_reference.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
