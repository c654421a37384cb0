"""Generate the panorama-camera convention fixture from the reference's own Python files (build container only).

Run:  python tests/golden/make_golden_panorama.py  REFERENCE_ROOT   (a checkout of the reference)

vipe/utils/cameras.py and vipe/utils/geometry.py are loaded by path with the packages they import but do not need here
(`pycg.isometry`, `vipe.ext.lietorch`) stubbed as empty modules (the technique of make_golden_msda.py).  Recorded, in
float64: `PanoramaCameraModel.iproj_disp` (cameras.py:366-387) on seeded normalised coordinates, and
`project_points_to_panorama` (geometry.py:89-120) on seeded points.  Only DATA is written:
panorama_camera_reference.npz next to this script.
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else None


def load(name, relpath):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, relpath))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def stub(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def main():
    if REF is None:
        sys.exit(__doc__)
    dummy = type("Dummy", (), {})
    stub("pycg")
    stub("pycg.isometry", Isometry=dummy, Quaternion=dummy)
    stub("vipe")
    stub("vipe.ext")
    stub("vipe.ext.lietorch", SE3=dummy, SO3=dummy, LieGroupParameter=dummy, Sim3=dummy)
    cameras = load("ref_cameras", "vipe/utils/cameras.py")
    geometry = load("ref_geometry", "vipe/utils/geometry.py")
    g = torch.Generator().manual_seed(360)
    n = 300
    un = torch.rand(n, generator=g, dtype=torch.float64)
    vn = torch.rand(n, generator=g, dtype=torch.float64) * 0.98 + 0.01
    disp = torch.rand(n, generator=g, dtype=torch.float64) + 0.1
    model = cameras.PanoramaCameraModel(torch.zeros(4, dtype=torch.float64))
    xyzd, _, _ = model.iproj_disp(disp, un, vn)
    pts = torch.randn(n, 3, generator=g, dtype=torch.float64) * 2.0
    uvd = geometry.project_points_to_panorama(pts, return_depth=True)
    path = os.path.join(HERE, "panorama_camera_reference.npz")
    np.savez_compressed(path, un=un.numpy(), vn=vn.numpy(), disp=disp.numpy(), xyzd=xyzd.numpy(), points=pts.numpy(),
                        uvd=uvd.numpy(), camera_type=np.array(cameras.CameraType.PANORAMA.value))
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
