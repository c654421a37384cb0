"""The BA marginals' entry points without a GPU: exported under the unchanged ABI version, argument errors before any
launch, and the rescaling rule of the two output fields."""

import ctypes

import torch

from vipe_amd import _lib


def test_marginals_entry_points_are_exported_and_abi_version_stays():
    protos = _lib.parse_header()
    L = _lib.lib()
    for name, n_args in (("vipe_dense_ba_linearize", 20), ("vipe_dense_ba_marginals", 7)):
        assert name in protos and len(protos[name][1]) == n_args and hasattr(L, name)
    assert L.vipe_amd_abi_version() == 4


def test_marginals_argument_errors_do_not_launch():
    L = _lib.lib()
    p = _lib.BAParams(n_poses=4, n_views=1, ht=4, wd=6, M=0, t0=1, t1=4, camera=0, intr_factor=8.0)
    null20 = [None] * 13 + [None, 0, None, 0, None, None]
    assert L.vipe_dense_ba_linearize(ctypes.byref(p), *null20) == -1            # VIPE_EINVAL: no arrays
    assert L.vipe_dense_ba_marginals(None, None, None, 0, None, None, None) == -1
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: the view count is checked on the host before anything is launched
    p9 = _lib.BAParams(n_poses=4, n_views=9, ht=4, wd=6, M=0, t0=1, t1=4, camera=0, intr_factor=8.0)
    assert L.vipe_dense_ba_marginals(ctypes.byref(p9), fake, None, 0, None, None, None) == -3   # VIPE_EUNSUPPORTED
    args = [fake] * 5 + [None, None, fake] + [None] * 5 + [fake, 1 << 40, fake, 4096, None, None]
    assert L.vipe_dense_ba_linearize(ctypes.byref(p9), *args) == -3
    p.ht = 0
    assert L.vipe_dense_ba_marginals(ctypes.byref(p), fake, None, 0, None, None, None) == -1


def test_rescale_marginals():
    """disparities / s, translations * s: var / s^2; translation block * s^2, translation-rotation blocks * s"""
    from vipe_amd.slam.interface import rescale_marginals
    g = torch.Generator().manual_seed(0)
    A = torch.randn(3, 6, 6, generator=g, dtype=torch.float64)
    cov = A @ A.transpose(1, 2)
    var = torch.rand(3, 2, 4, 5, generator=g) + 0.1
    s = 2.5
    v2, c2 = rescale_marginals(var, cov, s)
    assert torch.allclose(v2, var / s**2)
    assert torch.allclose(c2[:, :3, :3], cov[:, :3, :3] * s**2) and torch.allclose(c2[:, 3:, 3:], cov[:, 3:, 3:])
    assert torch.allclose(c2[:, :3, 3:], cov[:, :3, 3:] * s) and torch.allclose(c2[:, 3:, :3], cov[:, 3:, :3] * s)
    # it is the covariance of (s t, phi): J cov J^T with J = diag(s, s, s, 1, 1, 1)
    J = torch.diag(torch.tensor([s, s, s, 1, 1, 1.0], dtype=torch.float64))
    assert torch.allclose(c2, J @ cov @ J)
    nan = torch.full((1, 6, 6), float("nan"), dtype=torch.float64)
    assert torch.isnan(rescale_marginals(var[:1], nan, s)[1]).all()
