"""Native-resolution ingest, host side: `StandardResize` against the reference's size / crop policy and intrinsics round
trip (tests/golden/frame_ingest_reference.npz, table (a) of make_golden_ingest.py), and the argument checks of
`vipe_frame_ingest` (no GPU needed: a rejected call launches nothing)."""

import os

import numpy as np
import pytest
import torch

from vipe_amd import _lib
from vipe_amd.slam.ingest import StandardResize


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "frame_ingest_reference.npz"))


def test_fixture_covers_the_sizes_that_matter(gold):
    ints = gold["policy/ints"]
    sizes = {(int(r[0]), int(r[1])) for r in ints}
    assert len(sizes) >= 40
    assert {(1080, 1920), (720, 1280), (2160, 3840), (480, 640), (384, 512), (328, 584)} <= sizes
    assert any(h > w for h, w in sizes)                                                  # portrait
    assert ((ints[:, 4] != ints[:, 5]).any() and (ints[:, 6] != ints[:, 7]).any())       # unequal crop halves
    assert (ints[:, 2] > ints[:, 0]).any()                                               # upscaling


def test_standard_resize_reproduces_the_reference_policy(gold):
    for row, fac in zip(gold["policy/ints"], gold["policy/factors"]):
        h0, w0, h1, w1, top, bottom, left, right, scx, scy = (int(x) for x in row)
        r = StandardResize(h0, w0)
        assert r.size == (h1, w1), (h0, w0)
        assert r.crop == (top, bottom, left, right), (h0, w0)
        assert r.out_size == (h1 - top - bottom, w1 - left - right) and r.out_size[0] % 8 == 0 and r.out_size[1] % 8 == 0
        assert (r.scx, r.scy) == (scx, scy)
        assert r.fac_x == fac[0] and r.fac_y == fac[1], (h0, w0)  # the same float64 quotients, bit for bit


def test_intrinsics_round_trip_matches_the_reference(gold):
    K_in = gold["policy/K_in"]
    for i, row in enumerate(gold["policy/ints"]):
        r = StandardResize(int(row[0]), int(row[1]))
        for j, n in enumerate((4, 5)):  # pinhole, MEI (the fifth coefficient is left alone)
            K = torch.from_numpy(K_in[j, :n].copy())
            fwd = r.forward_intrinsics(K)
            rec = r.recover_intrinsics(fwd)
            assert fwd.shape == (n,) and rec.shape == (n,)
            np.testing.assert_allclose(fwd.numpy(), gold["policy/K_fwd"][i, j, :n], rtol=1e-6, atol=0)
            np.testing.assert_allclose(rec.numpy(), gold["policy/K_rec"][i, j, :n], rtol=1e-6, atol=0)
            np.testing.assert_allclose(rec.numpy(), K_in[j, :n], rtol=1e-6, atol=0)  # forward then recover returns K
            if n == 5:
                assert fwd[4].item() == K_in[j, 4] and rec[4].item() == K_in[j, 4]
            assert torch.equal(K, torch.from_numpy(K_in[j, :n]))  # the argument is not modified


def test_intrinsics_round_trip_in_float32():
    K = torch.tensor([1234.5, 1240.25, 961.75, 543.5], dtype=torch.float32)
    for h0, w0 in ((1080, 1920), (96, 160), (777, 333)):
        r = StandardResize(h0, w0)
        rec = r.recover_intrinsics(r.forward_intrinsics(K))
        assert rec.dtype == torch.float32
        np.testing.assert_allclose(rec.numpy(), K.numpy(), rtol=1e-6, atol=0)


def test_abi_exposes_frame_ingest_and_rejects_bad_geometry():
    protos = _lib.parse_header()
    assert "vipe_frame_ingest" in protos and len(protos["vipe_frame_ingest"][1]) == 17
    L = _lib.lib()
    p = 0x1000  # never dereferenced: every call below is rejected before a launch

    def call(rgb=p, dtype=_lib.F32, mask=None, depth=None, H0=37, W0=53, h1=29, w1=43, top=2, left=1, H=24, W=40,
             images=p, x4=p, mask8=None, disps=None):
        return L.vipe_frame_ingest(rgb, dtype, mask, depth, H0, W0, h1, w1, top, left, H, W, images, x4, mask8, disps, None)

    assert call(H=25) == -1 and call(W=36) == -1            # not multiples of 8
    assert call(top=6) == -1 and call(left=4) == -1         # the crop leaves (h1, w1)
    assert call(top=-1) == -1 and call(left=-1) == -1
    assert call(H=0) == -1 and call(h1=0) == -1 and call(H0=0) == -1
    assert call(rgb=None) == -1 and call(images=None) == -1 and call(x4=None) == -1
    assert call(dtype=_lib.F64) == -1 and call(dtype=7) == -1
    assert call(mask=p) == -1 and call(depth=p) == -1       # an input without the output it fills
