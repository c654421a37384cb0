"""`vipe_depth_consistency` on the device against the float64 reference of tests/depth_consistency_reference.py, on its
seeded cases ((24, 40) maps - more than one 64 x 4 tile in both directions after the export geometry, sizes that are no
multiple of the tile): the three cameras, identity / crop and upsampling / downsampling / pure resize, a two-view rig,
K = 1 and K = 8, neighbour entries that name nothing, rows that repeat or name nothing, non-positive source pixels and
neighbour taps, the empty batch.  Criterion (`compare`): a pixel whose pairs are all decided has the reference's byte;
any other pixel's nibbles differ by at most the number of its undecided pairs; a map without a row keeps its sentinel."""
import numpy as np
import pytest
import torch

import depth_consistency_reference as cr
import depth_export_reference as dr

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def on_device(case, fresh_out=False, **over):
    from vipe_amd.slam.ingest import depth_consistency
    c = {**case, **over}
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    N = c["nbr"].shape[0]
    out = None if fresh_out else torch.full((N, c["params"][4], c["params"][5]), cr.SENTINEL, dtype=torch.uint8, device=dev())
    got = depth_consistency(t(c["disp"]), t(c["poses"]), t(c["rig"]), t(c["intrinsics"]), c["camera"], c["params"],
                            t(c["rows"]), t(c["nbr"]), c["tol"], out=out)
    assert out is None or got is out
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("name", cr.CASES)
def test_kernel_matches_reference(name):
    case, ref = cr.cached_case(name)
    s = cr.summary(ref)
    assert s["undecided"] <= 0.02 * s["total"], "the cap on undecided pairs, on the very inputs the device gets"
    got = on_device(case)
    exact, loose = cr.compare(got, ref)
    diff = int((got[ref["written"]] != ref["byte"][ref["written"]]).sum())
    print(f"{name}: {exact} pixels compared exactly, {loose} with undecided pairs ({diff} of those differ), pairs {s}")
    assert exact > 0.9 * (exact + loose)


def test_fresh_output_is_zero_filled_and_rows_default_to_identity():
    case, ref = cr.cached_case("pinhole_identity")
    assert case["rows"] is None and ref["written"].all()
    got = on_device(case, fresh_out=True)
    cr.compare(got, ref)
    # a map without a row in a fresh output: zeros
    edge, eref = cr.cached_case("edge_entries")
    got = on_device(edge, fresh_out=True)
    assert not got[~eref["written"]].any()
    cr.compare(got, eref, sentinel=0)


def test_empty_batch():
    case, _ = cr.cached_case("pinhole_up_crop")
    got = on_device(case, rows=np.zeros(0, np.int64), nbr=np.zeros((0, 4), np.int64))
    assert got.shape == (0, 61, 97)


@pytest.mark.parametrize("camera", ["pinhole", "panorama"])
def test_analytic_scene_on_the_device(camera):
    """the ray-cast scene straight through the kernel: wherever every pair of a pixel is decided, all neighbours that
    see the point confirm it (agree == visible); with one map scaled by 1.4 on a rectangle, its pixels there find no
    agreement at all although they are seen"""
    from vipe_amd.slam.interface import unpack_depth_conf
    sc = cr.panorama_scene() if camera == "panorama" else cr.analytic_scene(camera, V=2)
    R = sc["disp"].shape[0]
    nbr = np.array([([q for q in range(R) if q != r] + [-1] * 8)[:8] for r in range(R)], dtype=np.int64)
    case = dict(sc, params=dr.identity_params(*cr.HW), rows=None, nbr=nbr, tol=0.05)
    ref = cr.depth_consistency_ref(**case)
    got = on_device(case)
    cr.compare(got, ref)
    agree, visible = (t.numpy() for t in unpack_depth_conf(torch.from_numpy(got)))
    sure = ref["undecided"] == 0
    assert sure.mean() > 0.9 and (agree[sure] == visible[sure]).all() and visible[sure].mean() > 3
    row, (y0, y1, x0, x1) = 2, (6, 18, 8, 30)
    bad = dict(case, disp=cr.corrupt(sc["disp"], row, (y0, y1, x0, x1)))
    bref = cr.depth_consistency_ref(**bad)
    got = on_device(bad)
    cr.compare(got, bref)
    agree, visible = (t.numpy() for t in unpack_depth_conf(torch.from_numpy(got)))
    sure = (bref["undecided"][row] == 0)[y0:y1, x0:x1]
    assert (agree[row, y0:y1, x0:x1][sure] == 0).all() and visible[row, y0:y1, x0:x1][sure].mean() > 3
