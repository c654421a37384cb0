"""The fused lookup + 1x1 convolution as half-CU persistent workgroups (`corr_lookup_conv_kernel`): 64 pixels per pass, the
next group's rows loading under the current group's arithmetic, coordinates and slots fetched a group further ahead,
every prefetch past the last group clamped to it.

What can go wrong is in the walk - which group a workgroup takes next, what its prefetches read behind the end, whose
rows are in the registers when a level is computed - so the grids are tiny and `max_workgroups` makes single workgroups
walk many groups.  Everything is compared bit for bit: against oracle/corr.py through 0/1 convolution weights (all 196
channels), between launch forms, and against the parent commit's kernel (tests/golden/fused_lookup_parent_bits.npz).
"""

import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def identity_lookup(levels, coords, slots, grid, **launch):
    """all 196 channels of the fused kernel, bit for bit: 0/1 weights copy channels 0..127, then 68..195 (one fp16 value
    x 1.0 accumulated in fp32 and rounded back is itself) - tests/test_gpu_grids.py::_identity_lookup with a launch form"""
    from vipe_amd.ext import droid_net_ext
    from vipe_amd.slam.update_engine import _Packed
    E, h, w = coords.shape[:3]
    out = torch.zeros(E, h, w, 196, dtype=torch.float16, device=dev())
    for c0 in (0, 68):
        wt = torch.zeros(128, 200, 1, 1)
        wt[torch.arange(128), c0 + torch.arange(128)] = 1.0
        pk = _Packed(wt.half(), torch.zeros(128), dev())
        o = torch.empty(E, h, w, 128, dtype=torch.float16, device=dev())
        droid_net_ext.corr_lookup_conv1x1(levels, coords, pk.packed, pk.bias, o, act="none", slots=slots, grid=grid, **launch)
        out[..., c0:c0 + 128] = o
    return out


def oracle_lookup(reference_levels, coords):
    """oracle/corr.py on the device pyramid -> [E,h,w,196] uint16"""
    from oracle import corr as ocorr
    ref = ocorr.corr_lookup([x.cpu().numpy() for x in reference_levels], coords.cpu().numpy()[None], 3)[0]  # [E,196,h,w]
    return np.ascontiguousarray(ref.transpose(0, 2, 3, 1)).view(np.uint16)


def bits(t):
    return t.cpu().numpy().view(np.uint16)


def anywhere(E, h, w, g):
    """coordinates uniform in [-3, w + 6) x [-3, h + 6), one row of pixels at -50 (windows wholly outside the map)"""
    coords = torch.rand(E, h, w, 2, generator=g) * torch.tensor([w + 9.0, h + 9.0]) - 3.0
    coords[E - 1, h // 2] = -50.0
    return coords.to(dev()).contiguous()


@functools.lru_cache(maxsize=None)
def case_8x64():
    """E = 3 on the 8 x 64 grid (8 groups of 64 pixels per edge) in both layouts, the oracle's lookup and the default
    launch's result per layout"""
    from vipe_amd.ext import droid_net_ext
    E, h, w = 3, 8, 64
    g = torch.Generator().manual_seed(31)
    f1 = torch.randn(E, 128, h, w, generator=g).half().to(dev())
    f2 = torch.randn(E, 128, h, w, generator=g).half().to(dev())
    ref_lv = droid_net_ext.corr_pyramid_build(f1, f2, 4)
    coords = anywhere(E, h, w, g)
    layouts = {"reference": ref_lv, "blocked": droid_net_ext.pyramid_to_blocked(ref_lv, h, w)}
    assert layouts["blocked"][0].dim() == 7
    default = {k: bits(identity_lookup(lv, coords, None, (h, w))) for k, lv in layouts.items()}
    return layouts, coords, oracle_lookup(ref_lv, coords), default


@pytest.mark.parametrize("layout", ["reference", "blocked"])
def test_many_passes_per_workgroup(layout):
    """24 groups walked by 1, 2, 3 and 5 workgroups: up to 24 passes each, odd and even pass counts, a last round that
    not every workgroup takes part in (24 = 4 x 5 + 4), prefetches one and two steps past the end in every workgroup"""
    layouts, coords, want, default = case_8x64()
    assert np.array_equal(default[layout], want), "default launch differs from the oracle"
    for m in (1, 2, 3, 5):
        got = bits(identity_lookup(layouts[layout], coords, None, (8, 64), max_workgroups=m))
        assert np.array_equal(got, default[layout]), f"max_workgroups={m} differs from the default launch"


@pytest.mark.parametrize("layout", ["reference", "blocked"])
def test_shared_cu_launch_has_the_same_bits(layout):
    """share_cu only changes how many workgroups a compute unit holds (its LDS request) and the grid"""
    layouts, coords, want, default = case_8x64()
    for m in (0, 1, 2, 3, 5):
        got = bits(identity_lookup(layouts[layout], coords, None, (8, 64), max_workgroups=m, share_cu=True))
        assert np.array_equal(got, default[layout]), f"share_cu with max_workgroups={m} differs"


@pytest.mark.parametrize("grid", [(9, 18), (41, 73)])
def test_ragged_pixel_count_and_permuted_slots(grid):
    """162 and 2993 pixels per edge (last group of 34 / 49 pixels: its other lanes read the last pixel's rows and store
    nothing), pyramids in pool slots that are not the edges' order, windows over every border and wholly outside"""
    from vipe_amd.slam.networks import CorrPool
    h, w = grid
    g = torch.Generator().manual_seed(1000 * h + w)
    fmaps = torch.randn(4, 128, h, w, generator=g).half().to(dev())
    ii, jj = torch.tensor([0, 1, 3, 2, 3]), torch.tensor([1, 0, 3, 0, 1])
    E = 5
    # slots 0..2 filled with (2, 2), edge 0 and (3, 2); the first and the last dropped again; the other four edges take
    # the freed slots and new ones: the slot vector is no identity
    pool = CorrPool(capacity=4)
    pool.add_edges(fmaps, torch.tensor([2, 0, 3], device=dev()), torch.tensor([2, 1, 2], device=dev()), frame_range=(0, 4))
    pool = pool[np.array([1])]
    pool.add_edges(fmaps, ii[1:].to(dev()), jj[1:].to(dev()))
    assert len(pool) == E and pool.blocked
    assert not torch.equal(pool.slots.cpu().long(), torch.arange(E)), "the slot vector should not be the identity"
    lv = pool.corr_pyramid
    coords = anywhere(E, h, w, g)
    hd = pool.lookup_deferred(coords)
    assert hd[0] == "lookup" and hd[3] is not None and hd[4] == (h, w)
    want = oracle_lookup(lv, coords)
    # the pool holds the edges asked for (level 0 against the fp32 contraction), so `want` is no self-comparison
    f1, f2 = fmaps[ii.to(dev())], fmaps[jj.to(dev())]
    ref0 = torch.matmul((f1.float() / 4).reshape(E, 128, h * w).transpose(1, 2), (f2.float() / 4).reshape(E, 128, h * w))
    d0 = (lv[0].float().reshape(E, h * w, h * w) - ref0).abs()
    assert float((d0 - ref0.abs() * 2.0 ** -10).max()) <= 2.0 ** -14
    for m in (1, 2, 7):
        got = bits(identity_lookup(hd[1], hd[2], hd[3], hd[4], max_workgroups=m))
        assert np.array_equal(got, want), f"max_workgroups={m} differs from the oracle"


def test_fewer_groups_than_workgroups():
    """one group: a single workgroup whose prefetches all fall behind the end"""
    from vipe_amd.ext import droid_net_ext
    h = w = 8  # level 3 is 1 x 1: blocked layout only (the reference layout needs 8-column rows down to level 3)
    g = torch.Generator().manual_seed(8)
    f1 = torch.randn(1, 128, h, w, generator=g).half().to(dev())
    f2 = torch.randn(1, 128, h, w, generator=g).half().to(dev())
    ref_lv = droid_net_ext.corr_pyramid_build(f1, f2, 4)
    coords = anywhere(1, h, w, g)
    lv = droid_net_ext.pyramid_to_blocked(ref_lv, h, w)
    assert np.array_equal(bits(identity_lookup(lv, coords, None, (h, w))), oracle_lookup(ref_lv, coords))


def test_results_beside_a_neighbour_on_another_stream():
    """The operator's first fork: the lookup (share_cu) on one stream, the flow encoder's 7x7 and 3x3 convolutions on
    another, both writing channel ranges of one [E,h,w,320] buffer.  Same results as the same launches on one stream."""
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    from vipe_amd.ext import droid_net_ext
    from vipe_amd.slam.networks import UpdateModule
    E, h, w = 4, 24, 64
    torch.manual_seed(0)
    eng = UpdateModule().eval().engine(dev())
    g = torch.Generator().manual_seed(5)
    f1 = torch.randn(E, 128, h, w, generator=g).half().to(dev())
    f2 = torch.randn(E, 128, h, w, generator=g).half().to(dev())
    lv = droid_net_ext.corr_pyramid_build(f1, f2, 4, layout=droid_net_ext.BLOCKED)
    coords = anywhere(E, h, w, g)
    motn = (torch.randn(E, h, w, 4, generator=g) * 2).half().to(dev())

    def lookup(xbuf):
        droid_net_ext.corr_lookup_conv1x1(lv, coords, eng.corr0.packed, eng.corr0.bias, xbuf, out_coff=128, act="relu",
                                          grid=(h, w), share_cu=True)

    def flow_encoder(xbuf, fbuf):
        check(lib().vipe_conv2d_fused(ptr(motn), 4, 0, None, 0, 0, 4, ptr(eng.flow0.packed), ptr(eng.flow0.bias), None, 0, 0,
                                      ptr(fbuf), 128, 0, None, 0, 0, None, 0, 0, None, None, None, 0, 0, E, h, w, 4, 128, 7, 7,
                                      1, 0, stream_ptr(motn)), "flow0")
        check(lib().vipe_conv2d_fused(ptr(fbuf), 128, 0, None, 0, 0, 128, ptr(eng.flow2.packed), ptr(eng.flow2.bias), None, 0, 0,
                                      ptr(xbuf), 320, 256, None, 0, 0, None, 0, 0, None, None, None, 0, 0, E, h, w, 128, 64, 3,
                                      3, 1, 0, stream_ptr(fbuf)), "flow2")

    def buffers():
        return (torch.full((E, h, w, 320), 3.0, dtype=torch.float16, device=dev()),
                torch.zeros(E, h, w, 128, dtype=torch.float16, device=dev()))

    x1, fb1 = buffers()
    lookup(x1)
    flow_encoder(x1, fb1)
    x2, fb2 = buffers()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    lookup(x2)
    with torch.cuda.stream(side):
        flow_encoder(x2, fb2)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(x1, x2) and torch.equal(fb1, fb2)
    assert torch.all(x1[..., :128] == 3.0), "channels of neither kernel were written"
    assert float(x1[..., 128:256].float().abs().max()) > 0 and float(x1[..., 256:].float().abs().max()) > 0


def test_bits_unchanged_from_parent():
    """the cases of tests/golden/make_golden_fused_lookup_parent.py on the current build, in the default, the capped and the
    shared-CU launch form, against what the parent commit's kernel wrote"""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_fused_lookup_parent as gen
    want = np.load(os.path.join(GOLDEN, "fused_lookup_parent_bits.npz"))
    assert sorted(want.files) == sorted(set(gen.GOLDEN_KEY.values()))
    for launch in ({}, {"max_workgroups": 3}, {"share_cu": True}):
        got = gen.run_case(**launch)
        assert sorted(got) == sorted(gen.GOLDEN_KEY)
        for k, v in got.items():
            w = want[gen.GOLDEN_KEY[k]]
            assert v.shape == w.shape and np.array_equal(v, w), (k, launch)
