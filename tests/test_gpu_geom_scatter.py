"""The slam_ext geometry kernels and the scatter kernel beyond one workgroup, against host references.

Geometry (`geom_ops.hip`): grids on both sides of the 256-lane workgroup (oracle/frame_cases.py: ragged with ~12 trips
per lane, five pixels past one workgroup, exactly one, less than a wave), pose / disparity / intrinsics indices that do
not alias, a permuted frame subset with per-entry thresholds for the depth filter - against oracle/frame_ops.py in
float32 (the kernel's operation order) and float64 (which says how much float32 may matter, and which pixels sit on a
decision boundary).  tests/test_oracle_frame_ops.py checks the inputs themselves without a GPU.

Scatter (`aux_ops.hip`): the grid-stride loop's second trip, 4096-way contention on the compare-and-swap loops, the
fp16 path on odd inner sizes and odd element offsets - against torch on the host.
"""

import functools

import numpy as np
import pytest
import torch

from oracle import frame_cases as fc
from oracle import frame_ops

pytestmark = pytest.mark.gpu

CAP = 0.005  # the share of pixels a comparison may leave out


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def T(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(dev())


# ------------------------------------------------------------------------------------------------ geometry


@pytest.mark.parametrize("grid", fc.GRIDS)
def test_frame_distance_beyond_one_workgroup(grid):
    """Every pair within 1e-4 of ITS OWN float32-oracle value (the kernel's fp32 sum - ceil(2P/256) non-negative terms
    per lane, six shuffle steps, four adds: under 40 roundings at P = 2993, ~2.4e-6 - cannot use that up); the pair that
    looks at a camera far behind the source is exactly 1000; one pair is scored over a masked subset of its pixels."""
    from vipe_amd.ext import slam_ext
    c = fc.geom_case(*grid)
    ref = frame_ops.frame_distance(c.fd_poses, c.disps, c.intr2, fc.FD_PI, fc.FD_PJ, fc.FD_QI, fc.FD_QJ, fc.FD_DI, fc.BETA)
    d = slam_ext.frame_distance(T(c.fd_poses), T(c.disps), T(c.intr2), T(fc.FD_PI), T(fc.FD_PJ), T(fc.FD_QI), T(fc.FD_QJ),
                                T(fc.FD_DI), fc.BETA).cpu().numpy()
    rel = np.abs(d - ref) / np.abs(ref)
    print("frame_distance", grid, "rel err per pair", rel)
    assert d[fc.FD_FAR] == 1000.0 and ref[fc.FD_FAR] == 1000.0
    assert ref[fc.FD_PARTIAL] < 1000.0
    assert np.all(rel <= 1e-4), (rel, d, ref)


@pytest.mark.parametrize("bidirectional", [False, True])
def test_frame_distance_rig_against_host_composed_view_poses(bidirectional):
    """`vipe_frame_distance_rig` on a two-view rig at the (41, 73) grid against the plain oracle `frame_distance` run on
    per-view poses R_v^-1 G_n composed on the host (oracle/se3.py, float64): same- and cross-view pairs, 1e-4 per pair."""
    from vipe_amd.ext import slam_ext
    r = fc.rig_case(41, 73)
    ref, _ = fc.rig_reference(r, bidirectional)
    d = slam_ext.frame_distance_rig(T(r.poses), T(r.rig), T(r.disps), T(r.intr_full), T(fc.RIG_PI), T(fc.RIG_QI),
                                    T(fc.RIG_PJ), T(fc.RIG_QJ), fc.BETA, bidirectional=bidirectional).cpu().numpy()
    rel = np.abs(d - ref) / np.abs(ref)
    print("frame_distance_rig", bidirectional, "rel err per pair", rel)
    assert np.all(rel <= 1e-4), (rel, d, ref)


@pytest.mark.parametrize("grid", fc.GRIDS)
def test_depth_filter_permuted_subset_with_its_own_thresholds(grid):
    """Counts equal to the float32 oracle's for frames [5, 0, 7, 2] (output slot != frame, first and last frame: some of
    the six neighbours do not exist) with one threshold per entry; only pixels whose float64 margin to the threshold is
    below 1e-4 of it are left out, at most 0.5 % of them."""
    from vipe_amd.ext import slam_ext
    c = fc.geom_case(*grid)
    args = (c.g.poses, c.disps, c.intr, fc.DF_INDS, c.df_thresh)
    ref = frame_ops.depth_filter(*args)
    _, margin = frame_ops.depth_filter(*args, dtype=np.float64, with_margin=True)
    cnt = slam_ext.depth_filter(*(T(a) for a in args)).cpu().numpy()
    left_out = margin < 1e-4 * c.df_thresh[:, None, None]
    print("depth_filter", grid, "left out", int(left_out.sum()), "differ", int((cnt != ref).sum()))
    assert cnt.shape == ref.shape == (len(fc.DF_INDS), c.ht, c.wd)
    assert left_out.mean() <= CAP
    assert np.array_equal(cnt[~left_out], ref[~left_out])
    assert ref.max() >= 3 and ref.min() == 0 and cnt.max() <= 6


@pytest.mark.parametrize("grid", fc.GRIDS)
def test_projmap_and_iproj_beyond_one_workgroup(grid):
    """Tolerance = 4 x the float32 oracle's own distance from the float64 one on these inputs (division and square-root
    rounding is all that separates the kernel from numpy's float32), never above the 2e-3 px / 1e-3 the suite already
    holds them to; `valid` equal.  Pixels whose float64 depth is within 1e-5 of a branch point are left out."""
    from vipe_amd.ext import slam_ext
    c = fc.geom_case(*grid)
    args = (c.pm_poses, c.disps, c.intr, fc.PM_II, fc.PM_JJ)
    rc, rv = frame_ops.projmap(*args)
    rc64, rv64, depth = frame_ops.projmap(*args, dtype=np.float64, with_depth=True)
    assert (depth < 0.01).any() and ((depth > 0.01) & (depth < 0.25)).any()  # both branches below MIN_DEPTH occur
    coords, valid = (t.cpu().numpy() for t in slam_ext.projmap(*(T(a) for a in args)))
    keep_v = np.abs(depth - 0.25) >= 1e-5
    keep_c = np.abs(depth - 0.01) >= 1e-5
    assert (~keep_v).mean() <= CAP and (~keep_c).mean() <= CAP
    tol = min(4 * np.abs(rc - rc64)[keep_c].max(), 2e-3)
    err = np.abs(coords - rc)[keep_c].max()
    print("projmap", grid, "err", err, "tol", tol)
    assert tol > 0 and err <= tol
    assert np.array_equal(valid[..., 0][keep_v], rv[..., 0][keep_v]) and np.array_equal(rv[..., 0][keep_v], rv64[..., 0][keep_v])
    assert 0 < valid.mean() < 1
    rp, rp64 = (frame_ops.iproj(c.g.poses, c.disps, c.intr, dtype=t) for t in (np.float32, np.float64))
    pts = slam_ext.iproj(T(c.g.poses), T(c.disps), T(c.intr)).cpu().numpy()
    tol = min(4 * np.abs(rp - rp64).max(), 1e-3)
    err = np.abs(pts - rp).max()
    print("iproj", grid, "err", err, "tol", tol)
    assert tol > 0 and err <= tol


def test_frame_ops_bits_unchanged():
    """tests/golden/geom_parent_bits.npz holds what the eight frame geometry operations computed on the device before the
    pinhole and the sphere kernels became two instantiations of one pixel walk (tests/golden/make_golden_geom_parent.py:
    the inputs of this file and of tests/test_gpu_panorama.py, plus one per family at exactly 75 % valid pixels, where the
    pinhole family answers 1000 and the sphere the mean).  No atomics, fixed-order reductions: the same bits, every array."""
    import os
    import sys
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sys.path.insert(0, gold)
    import make_golden_geom_parent as mk
    Z = np.load(os.path.join(gold, "geom_parent_bits.npz"))
    got = mk.run_case()
    assert sorted(got) == sorted(Z.files)
    differ = [k for k in Z.files if not np.array_equal(got[k].view(np.uint32), Z[k].view(np.uint32))]
    print("frame ops:", len(Z.files), "arrays,", "all equal" if not differ else f"DIFFERENT: {differ}")
    assert not differ
    assert Z["pinhole_quarter_invalid"][0] == 1000.0 and 0.0 < Z["panorama_quarter_invalid"][0] < 1000.0


# ------------------------------------------------------------------------------------------------ scatter

SLOTS = 37


@functools.lru_cache(maxsize=None)
def _stride_case():
    """[2, 4099, 257] float32 = 2 106 886 elements: 9 734 more than the 8192 x 256 lanes of the largest launch, so the
    grid-stride loop takes a second trip; odd inner size.  The float64 host references are computed once."""
    gen = torch.Generator().manual_seed(41)
    src = torch.randn(2, 4099, 257, generator=gen)
    index = {"rows": torch.randint(0, SLOTS, (4099,), generator=gen), "full": torch.randint(0, SLOTS, (2, 4099, 257), generator=gen)}
    assert src.numel() > 8192 * 256
    ref = {}
    for kind, idx in index.items():
        full = idx.view(1, -1, 1).expand(src.shape) if kind == "rows" else idx
        s64 = src.double()

        def reduce(values, how, init):
            return torch.full((2, SLOTS, 257), init, dtype=torch.float64).scatter_reduce(1, full, values, how, include_self=how == "sum")
        ref[kind] = {"sum": reduce(s64, "sum", 0.0), "min": reduce(s64, "amin", float("inf")), "max": reduce(s64, "amax", float("-inf")),
                     "abs": reduce(s64.abs(), "sum", 0.0), "rows": reduce(torch.ones_like(s64), "sum", 0.0)}
        assert bool((ref[kind]["rows"] > 0).all())  # every output is reached
    return src, index, ref


@pytest.mark.parametrize("kind", ["rows", "full"])
@pytest.mark.parametrize("red", ["sum", "min", "max"])
def test_scatter_grid_stride_second_trip(kind, red):
    """`scatter_kernel` with more elements than lanes, through `vipe_scatter_rows` ([E] index) and `vipe_scatter`
    (full-shape index): min / max exact, each sum within (rows in its slot) * 2^-24 * sum |x| of the float64 one."""
    from vipe_amd.ext import scatter
    src, index, ref = _stride_case()
    out = scatter.scatter(src.to(dev()), index[kind].to(dev()), dim=1, dim_size=SLOTS, reduce=red).cpu()
    assert out.shape == (2, SLOTS, 257) and out.dtype == torch.float32
    r = ref[kind]
    if red == "sum":
        err, bound = (out.double() - r["sum"]).abs(), r["rows"] * 2.0 ** -24 * r["abs"]
        print("scatter sum", kind, "worst err / bound", float((err / bound).max()))
        assert bool((err <= bound).all())
    else:
        assert torch.equal(out.double(), r[red])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_scatter_contention_on_one_slot(dtype):
    """4096 rows into slot 0 of three: every lane of the launch fights for the same three addresses.  mul over factors
    U(0.999, 1.001) within 2 * 4096 * eps of the extended-precision product; min / max exact on an all-negative and on a
    mixed source, `arg` names a row that attains the extreme, and is E in the slots nothing reached."""
    from vipe_amd.ext import scatter, scatter_ext
    E = 4096
    gen = torch.Generator().manual_seed(43)
    idx = torch.zeros(E, dtype=torch.int64, device=dev())
    fac = (0.999 + 0.002 * torch.rand(1, E, 3, generator=gen, dtype=torch.float64)).to(dtype)
    out = scatter.scatter(fac.to(dev()), idx, dim=1, dim_size=3, reduce="mul").cpu()
    want = np.prod(fac.numpy().astype(np.longdouble), axis=1)
    rel = np.abs(out[:, 0].numpy().astype(np.longdouble) - want) / want
    print("scatter mul", dtype, "rel err", rel, "bound", 2 * E * torch.finfo(dtype).eps)
    assert np.all(rel <= 2 * E * torch.finfo(dtype).eps)
    assert bool((out[:, 1:] == 1.0).all())
    mixed = torch.randn(1, E, 3, generator=gen, dtype=torch.float64).to(dtype)
    for name, src in (("negative", -mixed.abs() - 0.5), ("mixed", mixed)):
        for red, fn, want in (("min", scatter_ext.scatter_min, src.amin(1)), ("max", scatter_ext.scatter_max, src.amax(1))):
            val, arg = fn(src.to(dev()), idx, 1, None, 3)
            val, arg = val.cpu(), arg.cpu()
            assert torch.equal(val[:, 0], want), (name, red)
            assert bool((val[:, 1:] == 0).all()) and bool((arg[:, 1:] == E).all()), (name, red)
            assert arg.dtype == torch.int64 and bool(((arg[:, 0] >= 0) & (arg[:, 0] < E)).all()), (name, red)
            assert torch.equal(src.gather(1, arg[:, :1])[:, 0], want), (name, red)


@pytest.mark.parametrize("red", ["sum", "mean", "mul", "min", "max"])
def test_scatter_fp16_odd_inner_size_at_an_odd_offset(red):
    """The fp16 path does its compare-and-swap on the enclosing 32-bit word and picks a half of it: inner size 5 and an
    `out` that starts at element 3 of a larger half buffer put consecutive elements in alternating halves, and the first
    and the last of them in a word they share with a sentinel.  Against a float32 composition rounded to half: sum and
    mean 4e-3 (at most 4 values of |x| < 0.5 per slot: partial sums stay below 2, where a half rounding is <= 4.9e-4),
    min / max exact, mul within 2 half ulps per factor; no sentinel moves."""
    from vipe_amd.ext import scatter
    gen = torch.Generator().manual_seed(47)
    E, K, N, OFF, SENT = 19, 5, 7, 3, 77.0
    ix = torch.tensor([0, 5, 1, 1, 6, 3, 0, 5, 3, 6, 1, 0, 5, 3, 6, 0, 1, 5, 3])  # slots 2 and 4 stay empty; 4 rows at most
    counts = torch.bincount(ix, minlength=N)
    assert E == len(ix) and counts.max() == 4 and counts[2] == 0
    if red == "mul":
        src = (0.5 + torch.rand(E, K, generator=gen)).half()
    else:
        src = (torch.rand(E, K, generator=gen) - 0.5).half()
    init = {"sum": 0.0, "mean": 0.0, "mul": 1.0, "min": 60000.0, "max": -60000.0}[red]
    buf = torch.full((OFF + N * K + 6,), SENT, dtype=torch.float16, device=dev())
    out = buf[OFF:OFF + N * K].view(N, K)
    out.fill_(init)
    assert out.is_contiguous() and (out.data_ptr() - buf.data_ptr()) == 2 * OFF and out.data_ptr() % 4 == 2
    got = scatter.scatter(src.to(dev()), ix.to(dev()), dim=0, out=out, reduce=red)
    assert got.data_ptr() == out.data_ptr()
    full = ix.view(-1, 1).expand(E, K)
    how = {"sum": "sum", "mean": "sum", "mul": "prod", "min": "amin", "max": "amax"}[red]
    ref = torch.full((N, K), init).scatter_reduce(0, full, src.float(), how, include_self=True)
    if red == "mean":
        ref = ref / counts.clamp(min=1).view(-1, 1)
    ref = ref.half()
    res = buf.cpu()
    val = res[OFF:OFF + N * K].view(N, K)
    assert bool((res[:OFF] == SENT).all()) and bool((res[OFF + N * K:] == SENT).all()), red
    err = (val.float() - ref.float()).abs()
    print("scatter fp16", red, "max err", float(err.max()))
    if red in ("sum", "mean"):
        assert float(err.max()) <= 4e-3
    elif red == "mul":
        ulp = torch.from_numpy(np.spacing(ref.numpy()).astype(np.float32))
        assert bool((err <= 2 * counts.view(-1, 1) * ulp).all())
    else:
        assert torch.equal(val, ref)
    assert bool((val[2] == init).all()) and bool((val[4] == init).all())


# ------------------------------------------------------------------------------------------------ nearest neighbours


@pytest.mark.parametrize("M,N,knn", [(3001, 1024, 4), (3001, 1025, 4), (3001, 2048, 8), (300, 8, 8), (1, 2500, 4)])
def test_nearest_neighbours_at_the_tile_boundary(M, N, knn):
    """`test_nearest_neighbours_matches_brute_force`'s assertions with the tree at, one past and at twice the kernel's
    1024-point LDS tile, with a tree of exactly knn points, and with a single query."""
    from vipe_amd.ext import utils_ext
    g = torch.Generator().manual_seed(N * 10 + knn)
    q = torch.rand(M, 3, generator=g).to(dev())
    t = torch.rand(N, 3, generator=g).to(dev())
    dist, idx = utils_ext.nearest_neighbours(q, t, knn)
    assert dist.shape == (M, knn) and idx.shape == (M, knn) and idx.dtype == torch.int32
    d2 = torch.cdist(q.double(), t.double()) ** 2
    want_d, want_i = torch.topk(d2, knn, dim=1, largest=False)
    assert (dist.double() - want_d).abs().max().item() < 1e-6
    got_d = torch.gather(d2, 1, idx.long())
    assert (got_d - want_d).abs().max().item() < 1e-12  # the returned indices realise the k smallest distances
    assert bool((dist[:, 1:] >= dist[:, :-1]).all())
    if N == knn:
        assert sorted(idx[0].tolist()) == list(range(N))
    with pytest.raises(RuntimeError):
        utils_ext.nearest_neighbours(q, t[:2], 4)  # knn > N (knn.cu:32)
