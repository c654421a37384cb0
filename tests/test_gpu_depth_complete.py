"""`vipe_depth_anchor_bits` + `vipe_depth_complete` on the device against tests/depth_complete_reference.py: the neighbour
lists exactly (integers: no tolerance) at every target of every case, anchors bit for bit, every target inside the float32
bound of a branch it may take, fewer than 2 % of a case's targets undecided, the counters within the undecided count.
The seeded cases are `depth_complete_reference.CASES` (23 x 41 to 61 x 130, no multiples of the 64 x 4 tile, widths 63, 64,
65, 129 and 130 around the bit words, B <= 3, K in {1, 2, 5, 8}, R in {1, 3, 12, 64}, f16 and f32, both domains, wrap_x,
a mask, NaN / inf / 0 / negative values, a hole wider than 2R); every reference is computed once per module."""
import functools

import numpy as np
import pytest
import torch

import depth_complete_reference as dr
import test_gpu_frame_depth as fd

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def refs_of(name):
    return dr.case_refs(next(c for c in dr.CASES if c["name"] == name))


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(fd.dev())


def run(sparse, pred, mask, case, **kw):
    """-> (out, scale, shift, nbr, stats) as numpy, of one `ingest.depth_complete` call with everything asked for"""
    from vipe_amd.slam import ingest
    args = dict(K=case["K"], radius=case["R"], domain=case["domain"], mask=t(mask), wrap_x=bool(case.get("wrap")),
                want_fit=True, want_neighbours=True)
    args.update(kw)
    res = ingest.depth_complete(t(sparse), t(pred), **args)
    torch.cuda.synchronize()
    return tuple(None if r is None else r.cpu().numpy() for r in res)


def check(case, sparse, refs, out, scale, shift, nbr, stats):
    targets = undecided = 0
    want = np.zeros(4, dtype=np.int64)
    for b, ref in enumerate(refs):
        n, u = dr.check_image(ref, sparse[b], out[b], nbr[b], scale[b], shift[b])
        targets, undecided, want = targets + n, undecided + u, want + ref["stats"]
    print(f"{case['name']}: {targets} targets, {undecided} undecided, counters {stats.tolist()} against {want.tolist()}")
    assert int(stats.sum()) == targets, "every target counts exactly once"
    assert np.abs(stats - want).max() <= undecided, "the counters lie within the undecided count of the reference's"
    assert undecided <= dr.UNDECIDED_CAP * targets
    return targets


@pytest.mark.parametrize("name", [c["name"] for c in dr.CASES])
def test_seeded_cases(name):
    case = next(c for c in dr.CASES if c["name"] == name)
    sparse, pred, mask, refs = refs_of(name)
    assert check(case, sparse, refs, *run(sparse, pred, mask, case)) > 500


@pytest.mark.parametrize("name", ["37x63_k1_r3_disp", "45x129_k5_r64_f16_disp", "25x25_k5_r12_wrap_min", "35x65_k5_r3_mask_poison"])
def test_invariance_batch_split_repeat_and_dirty_buffers(name):
    from vipe_amd.slam import ingest
    case = next(c for c in dr.CASES if c["name"] == name)
    sparse, pred, mask, _ = refs_of(name)
    whole = run(sparse, pred, mask, case)
    again = run(sparse, pred, mask, case)
    bits = lambda a: a.view(np.uint16 if a.dtype == np.float16 else np.uint32 if a.dtype == np.float32 else a.dtype)
    for a, b in zip(whole, again):
        assert np.array_equal(bits(a), bits(b)), "the same call twice"
    stats = np.zeros(4, dtype=np.int64)
    for b in range(case["B"]):
        one = run(sparse[b:b + 1], pred[b:b + 1], None if mask is None else mask[b:b + 1], case)
        for a, o in zip(whole[:4], one[:4]):
            assert np.array_equal(bits(a[b]), bits(o[0])), f"image {b} alone"
        stats += one[4]
    assert np.array_equal(stats, whole[4])
    # a dirty output buffer, and counters that are added to
    dirty = torch.full(sparse.shape, float("nan"), dtype=t(sparse).dtype, device=fd.dev())
    st = torch.tensor([5, 6, 7, 8], dtype=torch.int64, device=fd.dev())
    res = ingest.depth_complete(t(sparse), t(pred), K=case["K"], radius=case["R"], domain=case["domain"], mask=t(mask),
                                wrap_x=bool(case.get("wrap")), out=dirty, stats=st)
    assert res[0] is dirty and res[1] is None and res[2] is None and res[3] is None and res[4] is st
    assert np.array_equal(bits(dirty.cpu().numpy()), bits(whole[0]))
    assert np.array_equal(st.cpu().numpy() - np.array([5, 6, 7, 8]), whole[4])


def edge(sparse, pred, K=5, R=12, domain="disp", wrap=False, mask=None):
    case = dict(name="edge", K=K, R=R, domain=domain, wrap=wrap)
    sparse, pred = sparse[None], pred[None]
    ref = dr.complete_ref(sparse[0], pred[0], K, R, domain, mask, wrap)
    res = run(sparse, pred, None if mask is None else mask[None], case)
    check(case, sparse, [ref], *res)
    return ref, res


def test_no_anchor_every_anchor_one_anchor():
    rng = np.random.default_rng(3)
    pred = rng.uniform(0.5, 2.0, (23, 41)).astype(np.float32)
    ref, (out, scale, shift, nbr, stats) = edge(np.zeros_like(pred), pred)
    assert stats.tolist() == [0, 0, 23 * 41, 0] and not out.any() and (nbr == -1).all(), "no anchor: every target unreached"
    full = rng.uniform(0.5, 2.0, (23, 41)).astype(np.float32)
    ref, (out, scale, shift, nbr, stats) = edge(full, pred)
    assert stats.tolist() == [0, 0, 0, 0] and np.array_equal(out[0], full) and (scale == 1).all() and (shift == 0).all()
    one = np.zeros_like(pred)
    one[11, 20] = 1.25
    ref, (out, scale, shift, nbr, stats) = edge(one, pred, R=12)
    n_disc = sum(1 for y in range(23) for x in range(41) if 0 < (y - 11) ** 2 + (x - 20) ** 2 <= 144)
    assert stats.tolist() == [0, n_disc, 23 * 41 - 1 - n_disc, 0], "one neighbour: scale only inside the disc, unreached outside"
    assert out[0, 11, 20] == np.float32(1.25) and (nbr[0, 11, 8] == [11 * 41 + 20, -1, -1, -1, -1]).all() and (nbr[0, 11, 7] == -1).all()


def test_borders_corners_and_fewer_than_k():
    """anchors only in the middle: the four corners and all four borders are targets with partly empty windows, and R = 64
    reaches across the whole image; three anchors with K = 8: short lists"""
    rng = np.random.default_rng(4)
    H, W = 33, 67
    pred = rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
    sparse = np.zeros_like(pred)
    sparse[14:19, 30:37] = rng.uniform(0.5, 2.0, (5, 7))
    ref, (out, _, _, nbr, stats) = edge(sparse, pred, K=5, R=64, domain="depth")
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 33), (H - 1, 33), (16, 0), (16, W - 1)):
        assert out[0, y, x] > 0 and (nbr[0, y, x] >= 0).all()
    three = np.zeros_like(pred)
    three[3, 3], three[20, 40], three[32, 66] = 1.0, 1.5, 0.75
    ref, (out, _, _, nbr, stats) = edge(three, pred, K=8, R=64)
    assert ((nbr[0] >= 0).sum(-1).max() == 3) and stats[2] == 0


def test_wrap_reaches_across_the_seam():
    rng = np.random.default_rng(5)
    H, W = 9, 70
    pred = rng.uniform(0.5, 2.0, (H, W)).astype(np.float32)
    sparse = np.zeros_like(pred)
    sparse[:, 66:] = rng.uniform(0.5, 2.0, (H, 4))  # anchors in the last four columns only
    _, (out_w, _, _, nbr_w, stats_w) = edge(sparse, pred, K=3, R=8, wrap=True)
    _, (out_n, _, _, nbr_n, stats_n) = edge(sparse, pred, K=3, R=8, wrap=False)
    assert (out_w[0, :, :4] > 0).all() and not out_n[0, :, :4].any(), "columns 0..3 see the anchors only round the seam"
    assert (nbr_w[0, 4, 0, 0] == 4 * W + 69) and stats_n[2] > stats_w[2]


def test_composition_with_nearest_neighbours_on_the_device():
    """without wrap_x and with R = 64 not binding (the image's diagonal is shorter), the lists are those of `nonzero` +
    `utils_ext.nearest_neighbours`, whose tie rule is the lower tree index: row-major order"""
    from vipe_amd.ext import utils_ext
    case = dict(K=5, R=64, domain="depth")
    sparse, pred = dr.make_case(77, 23, 41, 0.2)
    assert 22 ** 2 + 40 ** 2 < 64 ** 2
    nbr = run(sparse[None], pred[None], None, case)[3][0]
    anchor, target = dr.classify(sparse, pred)
    tree = torch.nonzero(t(anchor)).float().contiguous()
    query = torch.nonzero(t(target)).float().contiguous()
    _, idx = utils_ext.nearest_neighbours(query, tree, 5)
    pix = (tree[:, 0] * 41 + tree[:, 1]).long()[idx.long()].cpu().numpy()
    assert np.array_equal(nbr[target], pix)


def test_ext_knn_scale_shift():
    """the ext entry point with `kss_completer`'s arguments, against the float64 rule (the reference's own fixture could
    not be made: see tests/test_depth_complete_reference.py)"""
    from vipe_amd.ext import depth_complete_ext
    rng = np.random.default_rng(9)
    maps = [dr.make_case(900 + b, 61, 97, 0.02, domain="disp") for b in range(2)]
    sparse, pred = np.stack([m[0] for m in maps]), np.stack([m[1] for m in maps])
    sparse_masks = sparse > 0
    complete_masks = ~sparse_masks & (rng.random(sparse.shape) < 0.9)
    junk = np.where(sparse_masks, sparse, np.float32(7.0))  # what lies outside sparse_masks must not count
    out, scale, shift = depth_complete_ext.knn_scale_shift(t(junk), t(pred), t(sparse_masks), t(complete_masks), K=5, radius=64)
    torch.cuda.synchronize()
    for b in range(2):
        ref = dr.complete_ref(sparse[b], pred[b], 5, 64, "disp", complete_masks[b].astype(np.uint8))
        n, u = dr.check_image(ref, sparse[b], out[b].cpu().numpy(), None, scale[b].cpu().numpy(), shift[b].cpu().numpy())
        assert n > 4000 and u <= dr.UNDECIDED_CAP * n
        assert not out[b].cpu().numpy()[~sparse_masks[b] & ~complete_masks[b]].any()


def test_wrapper_argument_checks():
    from vipe_amd.ext import depth_complete_ext
    from vipe_amd.slam import ingest
    dev = fd.dev()
    s, p = torch.zeros(2, 9, 30, device=dev), torch.ones(2, 9, 30, device=dev)
    out, scale, shift, nbr, stats = ingest.depth_complete(s[:0], p[:0], want_fit=True, want_neighbours=True)
    assert tuple(out.shape) == (0, 9, 30) and tuple(nbr.shape) == (0, 9, 30, 5) and stats.tolist() == [0, 0, 0, 0], "B == 0"
    for bad in (dict(K=0), dict(K=9), dict(radius=0), dict(radius=65), dict(domain="range"), dict(wrap_x=True, radius=15),
                dict(mask=torch.ones(2, 9, 30, device=dev)), dict(mask=torch.ones(2, 9, 31, dtype=torch.bool, device=dev)),
                dict(out=torch.zeros(2, 9, 30, dtype=torch.float16, device=dev)), dict(out=torch.zeros(1, 9, 30, device=dev)),
                dict(stats=torch.zeros(3, dtype=torch.int64, device=dev)), dict(stats=torch.zeros(4, dtype=torch.int32, device=dev))):
        with pytest.raises(RuntimeError):
            ingest.depth_complete(s, p, **bad)
    for a, b in ((s, p.half()), (s, p[:1]), (s[0], p[0]), (s.double(), p.double()), (s.transpose(1, 2), p.transpose(1, 2))):
        with pytest.raises(RuntimeError):
            ingest.depth_complete(a, b)
    assert ingest.depth_complete(s, p, wrap_x=True, radius=14)[4].tolist() == [0, 0, 2 * 9 * 30, 0]
    m = torch.ones(2, 9, 30, dtype=torch.bool, device=dev)
    for args in ((s.half(), p.half(), m, m), (s, p[:1], m, m), (s, p, m.to(torch.uint8), m), (s, p, m, m[:1])):
        with pytest.raises(RuntimeError):
            depth_complete_ext.knn_scale_shift(*args)
    # the bit buffer is kept and reused
    before = ingest._anchor_bits(1, dev).data_ptr()
    ingest.depth_complete(s, p)
    assert ingest._anchor_bits(1, dev).data_ptr() == before
