"""The operator's tail with `heads0` split by consumer (vipe_update_weights.agg1_w / heads_dw_w): agg1 (128 -> 128) into
hbuf[..., 256:], the GraphAgg chain (segmented mean, agg2, eta) beside the heads, then delta0|weight0 (128 -> 256) into
hbuf[..., :256] and heads2.  The split is taken in the two-stream form only (`op_side_min_edges`, 1 here for the engines
that are to take it); on one stream the one 384-channel launch stays.

Every output element of hbuf, dw and eta is computed by the same kernel over the same 128-channel output slice in the
same K order as in the one 384-channel launch - the tile kernels and the gather kernels both cut the output channels
into independent 128-wide workgroup slices - so the split changes WHEN the chain runs and nothing it computes: all
comparisons here are bit for bit (`torch.equal`), on an aligned grid (4 x 64 tiles) and on the ragged 41 x 73 grid of
16:9 video (FLAT tiles)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _inputs(E, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    net = torch.randn(E, h, w, 128, generator=g).tanh().half().to(dev())
    xbuf = torch.zeros(E, h, w, 320, dtype=torch.float16, device=dev())
    xbuf[..., :128] = torch.randn(E, h, w, 128, generator=g).relu().half().to(dev())
    corr = torch.zeros(E, h, w, 200, dtype=torch.float16, device=dev())
    corr[..., :196] = (torch.randn(E, h, w, 196, generator=g) * 0.5).half().to(dev())
    motn = (torch.randn(E, h, w, 4, generator=g) * 3).half().to(dev())
    return net, xbuf, corr, motn


def _parent_tail(eng, net_out, ix, n_src):
    """The tail as it was sequenced before the split, issued by hand on buffers of its own: the 384-channel heads0,
    heads2, then segmented mean -> agg2 -> eta."""
    from vipe_amd._lib import check, lib, ptr, stream_ptr
    from vipe_amd.slam.update_engine import segment_csr

    E, H, W, _ = net_out.shape
    hbuf = torch.full((E, H, W, 384), -7.0, dtype=torch.float16, device=dev())
    dw = torch.full((E, H, W, 4), -7.0, dtype=torch.float32, device=dev())
    eng._conv(eng.heads0, net_out, 0, E, H, W, y=hbuf, act="relu")
    eng._conv(eng.heads2, hbuf, 0, E, H, W, mode="heads", fout=dw, cin=256)
    order, rowptr = segment_csr(ix, n_src)
    agg = torch.empty(n_src, H, W, 128, dtype=torch.float16, device=dev())
    a2 = torch.empty_like(agg)
    eta = torch.full((n_src, H, W), -7.0, dtype=torch.float32, device=dev())
    check(lib().vipe_segment_mean_nhwc_f16(ptr(hbuf), 384, 256, ptr(order), ptr(rowptr), ptr(agg), n_src, H * W, 128,
                                           stream_ptr(hbuf)), "segment_mean")
    eng._conv(eng.agg2, agg, 0, n_src, H, W, y=a2, act="relu")
    eng._conv(eng.eta, a2, 0, n_src, H, W, mode="eta", fout=eta)
    return hbuf, dw, eta


# (E, h, w, source slot of every edge): 5 edges on two 4 x 64 tiles per image; one edge on the ragged grid the
# reference's resize gives for 16:9 video (FLAT tiles: 12 of 256 positions, the last one partly beyond the image)
GRIDS = {"aligned_8x64": (5, 8, 64, [0, 0, 1, 2, 2]), "ragged_41x73": (1, 41, 73, [0])}


@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_split_tail_equals_the_one_launch_tail_bit_for_bit(grid, monkeypatch):
    from vipe_amd.slam.networks import UpdateModule
    from vipe_amd.slam.update_engine import UpdateEngine

    E, h, w, src = GRIDS[grid]
    ix = torch.tensor(src, device=dev())
    n_src = max(src) + 1
    torch.manual_seed(0)
    um = UpdateModule().eval()
    monkeypatch.delenv("VIPE_AMD_HEADS_BY_CONSUMER", raising=False)
    monkeypatch.setenv("VIPE_AMD_FUSED_HEADS", "0")  # the two-launch heads: the fused pair sums in another order
    eng = UpdateEngine(um, dev())
    assert not eng.fused_heads_on and not eng._wdesc.heads2_frag
    monkeypatch.setenv("VIPE_AMD_HEADS_BY_CONSUMER", "0")
    eng_one = UpdateEngine(um, dev())  # the same weights, heads0 as one launch (null agg1_w / heads_dw_w)
    assert eng.heads_by_consumer and not eng_one.heads_by_consumer
    assert eng._wdesc.agg1_w and eng._wdesc.heads_dw_w and not eng_one._wdesc.agg1_w and not eng_one._wdesc.heads_dw_w
    monkeypatch.delenv("VIPE_AMD_HEADS_BY_CONSUMER")
    eng_single = UpdateEngine(um, dev())  # split packed, but E below the two-stream threshold: the one launch
    eng.op_side_min_edges = eng_one.op_side_min_edges = 1
    assert eng_single.op_side_min_edges > E
    net, xbuf, corr, motn = _inputs(E, h, w, seed=11)
    pg = eng.gate_context(xbuf)
    outs = {}
    for name, e_, native in (("split/native", eng, True), ("split/python", eng, False), ("one/native", eng_one, True),
                             ("one/python", eng_one, False), ("single/native", eng_single, True),
                             ("single/python", eng_single, False)):
        e_._bufs["h"] = torch.full((E, h, w, 384), -3.0, dtype=torch.float16, device=dev())  # nothing left over from a run before
        n2, dw, eta, _ = e_.forward_nhwc(net, xbuf.clone(), corr, motn, ix=ix, n_src=n_src, pgate=pg, native=native)
        outs[name] = (n2.clone(), dw.clone(), eta.clone(), e_._bufs["h"].clone())
    # every run against the tail sequenced by hand in the old order from that run's own new state
    for name, (n2, dw, eta, hbuf) in outs.items():
        hbuf_p, dw_p, eta_p = _parent_tail(eng, n2, ix, n_src)
        assert torch.equal(hbuf[..., 256:], hbuf_p[..., 256:]) and torch.equal(hbuf[..., :256], hbuf_p[..., :256]), name
        assert torch.equal(dw, dw_p) and torch.equal(eta, eta_p), name
    # the runs among each other.  The pooled global context is an atomic sum over one workgroup per 256 pixels: two
    # terms per image on 8 x 64 (order-free), twelve on 41 x 73, where the new state itself may differ in its last bit
    # from run to run - there the comparison above, from each run's own state, is the whole statement
    if h * w <= 512:
        ref = outs["split/python"]
        for name, got in outs.items():
            for what, a, b in zip(("net", "dw", "eta", "hbuf"), got, ref):
                assert torch.equal(a, b), (name, what)


def test_fused_heads_native_equals_python_sequenced_and_leaves_the_rest_alone(monkeypatch):
    """With the fused heads on (the default on 4 x 64 tiles, in the two-stream form): the native and the Python-sequenced operator are
    bit-identical, hbuf[..., :256] is not written any more, and net', eta and hbuf[..., 256:] are those of the two-launch
    heads; dw agrees with theirs to the rounding (tests/test_gpu_fused_heads.py holds it to the reference)."""
    from vipe_amd.slam.networks import UpdateModule
    from vipe_amd.slam.update_engine import UpdateEngine

    E, h, w, src = GRIDS["aligned_8x64"]
    ix = torch.tensor(src, device=dev())
    torch.manual_seed(0)
    um = UpdateModule().eval()
    monkeypatch.delenv("VIPE_AMD_HEADS_BY_CONSUMER", raising=False)
    monkeypatch.delenv("VIPE_AMD_FUSED_HEADS", raising=False)
    eng = UpdateEngine(um, dev())
    assert eng.fused_heads_on and eng.fused_heads(h, w) and eng._wdesc.heads2_frag and not eng.fused_heads(41, 73)
    monkeypatch.setenv("VIPE_AMD_FUSED_HEADS", "0")
    eng_two = UpdateEngine(um, dev())
    monkeypatch.delenv("VIPE_AMD_FUSED_HEADS")  # the library reads the switch at every call
    assert not eng_two.fused_heads(h, w) and eng.fused_heads(h, w)
    net, xbuf, corr, motn = _inputs(E, h, w, seed=11)
    pg = eng.gate_context(xbuf)
    for side_from in (1, 64):  # two streams (agg1, chain || delta0|weight0 with the heads) / one: the two-launch heads
        eng.op_side_min_edges = eng_two.op_side_min_edges = side_from
        outs = {}
        for name, e_, native in (("fused/native", eng, True), ("fused/python", eng, False), ("two/native", eng_two, True)):
            e_._bufs["h"] = torch.full((E, h, w, 384), -3.0, dtype=torch.float16, device=dev())
            n2, dw, eta, _ = e_.forward_nhwc(net, xbuf.clone(), corr, motn, ix=ix, n_src=3, pgate=pg, native=native)
            outs[name] = (n2.clone(), dw.clone(), eta.clone(), e_._bufs["h"].clone())
        for a, b in zip(outs["fused/native"], outs["fused/python"]):
            assert torch.equal(a, b), side_from
        f, t = outs["fused/native"], outs["two/native"]
        if side_from > E:
            assert all(torch.equal(a, b) for a, b in zip(f, t))
            continue
        assert bool((f[3][..., :256] == -3.0).all()), side_from
        assert torch.equal(f[0], t[0]) and torch.equal(f[2], t[2]) and torch.equal(f[3][..., 256:], t[3][..., 256:]), side_from
        assert float((f[1] - t[1]).abs().max()) <= 4e-3  # oracle/conv_epilogues.py FP16_CAP on either against the reference


def test_split_tail_without_graph_agg_and_with_upmask():
    """ix None: no chain, agg1 still fills hbuf[..., 256:]; want_upmask reads the chain's a2 after the heads."""
    from vipe_amd.slam.networks import UpdateModule

    E, h, w = 2, 4, 64
    torch.manual_seed(0)
    eng = UpdateModule().eval().engine(dev())
    assert eng.heads_by_consumer
    net, xbuf, corr, motn = _inputs(E, h, w, seed=12)
    ix = torch.tensor([1, 0], device=dev())
    res = []
    for native in (True, False):
        n2, dw, eta, up = eng.forward_nhwc(net, xbuf.clone(), corr, motn, native=native)
        assert eta is None and up is None
        res.append((n2.clone(), dw.clone(), eng._bufs["h"].clone()))
        n2, dw, eta, up = eng.forward_nhwc(net, xbuf.clone(), corr, motn, ix=ix, n_src=2, want_upmask=True, native=native)
        res[-1] += (n2.clone(), dw.clone(), eta.clone(), up.clone())
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.equal(res[0][0], res[0][3]) and torch.equal(res[0][1], res[0][4])  # the chain does not touch net', dw
