"""The factor graph's integer bookkeeping (`vipe_amd.slam.edge_index.EdgeIndex`) and the host-side helpers of
`vipe_amd.slam.factor_graph`, on the CPU: nothing here launches a kernel."""

import types

import numpy as np
import pytest
import torch

from vipe_amd.slam import factor_graph as fg
from vipe_amd.slam.edge_index import NAMES, EdgeIndex


def _bare_graph():
    g = object.__new__(fg.FactorGraph)
    g.device = torch.device("cpu")
    g.ii, g.jj = torch.tensor([3, 4, 5]), torch.tensor([1, 2, 3])
    g.ii_inac = g.jj_inac = torch.zeros(0, dtype=torch.long)
    return g


def test_assigning_age_after_reading_the_host_arrays_keeps_the_edge_list():
    """What the reference's callers do (`graph.age = ...`): the other four arrays keep their values."""
    g = _bare_graph()
    g.host_edges()
    g.age = torch.tensor([7, 7, 7])
    h = g.host_edges()
    assert h["ii"].tolist() == [3, 4, 5] and h["jj"].tolist() == [1, 2, 3] and h["age"].tolist() == [7, 7, 7]
    assert h["ii_inac"].shape == (0,) and h["jj_inac"].shape == (0,)


@pytest.mark.parametrize("name,value", [("age", [7, 7, 7]), ("ii", [9, 8, 7]), ("ii", [9, 8]), ("ii_inac", [2, 2])])
def test_assigning_one_index_tensor_after_an_edit_keeps_the_other_arrays(name, value):
    """One attribute assigned directly after edits that made every device view stale, no attribute read in between:
    that array follows the tensor, the others are unchanged (`age` restarts when `ii` changes its length)."""
    g = _bare_graph()
    g._index.append(np.array([6]), np.array([4]))
    g._index.tick()
    g._index.remove(np.array([False, False, False, True]), store=True)
    want = {"ii": [3, 4, 5], "jj": [1, 2, 3], "age": [1, 1, 1], "ii_inac": [6], "jj_inac": [4]}
    setattr(g, name, torch.tensor(value))
    want[name] = value
    if name == "ii" and len(value) != 3:
        want["age"] = [0] * len(value)
    got = g.host_edges()
    assert {n: got[n].tolist() for n in NAMES} == want
    assert getattr(g, name).tolist() == value


class _NaiveIndex:
    """EdgeIndex restated with plain lists; the edge set is rebuilt from them every time."""

    def __init__(self):
        self.a = {n: [] for n in NAMES}

    def edges(self):
        a = self.a
        return set(zip(a["ii"], a["jj"])) | set(zip(a["ii_inac"], a["jj_inac"]))

    def absent(self, ii, jj):
        have = self.edges()
        return [(i, j) for i, j in zip(ii, jj) if (i, j) not in have]

    def append(self, ii, jj):
        self.a["ii"] += ii
        self.a["jj"] += jj
        self.a["age"] += [0] * len(ii)

    def remove(self, mask, store):
        a = self.a
        if store:
            a["ii_inac"] += [i for i, m in zip(a["ii"], mask) if m]
            a["jj_inac"] += [j for j, m in zip(a["jj"], mask) if m]
        for n in ("ii", "jj", "age"):
            a[n] = [x for x, m in zip(a[n], mask) if not m]

    def drop_keyframe(self, ix):
        a = self.a
        active = [i == ix or j == ix for i, j in zip(a["ii"], a["jj"])]
        inactive = [i == ix or j == ix for i, j in zip(a["ii_inac"], a["jj_inac"])]
        for n in ("ii_inac", "jj_inac"):
            a[n] = [x for x, m in zip(a[n], inactive) if not m]
        for n in ("ii", "jj", "ii_inac", "jj_inac"):
            a[n] = [x - (x >= ix) for x in a[n]]
        return active, inactive

    def tick(self):
        self.a["age"] = [x + 1 for x in self.a["age"]]


def test_edge_index_equals_a_naive_restatement_over_a_random_sequence():
    rng = np.random.default_rng(20261016)
    idx, ref = EdgeIndex(torch.device("cpu")), _NaiveIndex()
    seen = dict.fromkeys(NAMES)  # device tensors read so far, with the host values they were made from
    n_frames, counts = 6, dict.fromkeys(("append", "store", "drop", "keyframe", "tick", "filter"), 0)

    def compare(changed):
        for n in NAMES:
            assert idx.host[n].dtype == np.int64 and idx.host[n].tolist() == ref.a[n], n
        assert idx.edge_set() == ref.edges()
        for n in NAMES:
            if n not in changed and seen[n] is not None:
                assert idx.device(n) is seen[n], f"{n} was uploaded again although it did not change"
            if rng.random() < 0.3:
                seen[n] = idx.device(n)
                assert seen[n].dtype == torch.int64 and seen[n].tolist() == ref.a[n], n
            elif n in changed:
                seen[n] = None

    for _ in range(400):
        op = rng.choice(["append", "append", "store", "drop", "keyframe", "tick", "tick", "filter"])
        counts[op] += 1
        version, E = idx.version, len(ref.a["ii"])
        if op in ("append", "filter"):
            k = int(rng.integers(1, 9))
            ii, jj = rng.integers(0, n_frames, k), rng.integers(0, n_frames, k)  # may repeat an edge inside the batch
            new_i, new_j = idx.absent(ii, jj)
            new = ref.absent(ii.tolist(), jj.tolist())
            assert list(zip(new_i.tolist(), new_j.tolist())) == new
            changed = ()
            if op == "append" and new:
                idx.append(new_i, new_j)
                ref.append([e[0] for e in new], [e[1] for e in new])
                n_frames, changed = n_frames + int(rng.integers(0, 2)), ("ii", "jj", "age")
        elif op in ("store", "drop"):
            mask = rng.random(E) < 0.3
            idx.remove(mask, store=op == "store")
            ref.remove(mask.tolist(), op == "store")
            changed = ("ii", "jj", "age") + (("ii_inac", "jj_inac") if op == "store" else ())
        elif op == "keyframe":
            ix = int(rng.integers(0, n_frames))
            active, inactive = idx.drop_keyframe(ix)
            want = ref.drop_keyframe(ix)
            assert (active.tolist(), inactive.tolist()) == want
            compare(("ii", "jj", "ii_inac", "jj_inac"))
            idx.remove(active, store=False)  # as FactorGraph.rm_second_newest_keyframe does
            ref.remove(want[0], False)
            n_frames, changed = max(4, n_frames - 1), ("ii", "jj", "age", "ii_inac", "jj_inac")
        else:
            idx.tick()
            ref.tick()
            changed = ("age",)
        assert (idx.version > version) == bool(set(changed) - {"age"})
        compare(changed)
    assert min(counts.values()) >= 20 and len(ref.a["ii_inac"]) > 0


def test_update_batch_chunks_partition_the_groups_of_eight_source_frames():
    rng = np.random.default_rng(7)
    for _ in range(200):
        cnt = rng.integers(0, 40, int(rng.integers(1, 120))) * (rng.random() < 0.7)
        cnt = cnt * (rng.random(cnt.shape[0]) < 0.8)  # some frames are the source of no edge
        max_edges = int(rng.integers(8, 400))
        chunks = fg.chunk_groups(cnt, max_edges)
        size = {g0: int(cnt[g0:g0 + 8].sum()) for g0 in range(0, len(cnt), 8)}
        flat = [g0 for c in chunks for g0 in c]
        assert flat == [g0 for g0 in sorted(size) if size[g0] > 0]  # every non-empty group exactly once, in source order
        assert all(len(c) > 0 for c in chunks)
        for c in chunks:
            assert sum(size[g0] for g0 in c) <= max_edges or len(c) == 1
    assert fg.chunk_groups(np.zeros(0, dtype=np.int64), 8) == []


# `update_batch`'s budget arithmetic and residency rule on the 20-keyframe graph of the GPU parity test (E = 74), one
# pyramid = 696320 bytes on the 8 x 64 grid (blocked layout 8 x 64 sources, 2 x 4 rows, 2 x 32 columns, 4 levels, fp16).
# (V, volume GB, chunk edges, steps) -> (groups, max_edges, budget_rows, max_rows, policy, pyramids built over the passes):
# the budget arithmetic (volume bytes against the budget, max(8, ...), max(256, budget_rows // (8 V))) and the rule "keep a chunk
# while kept + its rows + the largest chunk's fit the budget" worked out for these inputs
BYTES_PER_PYRAMID = 512 * 512 * 2 * (1 + 1 / 4 + 1 / 16 + 1 / 64)
BACKEND_PLANS = [
    ((1, 160, 4096, 1), ([[0, 8, 16]], 4096, 246723, 74, "none", 74)),
    ((1, 160, 4096, 2), ([[0, 8, 16]], 4096, 246723, 74, "all", 74)),
    ((1, 160, 1, 2), ([[0], [8], [16]], 8, 246723, 32, "all", 74)),
    ((1, 0.04, 1, 2), ([[0], [8], [16]], 8, 61, 32, "some", 119)),
    ((1, 0.04, 4096, 2), ([[0, 8], [16]], 61, 61, 61, "some", 148)),
    ((1, 0.01, 4096, 2), ([[0], [8], [16]], 15, 15, 32, "some", 148)),
    ((1, 0.04, 1, 1), ([[0], [8], [16]], 8, 61, 32, "none", 74)),
    ((2, 160, 4096, 2), ([[0, 8, 16]], 4096, 246723, 148, "all", 148)),
    ((2, 0.04, 4096, 2), ([[0], [8], [16]], 30, 61, 64, "some", 296)),
    ((2, 0.01, 4096, 2), ([[0], [8], [16]], 8, 15, 64, "some", 296)),
]


def _backend_cnt():
    from vipe_amd.synth import make_graph
    ii = make_graph(n=20, height=64, width=512, radius=2, seed=53).ii
    assert len(ii) == 74
    return np.bincount(ii)


def _run_passes(plan, steps):
    """the pass loop of `update_batch` with dummy pyramids -> (pyramids built, kept_rows after every pass)"""
    res, built, kept = fg._PyramidResidency(plan), 0, []
    for _ in range(steps):
        for gi in range(len(plan.groups)):
            if res.get(gi) is None:
                vol = object()
                built += plan.rows[gi]
                res.offer(gi, vol)
                assert res.get(gi) in (None, vol)
        kept.append(res.kept_rows)
        assert res.kept_rows == sum(n for gi, n in enumerate(plan.rows) if res.get(gi) is not None)
    return built, kept


@pytest.mark.parametrize("args,want", BACKEND_PLANS, ids=[str(a) for a, _ in BACKEND_PLANS])
def test_backend_chunk_plan_and_pyramid_residency(args, want):
    (V, gb, chunk_edges, steps), (groups, max_edges, budget_rows, max_rows, policy, n_built) = args, want
    assert BYTES_PER_PYRAMID == 696320.0
    cnt = _backend_cnt()
    plan = fg.plan_backend_chunks(cnt, V, BYTES_PER_PYRAMID, steps, True, gb * 2**30, chunk_edges)
    assert (plan.groups, plan.max_edges, plan.budget_rows, plan.max_rows) == (groups, max_edges, budget_rows, max_rows)
    assert (plan.keep_all, plan.keep_some) == (policy == "all", policy == "some")
    size = {g0: int(cnt[g0:g0 + 8].sum()) for g0 in range(0, len(cnt), 8)}
    assert [g0 for c in plan.groups for g0 in c] == [g0 for g0 in sorted(size) if size[g0] > 0]
    assert plan.rows == [sum(size[g0] for g0 in c) * V for c in plan.groups] and plan.max_rows == max(plan.rows)
    assert all(n <= plan.max_edges * V or len(c) == 1 for c, n in zip(plan.groups, plan.rows))
    built, kept = _run_passes(plan, steps)
    assert built == n_built
    if policy == "all":
        assert kept == [74 * V] * steps
    elif policy == "none":
        assert kept == [0] * steps
    elif plan.max_rows > plan.budget_rows:
        # a single group of eight that alone exceeds the budget (the 0.01 GB rows, and two views at 0.04 GB) is still
        # worked on, and nothing stays resident next to it
        assert (gb, V) in ((0.01, 1), (0.04, 2), (0.01, 2)) and kept == [0] * steps
    else:  # what is kept leaves room for the largest chunk
        assert all(k + plan.max_rows <= plan.budget_rows for k in kept), kept
    assert kept == kept[:1] * steps and built == 74 * V * steps - kept[0] * (steps - 1)  # later passes rebuild what is not kept


def test_backend_chunk_plan_without_volumes_and_without_edges():
    cnt = _backend_cnt()
    plan = fg.plan_backend_chunks(cnt, 1, BYTES_PER_PYRAMID, 2, False, 0.04 * 2**30, 1)  # AltCorrBlock: nothing to keep
    assert (plan.keep_all, plan.keep_some) == (False, False)
    assert (plan.groups, plan.max_edges, plan.budget_rows, plan.rows) == ([[0], [8], [16]], 8, 61, [29, 32, 13])
    res = fg._PyramidResidency(plan)
    for gi in range(3):
        res.offer(gi, object())
    assert res.kept_rows == 0 and all(res.get(gi) is None for gi in range(3))
    empty = fg.plan_backend_chunks(np.zeros(0, dtype=np.int64), 1, BYTES_PER_PYRAMID, 2, True, 160 * 2**30, 4096)
    assert (empty.groups, empty.rows, empty.max_rows, empty.keep_all, empty.keep_some) == ([], [], 0, True, False)
    assert _run_passes(empty, 2) == (0, [0, 0])


def test_host_csr_groups_the_rows_by_source_node():
    rng = np.random.default_rng(3)
    dix = rng.integers(0, 7, 50)
    order, rowptr = fg.host_csr(dix, 9)
    assert order.dtype == np.int32 and rowptr.dtype == np.int32 and rowptr.shape == (10,) and rowptr[-1] == 50
    for s in range(9):
        assert order[rowptr[s]:rowptr[s + 1]].tolist() == np.flatnonzero(dix == s).tolist()


def test_per_view_rows_on_host_and_device_arrays():
    x = np.array([2, 0, 5])
    assert fg.per_view(x, 1) is x and fg.per_view(x, 3).tolist() == [6, 7, 8, 0, 1, 2, 15, 16, 17]
    t = torch.from_numpy(x)
    assert fg.per_view(t, 1) is t and fg.per_view(t, 3).tolist() == [6, 7, 8, 0, 1, 2, 15, 16, 17]


def test_host_tensors_never_reach_the_row_kernels():
    """The job structs carry raw addresses: a graph on host tensors raises instead of handing them to a kernel."""
    src, dst, idx = torch.zeros(4, 8), torch.zeros(4, 8), torch.tensor([0, 2])
    with pytest.raises(RuntimeError):
        fg.rows_gather([(src, dst, idx, 2, 32, 0)])
    stores = fg._EdgeStores(2, 2, torch.device("cpu"), with_pgate=False)
    with pytest.raises(RuntimeError):
        stores.append(torch.zeros(3, 128, 4).half(), torch.zeros(3, 128, 4).half(), torch.tensor([1]), None, 0)
    g = _bare_graph()
    g.buffer = types.SimpleNamespace(n_views=1)
    g.corr = g.net_n = g._stores = g._inac_cap = None
    g.target = g.weight = torch.zeros(1, 3, 2, 2, 2)
    g.target_inac = g.weight_inac = torch.zeros(1, 0, 2, 2, 2)
    with pytest.raises(RuntimeError):
        g.rm_factors(np.array([True, False, False]), store=True)
