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
