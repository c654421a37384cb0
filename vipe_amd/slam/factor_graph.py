"""Factor graph: edge lists + the update iteration (host-side mirror of vipe/slam/components/factor_graph.py).

`update()` is the hot loop A of SURVEY.md section 3.3 (factor_graph.py:231-314): reproject -> 4-level
correlation lookup -> flow-update operator -> dense BA.  Per iteration it issues 2 + (GRU convolutions) +
1 C-ABI calls on the current stream and never synchronises the host (the reference syncs in torch.unique,
scatter_mean's index.max(), every _tmult_mat_elements and the CPU spsolve).
"""

import ctypes
import dataclasses
import os

import numpy as np
import torch

from .._lib import check, check_gpu_contig, lib, parse_struct, require, stream_ptr, upload, upload_many
from ..ext import slam_ext
from .edge_index import NAMES, EdgeIndex, as_host
from .networks import AltCorrBlock, CorrBlock, CorrPool

# host-side work counters (edge counts known without touching the device): edges x operator applications, correlation
# pyramids built - what bench.py prices a whole clip's algorithmic bytes / FLOPs with (SURVEY 8d per-edge figures)
WORK = {"edge_updates": 0, "pyramids_built": 0}
BACKEND_VOLUME_GB = 160  # default of VIPE_AMD_BACKEND_VOLUME_GB: correlation pyramids `update_batch` keeps, of 288 GB


def warm_volume_pool(device, gigabytes=None):
    """Map the memory the first global BA of this process will ask for (`update_batch` keeps up to
    VIPE_AMD_BACKEND_VOLUME_GB of correlation pyramids) into torch's caching allocator NOW: a fresh process pays the
    driver ~0.9 s for the first 100 GB it maps (measured: the same 200-keyframe clip runs its two backend passes in
    1.7 s in a process that has held the memory before, 2.6 s in one that has not).  A long-lived worker that processes
    clip after clip is warm after its first clip; a benchmark's untimed warm-up should leave the process in that state."""
    if torch.device(device).type != "cuda":
        return 0
    want = float(gigabytes if gigabytes is not None else os.environ.get("VIPE_AMD_BACKEND_VOLUME_GB", BACKEND_VOLUME_GB)) * 2**30
    free, _ = torch.cuda.mem_get_info(device)
    n = int(min(want, 0.85 * free))
    if n <= 0:
        return 0
    x = torch.empty(n, dtype=torch.uint8, device=device)
    x[::1 << 21].zero_()  # touch every 2 MiB page
    del x
    return n


RowsJob = parse_struct("vipe_rows_job")   # include/vipe_amd.h
NhwcJob = parse_struct("vipe_nhwc_job")


def per_view(x, V):
    """edge indices `x` (numpy array or tensor) -> the rows of their V per-view terms: x * V + [0, V)"""
    if V == 1:
        return x
    views = torch.arange(V, device=x.device) if torch.is_tensor(x) else np.arange(V)
    return (x[:, None] * V + views).reshape(-1)


def host_csr(dix, n_src):
    """`update_engine.segment_csr` on the host (torch.bincount reads its maximum back: a stream drain): the rows grouped
    by source node `dix` [n] -> int32 (order [n], rowptr [n_src + 1])"""
    order = np.argsort(dix, kind="stable").astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(dix, minlength=n_src))]).astype(np.int32)
    return order, rowptr


def chunk_groups(cnt, max_edges):
    """`update_batch`'s chunks, cnt[f] = edges with source frame f.  The reference walks the source keyframes in groups of
    8 (factor_graph.py:337-343) to bound memory.  The operator couples edges only through GraphAgg's per-source-frame
    mean, so ANY partition that keeps every source frame's edges together gives the same result: the non-empty groups are
    merged, in order, while a chunk stays within `max_edges` edges (a single group may exceed it).
    -> [[first frame of each group of the chunk], ...]"""
    groups, size = [], 0
    for g0 in range(0, len(cnt), 8):
        n8 = int(cnt[g0:g0 + 8].sum())
        if n8 == 0:
            continue
        if not groups or size + n8 > max_edges:
            groups.append([])
            size = 0
        groups[-1].append(g0)
        size += n8
    return groups


BackendChunkPlan = dataclasses.make_dataclass("BackendChunkPlan", frozen=True, fields=[
    ("groups", list), ("rows", list), ("max_rows", int), ("max_edges", int), ("budget_rows", int), ("keep_all", bool), ("keep_some", bool)])
# what `FactorGraph._backend_chunk` prepares once per chunk
_BackendChunk = dataclasses.make_dataclass("_BackendChunk", ["idx_x", "edges", "du", "dixs", "csr", "mask", "xb", "pgate"])


def plan_backend_chunks(cnt, n_views, bytes_per_pyramid, steps, use_volume, budget_bytes, chunk_edges):
    """`update_batch`'s chunks, cnt[f] = edges with source frame f.  With 288 GB of HBM the reference's groups of 8 source
    keyframes are merged until a chunk holds `chunk_edges` edges (4096: ~110 GB of pyramids at 48 x 64, normally one chunk)
    or fills the budget, whatever the grid: a pyramid takes 33 MB at 48 x 64, 238 MB at 64 x 128.  -> groups (`chunk_groups`
    up to max_edges), rows (per chunk its correlation pyramids, one per edge and view; max_rows: the largest chunk's),
    budget_rows (pyramids the budget holds), keep_all (every chunk's pyramids stay resident over the passes: the feature maps
    do not change), keep_some (they do not fit - ~4800 edges at 48 x 64, 300+ keyframes: `_PyramidResidency` keeps as MANY as fit)"""
    keep_all = bool(use_volume and steps > 1 and int(cnt.sum()) * n_views * bytes_per_pyramid <= budget_bytes)
    keep_some = bool(use_volume and steps > 1 and not keep_all)
    budget_rows = int(budget_bytes / bytes_per_pyramid)
    max_edges = max(8, min(chunk_edges, budget_rows // n_views))
    if keep_some:  # finer chunks: one eighth of the budget each, so that seven of eight budget shares can stay resident
        max_edges = max(8, min(max_edges, max(256, budget_rows // (8 * n_views))))
    groups = chunk_groups(cnt, max_edges)
    rows = [int(sum(cnt[g0:g0 + 8].sum() for g0 in grp)) * n_views for grp in groups]
    return BackendChunkPlan(groups, rows, max(rows, default=0), max_edges, budget_rows, keep_all, keep_some)


class _PyramidResidency:
    """The pyramids (opaque here) kept over the passes of one `update_batch`, `get(chunk)`: every chunk's, or those offered
    while they and the largest chunk still fit the budget together; the others are rebuilt every pass (8.5 us per edge)."""

    def __init__(self, plan):
        self.plan, self._vols, self.kept_rows = plan, {}, 0
        self.get = self._vols.get

    def offer(self, gi, vol):
        p, n = self.plan, self.plan.rows[gi]
        if p.keep_all or (p.keep_some and self.kept_rows + n + p.max_rows <= p.budget_rows):
            self._vols[gi] = vol
            self.kept_rows += n


def rows_gather(jobs):
    """ONE launch of `vipe_rows_gather`: per job (src, dst, idx, n_rows, row_bytes, dst_row0[, seg]) the rows idx[r] of `src`
    go to the rows dst_row0 + r of `dst` - whole, or with seg = (seg_bytes, seg_pitch, n_seg) that slice per pixel only"""
    arr = (RowsJob * len(jobs))()
    for j, job in zip(arr, jobs):
        src, dst, idx, n_rows, row_bytes, dst_row0, seg = (*job, None)[:7]
        check_gpu_contig(src, dst, idx)  # their addresses go to the kernel as they are
        require(idx.dtype == torch.int64, "row indices must be int64")
        j.src, j.dst, j.idx = src.data_ptr(), dst.data_ptr(), idx.data_ptr()
        j.src_row_pitch = j.dst_row_pitch = row_bytes
        j.seg_bytes, j.seg_pitch, j.n_seg = seg or (row_bytes, row_bytes, 1)
        j.n_rows, j.dst_row0 = int(n_rows), int(dst_row0)
    if jobs:
        check(lib().vipe_rows_gather(ctypes.addressof(arr), len(jobs), stream_ptr(jobs[0][2])), "rows_gather")


class _EdgeStores:
    """The big per-edge tensors of an incremental graph - hidden state `net` [n,h,w,128], operator input `xbuf`
    [n,h,w,320] (context features in channels [0,128), the rest scratch), hoisted gate context `pgate` [n,h,w,384] - in
    backing buffers with spare capacity, two banks each.  The reference concatenates (copies the whole tensor) on every
    `add_factors` and compacts with boolean masks on every `rm_factors` (factor_graph.py:160-170, 190-201: 4.4 MB per
    edge); here `append` is ONE launch that reads the new edges' source frames from the keyframe buffer and writes them
    channels-last behind the live rows (`vipe_gather_nchw_to_nhwc_f16`), and `compact` is ONE launch that moves the
    surviving rows of all tensors (and whatever small per-edge arrays the caller adds) into the other bank
    (`vipe_rows_gather`).  The operator ping-pongs `net` between its two banks (`net_spare`)."""

    def __init__(self, ht, wd, device, with_pgate):
        self.ht, self.wd, self.device, self.with_pgate = ht, wd, device, with_pgate
        self.cap = 0
        self.net, self.xb, self.pg = [None, None], [None, None], [None, None]
        self.cur = 0  # bank of xbuf / pgate

    def _alloc(self, cap):
        f16 = dict(dtype=torch.float16, device=self.device)
        shp = (cap, self.ht, self.wd)
        return ([torch.empty(shp + (128,), **f16) for _ in range(2)], [torch.empty(shp + (320,), **f16) for _ in range(2)],
                [torch.empty(shp + (384,), **f16) if self.with_pgate else None for _ in range(2)])

    def bank_of(self, net_n):
        """which net bank `net_n` is a view of (None: a tensor from outside)"""
        if net_n is not None and self.net[0] is not None:
            for k in (0, 1):
                if net_n.data_ptr() == self.net[k].data_ptr():
                    return k
        return None

    def reserve(self, rows, net_n, n_live):
        """room for `rows` rows; -> net_n (re-homed when the stores grew or `net_n` came from outside)"""
        grow = rows > self.cap
        if grow:
            cap = max(rows + rows // 4, 64)  # 25 % spare: the frontend's window oscillates by a few edges
            net, xb, pg = self._alloc(cap)
            if n_live and self.cap:
                xb[0][:n_live, ..., :128] = self.xb[self.cur][:n_live, ..., :128]
                if self.with_pgate:
                    pg[0][:n_live] = self.pg[self.cur][:n_live]
            old = net_n
            self.net, self.xb, self.pg, self.cur, self.cap = net, xb, pg, 0, cap
            if n_live and old is not None:
                self.net[0][:n_live] = old
                return self.net[0][:n_live]
            return None
        if n_live and self.bank_of(net_n) is None:  # assigned from outside (tests restore a saved state): adopt it
            self.net[0][:n_live] = net_n
            return self.net[0][:n_live]
        return net_n

    def net_spare(self, net_n):
        k = self.bank_of(net_n)
        return None if k is None else self.net[1 - k][:net_n.shape[0]]

    def append(self, buffer_nets, buffer_inps, frames, net_n, n_live):
        """rows [n_live, n_live + k): hidden state and context features of the frames `frames` [k] int64 (device) of the
        keyframe buffer's flattened [N,128,h*w] maps -> (net_n, xbuf, new xbuf rows)"""
        k = int(frames.shape[0])
        if n_live == 0:
            net_n = None  # (a zero-row view has no address to recognise its bank by)
        net_n = self.reserve(n_live + k, net_n, n_live)
        nb = 0 if net_n is None else self.bank_of(net_n)
        P = self.ht * self.wd
        require(frames.dtype == torch.int64, "frame indices must be int64")
        jobs = (NhwcJob * 2)()
        for j, (src, dst, ctot) in enumerate(((buffer_nets, self.net[nb], 128), (buffer_inps, self.xb[self.cur], 320))):
            check_gpu_contig(src, frames, dst)  # their addresses go to the kernel as they are
            jobs[j].src, jobs[j].frame, jobs[j].dst = src.data_ptr(), frames.data_ptr(), dst.data_ptr()
            jobs[j].dst_row_pitch, jobs[j].dst_ctot, jobs[j].dst_coff, jobs[j].dst_row0 = P * ctot, ctot, 0, n_live
        check(lib().vipe_gather_nchw_to_nhwc_f16(ctypes.addressof(jobs), 2, k, 128, P, stream_ptr(frames)), "gather_nchw_to_nhwc")
        n = n_live + k
        return self.net[nb][:n], self.xb[self.cur][:n], self.xb[self.cur][n_live:n]

    def compact(self, keep, n_keep, net_n, extra_jobs=()):
        """rows `keep` [n_keep] int64 (device, ascending) of every store -> the other bank, in ONE launch together with
        `extra_jobs` (as `rows_gather` takes them) of small per-edge arrays; -> (net_n, xbuf, pgate)"""
        P = self.ht * self.wd
        nb = self.bank_of(net_n)
        jobs = []
        if n_keep:
            jobs.append((self.net[nb], self.net[1 - nb], keep, n_keep, P * 128 * 2, 0))
            jobs.append((self.xb[self.cur], self.xb[1 - self.cur], keep, n_keep, P * 320 * 2, 0, (256, 640, P)))  # context features only
            if self.with_pgate:
                jobs.append((self.pg[self.cur], self.pg[1 - self.cur], keep, n_keep, P * 384 * 2, 0))
        rows_gather(jobs + list(extra_jobs))
        self.cur ^= 1
        return (self.net[1 - nb][:n_keep], self.xb[self.cur][:n_keep], self.pg[self.cur][:n_keep] if self.with_pgate else None)


def _index_property(name):
    """One integer array of the edge bookkeeping as the device tensor the reference keeps (factor_graph.py:66-75): made
    from the host array (`EdgeIndex`, what this class works on) when somebody reads the attribute; an assignment from
    outside replaces that array."""
    def put(self, tensor):
        self._index.assign(name, tensor)
        if name != "age":
            self._edges_changed()

    return property(lambda self: self._index.device(name), put)


class FactorGraph:
    # Opt-in (not in the reference, which discards the operator's upsampling mask: factor_graph.py:269): after every BA
    # of `update` - and after the last one of `update_batch` - the disparities the BA has just produced are upsampled to
    # full resolution with THIS iteration's mask into `buffer.disps_up` (DROID-SLAM's order; `_upsample_disps`).  Needs
    # `GraphBuffer(upsample_disps=True)`.  Off: not one launch, allocation or argument differs.
    upsample = False
    # With `upsample`: None - every source row of the graph is upsampled (the keyframe graphs).  A flattened buffer row
    # (slot * V): only source rows from there on are, the rows before it are left as they are - pass 2's graph, whose
    # sources include keyframes whose `disps_up` rows are the global BA's result and must not be rewritten.
    upsample_from_row = None
    _last_ba = None  # t0, t1, damping and flags of the last BA `update` / `update_batch` issued (`marginals`' defaults)

    def __init__(self, update_module, buffer, device, max_factors=48, incremental=True, cross_view=False):
        self.update_op = update_module
        self.buffer = buffer
        self.device = device
        self.max_factors = max_factors
        self.incremental = incremental
        self.cross_view = cross_view and buffer.n_views > 1  # factor_graph.py:62
        ht, wd = buffer.height // 8, buffer.width // 8
        self.ht, self.wd = ht, wd
        self.damping = 1e-6 * torch.ones_like(buffer.flattened_disps)  # factor_graph.py:76
        self.target = torch.zeros([1, 0, ht, wd, 2], device=device, dtype=torch.float)
        self.weight = torch.zeros([1, 0, ht, wd, 2], device=device, dtype=torch.float)
        # channels-last state of the flow-update operator: hidden state [E,h,w,128] and [inp | corr | flow] features
        self.corr, self.net_n, self.xbuf = None, None, None
        self.pgate = None  # [E,h,w,384]: context-feature part of the GRU gates, computed once per edge
        self._stores = None  # _EdgeStores: backing buffers of net_n / xbuf / pgate (incremental graphs)
        # hidden-state part of the gates for the CURRENT net_n (UpdateEngine.hidden_gate_state), computed on a second
        # stream in the shadow of the previous iteration's BA; None whenever net_n / the edge set changed since
        self._gate_state = None
        self._side = None
        # tuning of that stage ("the BA's shadow"): taken from this many active edges on; released by
        # the BA per Gauss-Newton iteration ("gated") or launched at once ("free"); share of the edges whose z|r part is
        # staged; shares of the pieces
        self.gate_overlap_min_edges = int(os.environ.get("VIPE_AMD_GATE_OVERLAP_MIN_EDGES", "64"))
        self.gate_overlap_mode = "gated"
        self.gate_overlap_share = 0.5
        self.gate_overlap_fractions = [0.4, 0.4, 0.2]
        self.target_inac = torch.zeros([1, 0, ht, wd, 2], device=device, dtype=torch.float)
        self.weight_inac = torch.zeros([1, 0, ht, wd, 2], device=device, dtype=torch.float)
        self._plan = None
        self._plan_serial = 0   # counts rebuilt edge plans: (serial, kind) identifies the index arrays handed to the BA
        self._ba_state = {}     # private BA workspace + the key of the plan it holds (slam_ext.dense_ba)
        self._spare = None      # _net_spare's private ping-pong tensor
        self._inac_cap = None   # backing buffers of target_inac / weight_inac (_inactive_room)

    ii, jj, age, ii_inac, jj_inac = (_index_property(n) for n in NAMES)  # factor_graph.py:66-75

    @property
    def _index(self):
        """the EdgeIndex, made on first use: tests build bare graphs with `object.__new__` and assign attributes"""
        index = self.__dict__.get("_edge_index")
        if index is None:
            index = self.__dict__["_edge_index"] = EdgeIndex(self.device)
        return index

    def host_edges(self):
        """The integer edge bookkeeping {ii, jj, age, ii_inac, jj_inac} as the host keeps it (numpy int64, read-only):
        what every method of this class works on."""
        return dict(self._index.host)

    def _edges_changed(self):
        """the edge set changed: everything derived from it goes - the edge plan with its per-t0 entries, the staged gates"""
        self._plan = None
        self._gate_state = None

    @torch.no_grad()
    def add_factors(self, ii, jj, remove=False):
        """factor_graph.py:119-173."""
        ii_h, jj_h = self._index.absent(as_host(ii), as_host(jj))
        if ii_h.shape[0] == 0:
            return
        if (self.max_factors > 0 and self._index.host["ii"].shape[0] + ii_h.shape[0] > self.max_factors and self.corr is not None
                and remove):
            # factor_graph.py:136-139 (the reference's `arange[argsort(age)]` is the permutation itself; torch's sort
            # leaves the order of equal ages unspecified - the stable order is used here)
            ix = np.argsort(self._index.host["age"], kind="stable")
            self.rm_factors(ix >= self.max_factors - ii_h.shape[0], store=True)
        ii, jj = upload_many([ii_h, jj_h], self.device)
        pi, qi, _, pj, qj, _ = self.buffer.expand_edge_multiview(ii, jj)
        V = self.buffer.n_views
        n_live = 0 if self.net_n is None else int(self.net_n.shape[0])
        f1, f2 = (pi, pj) if V == 1 else (pi * V + qi, pj * V + qj)  # one view: frame index = pose index
        if self.incremental:
            if self.corr is None:
                self.corr = CorrPool(capacity=max(64, self.max_factors + 16))
            lo, hi = int(min(ii_h.min(), jj_h.min())), int(max(ii_h.max(), jj_h.max()))
            # a cross-view self edge (i, i) is re-targeted to cross_view_idx[i, v] by expand_edge_multiview - after an
            # adaptive cross-view pass that may be ANY keyframe of the buffer: the host (ii, jj) do not bound the frames
            rng = (0, self.buffer.n_frames * V) if (self.cross_view and V > 1) else (lo * V, (hi + 1) * V)
            self.corr.add_edges(self.buffer.flattened_fmaps, f1, f2, frame_range=rng)
            WORK["pyramids_built"] += int(pi.shape[0])
            eng = self.update_op.engine(self.device)
            if self._stores is None:
                self._stores = _EdgeStores(self.ht, self.wd, self.device, eng.supports_gate_split(self.ht, self.wd))
            # hidden state and context features of the new edges' source frames, straight from the keyframe buffer into
            # the stores' tails (one launch; the reference gathers, permutes and concatenates: factor_graph.py:147-170)
            self.net_n, self.xbuf, xb_new = self._stores.append(self.buffer.flattened_nets, self.buffer.flattened_inps,
                                                                f1.contiguous(), self.net_n, n_live)
            if self._stores.with_pgate:
                pg = self._stores.pg[self._stores.cur]
                eng.gate_context(xb_new, out=pg[n_live:n_live + xb_new.shape[0]])
                self.pgate = pg[:n_live + xb_new.shape[0]]
        else:
            net = self.buffer.nets[pi, qi].permute(0, 2, 3, 1).contiguous()
            self.net_n = net if self.net_n is None else torch.cat([self.net_n, net], 0)
        target, _ = self.buffer.reproject_dense_disp(ii, jj)
        target = target[None]
        self._index.append(ii_h, jj_h)
        self._edges_changed()
        self.target = torch.cat([self.target, target], 1)
        self.weight = torch.cat([self.weight, torch.zeros_like(target)], 1)

    @torch.no_grad()
    def rm_factors(self, mask, store=False):
        """factor_graph.py:175-202.  The mask is read ONCE (the callers of this package pass host arrays); the integer
        bookkeeping is edited on the host mirror, and the surviving rows of every per-edge tensor - hidden state, context
        features, gate context, targets, weights - and the rows that go to the inactive store move in ONE launch
        (`_EdgeStores.compact`; the reference indexes each tensor with the boolean mask, a sync per tensor)."""
        m = as_host(mask, bool)
        if not m.any():
            return
        self._index.remove(m, store)
        self._edges_changed()
        V = self.buffer.n_views
        keep_x_np, drop_x_np = per_view(np.flatnonzero(~m), V), per_view(np.flatnonzero(m), V)
        keep_x, drop_x = upload_many([keep_x_np, drop_x_np], self.device)
        nk, nd = int(keep_x_np.shape[0]), int(drop_x_np.shape[0])
        if self.corr is not None:
            self.corr = self.corr[keep_x_np]  # host-side index: the pool only edits its slot vector
        self._contiguous_targets()
        row = int(self.target.shape[2] * self.target.shape[3] * 2 * 4)  # one edge's [h, w, 2] f32
        new_t = torch.empty((1, nk) + tuple(self.target.shape[2:]), dtype=self.target.dtype, device=self.device)
        new_w = torch.empty_like(new_t)
        extra = [(self.target, new_t, keep_x, nk, row, 0), (self.weight, new_w, keep_x, nk, row, 0)] if nk else []
        if store and nd:
            ti, wi, n0 = self._inactive_room(nd)
            extra += [(self.target, ti, drop_x, nd, row, n0), (self.weight, wi, drop_x, nd, row, n0)]
        st = self._stores
        if st is not None and self.net_n is not None and st.bank_of(self.net_n) is None and self.net_n.shape[0]:
            self.net_n = st.reserve(self.net_n.shape[0], self.net_n, self.net_n.shape[0])  # assigned from outside: adopt
        if st is not None and self.net_n is not None and st.bank_of(self.net_n) is not None:
            self.net_n, self.xbuf, pg = st.compact(keep_x, nk, self.net_n, extra)
            if self.pgate is not None:
                self.pgate = pg
        else:  # non-incremental graphs (the backend's): no stores, the small arrays in one launch all the same
            if self.net_n is not None:
                self.net_n = self.net_n[keep_x]
            rows_gather(extra)
        self.target, self.weight = new_t, new_w

    def add_neighborhood_factors(self, t0, t1, r=3):
        """factor_graph.py:396-409 (mono: c = 0)."""
        ii, jj = torch.meshgrid(torch.arange(t0, t1), torch.arange(t0, t1), indexing="ij")
        ii, jj = ii.reshape(-1), jj.reshape(-1)
        keep = ((ii - jj).abs() > 0) & ((ii - jj).abs() <= r)
        self.add_factors(ii[keep], jj[keep])

    @torch.no_grad()
    def add_proximity_factors(self, t0=0, t1=0, rad=2, nms=2, beta=0.25, thresh=16.0, remove=False, dist=None):
        """Edge proposal (factor_graph.py:411-488): neighbourhood edges i-rad-1..i-1 <-> i for i in [t0, t), then
        proximity edges (i, j), i in [t0, t), j in [t1, t), j <= i - rad, in order of increasing frame distance with
        non-maximum suppression around every edge already present or just added; all made bidirectional.

        Integer-exact mirror of the reference: the frame distances come from ONE launch of the HIP `frame_distance`
        kernel and ONE device-to-host copy; the suppression / ordering logic (a few hundred candidates) then runs on
        the host exactly as the reference's Python does (which instead pays one `.item()` sync per candidate)."""
        assert t0 >= t1, "t0 should be a subset of t1"
        t = self.buffer.n_frames
        iin, jjn = np.meshgrid(np.arange(t0, t, dtype=np.int64), np.arange(t1, t, dtype=np.int64), indexing="ij")
        iin, jjn = iin.reshape(-1), jjn.reshape(-1)
        if iin.size == 0:
            return
        if dist is not None:  # frame distances of exactly these candidates, computed earlier (SLAMFrontend prefetch)
            d = np.array(dist, dtype=np.float32).reshape(-1)
            assert d.shape[0] == iin.shape[0]
        else:
            ii, jj = upload_many([iin, jjn], self.device)
            d = self.buffer.frame_distance_dense_disp(ii, jj, beta=beta)
            d = (d[:, 0] if d.shape[1] == 1 else d.mean(-1)).cpu().numpy().astype(np.float32)
        nj = t - t1

        def suppress(i, j):
            if (t0 <= i < t) and (t1 <= j < t):
                d[(i - t0) * nj + (j - t1)] = np.inf

        # edges already in the graph (active + inactive): the same suppression, all edges at once per window offset
        D = d.reshape(t - t0, nj)  # view of d
        h = self.host_edges()
        I = np.concatenate([h["ii"], h["ii_inac"]])
        J = np.concatenate([h["jj"], h["jj_inac"]])
        if I.size:
            lim = np.maximum(np.minimum(np.abs(I - J) - 2, nms), 0)
            for di in range(-nms, nms + 1):
                for dj in range(-nms, nms + 1):
                    sel = (abs(di) + abs(dj)) <= lim
                    a, b = I[sel] + di, J[sel] + dj
                    ok = (a >= t0) & (a < t) & (b >= t1) & (b < t)
                    D[a[ok] - t0, b[ok] - t1] = np.inf
        d[(iin - rad < jjn) | (d > thresh)] = np.inf
        es = []
        for i in range(t0, t):
            if self.cross_view:
                es.append((i, i))
                suppress(i, i)
            for j in range(max(i - rad - 1, 0), i):
                es.append((i, j))
                es.append((j, i))
                suppress(i, j)
        # candidates in order of increasing distance; only those not above the threshold NOW can ever be taken (suppression
        # only raises distances): the global BA's 40 000 candidates shrink to a few thousand before the Python loop.  The
        # suppression diamonds are index offsets precomputed per radius (factor_graph.py:455-460 loops di, dj per edge)
        order = np.argsort(d, kind="stable")
        order = order[d[order] <= thresh]
        nt = t - t0
        diamonds = []
        for lim_k in range(nms + 1):
            dd = [(di, dj) for di in range(-nms, nms + 1) for dj in range(-nms, nms + 1) if abs(di) + abs(dj) <= lim_k]
            diamonds.append((np.array([x[0] for x in dd]), np.array([x[1] for x in dd])))
        for k in order.tolist():
            if d[k] > thresh:
                continue
            if len(es) > self.max_factors:
                break
            i, j = int(iin[k]), int(jjn[k])
            es.append((i, j))
            es.append((j, i))
            ddi, ddj = diamonds[max(min(abs(i - j) - 2, nms), 0)]
            a, b = i - t0 + ddi, j - t1 + ddj
            ok = (a >= 0) & (a < nt) & (b >= 0) & (b < nj)
            d[a[ok] * nj + b[ok]] = np.inf
        if len(es) == 0:
            return
        e = np.asarray(es, dtype=np.int64)
        self.add_factors(e[:, 0], e[:, 1], remove)

    @torch.no_grad()
    def rm_second_newest_keyframe(self, ix):
        """factor_graph.py:204-228: drop keyframe ix (= n_frames - 2) from the buffer and the graph."""
        self.buffer.remove_second_newest(ix)
        active, inactive = self._index.drop_keyframe(ix)
        self._edges_changed()
        if inactive.any():
            keep_x = per_view(upload(np.flatnonzero(~inactive), self.device), self.buffer.n_views)
            self.target_inac = self.target_inac[:, keep_x]
            self.weight_inac = self.weight_inac[:, keep_x]
        self.rm_factors(active, store=False)

    def get_edges_np(self):
        """factor_graph.py:110-117."""
        ii, jj = self.ii.cpu().numpy(), self.jj.cpu().numpy()
        w = torch.mean(self.weight, dim=[0, 2, 3, 4]).cpu().numpy()
        ix = np.argsort(ii)
        return np.stack([ii[ix], jj[ix]], axis=1), w[ix]

    @property
    def f_net(self):
        """GRU hidden state in the reference's layout [1,E,128,h,w] (factor_graph.py:84-86)."""
        return None if self.net_n is None else self.net_n.permute(0, 3, 1, 2)[None]

    @property
    def inp(self):
        return None if self.xbuf is None else self.xbuf[..., 0:128].permute(0, 3, 1, 2)[None]

    def _net_spare(self):
        """Ping-pong buffer for the new hidden state (the Q epilogue cannot write in place: 3x3 halo): the other bank of
        the edge stores, or - for graphs without stores and states assigned from outside - a private tensor."""
        sp = self._stores.net_spare(self.net_n) if self._stores is not None else None
        if sp is not None:
            return sp
        sp = self._spare
        if sp is None or sp.shape != self.net_n.shape or sp.data_ptr() == self.net_n.data_ptr():
            sp = torch.empty_like(self.net_n)
        self._spare = self.net_n  # the current state becomes next iteration's spare
        return sp

    def _edge_plan(self):
        """Index tensors that only change when the edge set changes (the reference recomputes them, with a
        torch.unique sync, on every update: factor_graph.py:267-268)."""
        if self._plan is None:
            pi, qi, di, pj, qj, _ = self.buffer.expand_edge_multiview(self.ii, self.jj)
            ii_h, jj_h = self._index.host["ii"], self._index.host["jj"]
            self._plan_serial += 1
            if self.cross_view or self.buffer.n_views > 1:
                from .update_engine import segment_csr
                du, dix = torch.unique(di, return_inverse=True)  # multi-view: take the expansion as computed on the device
                n_src = int(du.numel())
                csr = segment_csr(dix, n_src)
            else:  # one view: di = ii, everything from the host arrays
                du_h, dix_h = np.unique(ii_h, return_inverse=True)
                du, dix = upload_many([du_h, dix_h], self.device)
                n_src = int(du_h.shape[0])
                csr = tuple(upload_many(host_csr(dix_h, n_src), self.device, torch.int32))
            self._plan = dict(pi=pi, qi=qi, di=di, pj=pj, qj=qj, du=du, dix=dix, n_src=n_src, csr=csr,
                              t0=int(max(1, ii_h.min() + 1)), t1=int(max(ii_h.max(), jj_h.max()) + 1), base=int(min(ii_h.min(), jj_h.min())))
        return self._plan

    def _inactive_room(self, k):
        """target_inac / weight_inac grow for the whole video (factor_graph.py:184-189 concatenates, i.e. copies the
        whole store, on every eviction): backing buffers with spare capacity; -> (target buffer, weight buffer, first
        free row) with room for k more rows, the attributes re-pointed to the n + k rows (the caller fills the new ones)."""
        n = self.target_inac.shape[1]
        cap = self._inac_cap
        if cap is None or cap[0].shape[1] < n + k or cap[0].data_ptr() != self.target_inac.data_ptr():
            size = max(2 * (n + k), 256)
            cap = tuple(torch.empty((1, size) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
                        for x in (self.target_inac, self.weight_inac))
            cap[0][:, :n] = self.target_inac
            cap[1][:, :n] = self.weight_inac
            self._inac_cap = cap
        self.target_inac, self.weight_inac = cap[0][:, :n + k], cap[1][:, :n + k]
        return cap[0], cap[1], n

    def _upsample_disps(self, mask, du, own=None):
        """mask [n_src,h,w,576] f16 of the operator (row s belongs to source slot du[s], as `eta` does in update_finish)
        -> buffer.disps_up[du] = convex upsampling of buffer.disps[du], read and written in place through the flattened
        (frame * V + view) rows: no gathers.  `droid_net_ext.cvx_upsample` is the only route to the kernel.
        `own` = (rows, keep) of `_own_rows`: the kernel skips the mask rows whose entry of `rows` is -1, and only the
        rows with `keep` set are flagged."""
        from ..ext import droid_net_ext
        buf = self.buffer
        require(buf.disps_up is not None, "FactorGraph.upsample needs GraphBuffer(upsample_disps=True)")
        droid_net_ext.cvx_upsample(buf.flattened_disps[..., None], mask, rows=du if own is None else own[0],
                                   out=buf.flattened_disps_up[..., None])
        flags = buf.disps_up_valid.view(-1)
        if own is None:
            flags[du] = True
        else:  # no boolean-mask indexing: that would read the count back
            flags[du] = flags[du] | own[1]

    def _own_rows(self, P):
        """`upsample_from_row`: (P["du"] with the rows before it mapped to -1, which rows are kept), once per edge plan"""
        key = ("own_rows", int(self.upsample_from_row))
        if key not in P:
            keep = P["du"] >= key[1]
            P[key] = (torch.where(keep, P["du"], torch.full_like(P["du"], -1)), keep)
        return P[key]

    def _shift_plan(self, plan5, base):
        """(pi, qi, di, pj, qj) -> the same relative to keyframe `base` (+ base), see GraphBuffer.bundle_adjustment"""
        pi, qi, di, pj, qj = plan5
        if self.cross_view or base <= 0:  # cross-view self edges may point anywhere in the buffer: keep absolute indices
            return (pi, qi, di, pj, qj, 0)
        V = self.buffer.n_views
        return (pi - base, qi, di - base * V, pj - base, qj, base)

    def _ba_plan(self, P):  # cached expand_edge_multiview of the edge set, relative to the oldest keyframe used
        if "ba_plan" not in P:
            P["ba_plan"] = self._shift_plan((P["pi"], P["qi"], P["di"], P["pj"], P["qj"]), P["base"])
        return P["ba_plan"]

    @staticmethod
    def _ba_flags(t0, t1, **flags):  # window, damping and flags of one BA (`bundle_adjustment`): `update`'s, with `flags` over them
        return dict(dict(t0=t0, t1=t1, pose_damping=1e-3, pose_ep=0.1, motion_only=False, limited_disp=False,
                         optimize_intrinsics=False, optimize_rig_rotation=False), **flags)

    def _contiguous_targets(self):  # they reach the kernels as addresses of dense [1,E,h,w,2] rows (no-op on such tensors)
        self.weight, self.target = self.weight.contiguous(), self.target.contiguous()

    @torch.no_grad()
    def update(self, t0=None, t1=None, itrs=3, use_inactive=False, motion_only=False, fixed_motion=False,
               limited_disp=False):
        """run update operator on factor graph (factor_graph.py:230-314)."""
        assert self.incremental and self.corr is not None and self.xbuf is not None and self.net_n is not None
        assert not (motion_only and fixed_motion)
        P = self._edge_plan()
        t0 = P["t0"] if t0 is None else t0
        t1 = P["t1"] if t1 is None else t1
        buf = self.buffer
        E_act = int(P["pi"].shape[0])
        WORK["edge_updates"] += E_act
        if "io" not in P:  # per edge set: persistent coords / motion-feature buffers (stable addresses), frame masks
            P["io"] = (torch.empty((E_act, self.ht, self.wd, 2), dtype=torch.float32, device=self.device),
                       torch.empty((E_act, self.ht, self.wd, 4), dtype=torch.float16, device=self.device))
            P["mask"] = buf.masks[P["pi"], P["qi"]].contiguous()
        self._contiguous_targets()
        # motion features + coords1 in one launch (factor_graph.py:253-261)
        coords1, motn = slam_ext.reproject_motion_nhwc(buf.poses, buf.flattened_disps, buf.intrinsics, buf.rig,
                                                       P["pi"], P["qi"], P["pj"], P["qj"], P["di"],
                                                       self.target[0], camera=buf.camera_type, out=P["io"])
        eng = self.update_op.engine(self.device)
        # the lookup is deferred into the correlation encoder's first convolution (one kernel, no [E,h,w,200] tensor); the
        # whole operator is one natively sequenced library call
        corr = self.corr.lookup_deferred(coords1)
        up = {"want_upmask": True} if self.upsample else {}  # the mask head on the persistent a2: one more 1x1 conv
        self.net_n, dw, eta, upmask = eng.forward_nhwc(self.net_n, self.xbuf, corr, motn, ix=P["dix"], n_src=P["n_src"],
                                                       net_out=self._net_spare(), csr=P["csr"], pgate=self.pgate,
                                                       gate_state=self._gate_state, **up)
        self._gate_state = None
        # The new hidden state is final here, and the dense BA below keeps ONE workgroup busy for most of its time
        # (band Cholesky): everything of the next iteration's gates that depends on the hidden state alone - the
        # global-context terms and the hidden-state third of the z|r convolution, 18 % of the operator's FLOPs - is
        # issued on a second stream now and joins after the BA.  Speculative: wasted (off the critical path) when the
        # edge set changes before the next call.  Small edge sets are launch bound, not compute bound: not worth it.
        overlap = self.pgate is not None and E_act >= self.gate_overlap_min_edges
        ba_overlap = None
        if overlap:
            main = torch.cuda.current_stream(self.device)
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(main)
            # the BA's shadow is shorter than the whole stage: the z|r part is staged for a share of the edges only (the
            # others keep the unsplit convolution), the small global-context part for all of them
            n_staged = max(1, int(round(self.gate_overlap_share * E_act)))
            if self.gate_overlap_mode == "gated":
                # handed to the BA, which releases it in one piece per Gauss-Newton iteration, each behind the start of
                # that iteration's solve (vipe_overlap_fn): the solve needs a whole CU's LDS and would otherwise queue
                # behind the convolution's workgroups
                with torch.cuda.stream(self._side):  # the small global-context part at once, next to the first accumulate
                    eng.hidden_gate_state(self.net_n, self.pgate, parts=1)
                # the last piece has nothing after its solve to hide behind: it is the smallest
                fr = self.gate_overlap_fractions if len(self.gate_overlap_fractions) == itrs else None
                gate_state, ov = eng.gate_state_job(self.net_n, self.pgate, fractions=fr, n_staged=n_staged)
                ba_overlap = ov(self._side)
            else:  # "free": launched at once, competes with every BA kernel
                with torch.cuda.stream(self._side):
                    gate_state = eng.hidden_gate_state(self.net_n, self.pgate, n_staged=n_staged)
        # factor_graph.py:270-276 in one launch: target = coords1 + delta, weight with masked frames zeroed
        # (`weight[:, masks[pi, qi]] = 0` without the host sync of a boolean-mask assignment), damping[du] = eta.
        # target / weight are rewritten IN PLACE: their addresses only change with the edge set, so consecutive
        # iterations chain through them and the steady state allocates nothing
        slam_ext.update_finish(coords1, dw, P["mask"], self.target, self.weight, eta, P["du"], self.damping)
        if use_inactive:
            # factor_graph.py:296-304.  The selection of inactive edges and its multiview expansion only change with
            # the edge sets (or t0): cached in the edge plan, so the steady-state iteration has no boolean-mask
            # indexing (a device-to-host sync each) and no re-expansion
            key = ("inac", t0)
            if key not in P:
                h = self._index.host
                sel_h = np.flatnonzero((h["ii_inac"] >= t0 - 3) & (h["jj_inac"] >= t0 - 3))  # host arrays: no read-back
                # [selected inactive | active] index vectors straight from the host arrays: one staged copy
                ii, jj, sel_exp = upload_many([np.concatenate([h["ii_inac"][sel_h], h["ii"]]),
                                               np.concatenate([h["jj_inac"][sel_h], h["jj"]]),
                                               per_view(sel_h, buf.n_views)], self.device)
                base = int(min(h["ii"].min(), h["jj"].min(), *(h[k][sel_h].min() for k in ("ii_inac", "jj_inac") if sel_h.size)))
                plan = self._shift_plan(buf.expand_edge_multiview(ii, jj)[:5], base)
                # [selected inactive | active] targets / weights live in ONE buffer per edge set: the inactive part is
                # gathered once (it never changes), self.target / self.weight are views of the tail that the iteration
                # rewrites in place - the reference concatenates both every call (factor_graph.py:300-304)
                n_sel = int(sel_exp.shape[0])
                comb = tuple(torch.empty((1, n_sel + E_act) + tuple(x.shape[2:]), dtype=x.dtype, device=x.device)
                             for x in (self.target, self.weight))
                comb[0][:, :n_sel] = self.target_inac.index_select(1, sel_exp)
                comb[1][:, :n_sel] = self.weight_inac.index_select(1, sel_exp)
                P[key] = (ii, jj, plan, comb, n_sel)
            ii, jj, plan, comb, n_sel = P[key]
            plan_key = (self._plan_serial, "inac", t0)
            if self.target.data_ptr() != comb[0][:, n_sel:].data_ptr():
                comb[0][:, n_sel:] = self.target
                comb[1][:, n_sel:] = self.weight
                self.target, self.weight = comb[0][:, n_sel:], comb[1][:, n_sel:]
            target, weight = comb
        else:
            ii, jj, target, weight = self.ii, self.jj, self.target, self.weight
            plan = self._ba_plan(P)
            plan_key = (self._plan_serial, "act")
        E = target.shape[1]
        self._last_ba = self._ba_flags(t0, t1 if not fixed_motion else t0, motion_only=motion_only, limited_disp=limited_disp)
        buf.bundle_adjustment(target.view(E, -1, 2), weight.view(E, -1, 2), self.damping, ii, jj, n_iters=itrs,
                              **self._last_ba, plan=plan, ba_state=self._ba_state, plan_key=plan_key, overlap=ba_overlap)
        if self.upsample:  # after the BA: this iteration's mask on the disparities it has just produced
            self._upsample_disps(upmask, P["du"], own=None if self.upsample_from_row is None else self._own_rows(P))
        if overlap:
            main.wait_stream(self._side)
            self._gate_state = gate_state
        self._index.tick()

    @torch.no_grad()
    def marginals(self, t0=None, t1=None, **flags):
        """Marginal covariances (`GraphBuffer.ba_marginals`) of the BA problem over the graph's current edges, targets,
        weights and damping at the buffer's current state -> (disp_var [n*V,h,w], pose_cov [n,6,6], info), rows by
        keyframe slot, NaN where a frame / pose is not free.  Window, damping and flags default to those of the last BA
        that `update` / `update_batch` issued (before any: `update`'s own defaults); `t0` / `t1` / `flags` override them.
        Runs in the shared BA workspace, not in this graph's private one."""
        P = self._edge_plan() if int(self.ii.shape[0]) else None
        ba = dict(self._last_ba or self._ba_flags(P["t0"] if P else 0, P["t1"] if P else 0))
        ba.update(flags)
        ba.update({k: v for k, v in (("t0", t0), ("t1", t1)) if v is not None})
        E = self.target.shape[1]
        return self.buffer.ba_marginals(self.target.contiguous().view(E, -1, 2), self.weight.contiguous().view(E, -1, 2),
                                        self.damping, self.ii, self.jj, **ba, plan=self._ba_plan(P) if P else None)

    def _backend_chunk(self, plan, gi, eng):
        """What does not change about chunk `gi` during the passes of `update_batch`, prepared once: idx_x - its rows of the per-edge-
        and-view tensors (None: the whole graph), edges - their `expand_edge_multiview`; du, dixs, csr - buffer rows of the source
        nodes, source node of every row, its `host_csr`; mask - the source views' frame masks; xb - the operator's input [n,h,w,320]
        with the context features and, as the frontend has per edge, pgate - their part of the GRU gates (19 % of its FLOPs) or None"""
        buf, V, ii_np = self.buffer, self.buffer.n_views, self._index.host["ii"]
        sel = np.flatnonzero(np.isin(ii_np // 8 * 8, plan.groups[gi]))  # from the host arrays: an index vector, not a mask
        if sel.shape[0] == ii_np.shape[0]:
            idx_x, iis, jjs = None, self.ii, self.jj
        else:
            idx = upload(sel, self.device)
            idx_x, iis, jjs = per_view(idx, V), self.ii[idx], self.jj[idx]
        edges = buf.expand_edge_multiview(iis, jjs)
        pis, qis = edges[:2]
        du_np, dixs_np = np.unique(per_view(ii_np[sel], V), return_inverse=True)
        du, dixs = upload_many([du_np, dixs_np], self.device)
        mask = buf.masks[pis, qis].contiguous()
        csr = tuple(upload_many(host_csr(dixs_np, du_np.shape[0]), self.device, torch.int32))
        xb = torch.empty((plan.rows[gi], self.ht, self.wd, 320), dtype=torch.half, device=self.device)
        xb[..., 0:128] = buf.inps[pis, qis].permute(0, 2, 3, 1)
        pgate = eng.gate_context(xb) if eng.supports_gate_split(self.ht, self.wd) else None
        return _BackendChunk(idx_x=idx_x, edges=edges, du=du, dixs=dixs, csr=csr, mask=mask, xb=xb, pgate=pgate)

    @torch.no_grad()
    def update_batch(self, itrs, steps, optimize_intrinsics, optimize_rig_rotation, solver_verbose=False):
        """Backend update (hot loop B, factor_graph.py:316-394): volume-free correlation (AltCorrBlock over the
        buffer's feature maps), the flow-update operator applied in chunks of 8 source keyframes, then ONE dense BA
        over all edges with `itrs` Gauss-Newton iterations (t0 = 1, t1 = n_frames, pose damping 1e-5 / 1e-2)."""
        assert self.net_n is not None
        buf, eng = self.buffer, self.update_op.engine(self.device)
        # The reference's backend uses the volume-free AltCorrBlock to fit 24 GB devices (droid_net.py:121-176).  With
        # 288 GB of HBM the per-chunk volume (~33 MB per edge, ~1.5 GB per chunk of 8 source keyframes) is cheap, and
        # building it (one fused kernel, 10 us per edge) + the fused lookup is >10x faster than 49 x 128-channel dot
        # products per pixel and level; the volume kernels cover every grid (blocked store on the padded grid), AltCorrBlock
        # stays the reference-shaped alternative (VIPE_AMD_BACKEND_ALTCORR=1) for devices where the volumes do not fit.
        from ..ext import droid_net_ext
        use_volume = (droid_net_ext.fused_build_covers(buf.flattened_fmaps.shape[1], self.ht, self.wd, 4, buf.flattened_fmaps.dtype)
                      and os.environ.get("VIPE_AMD_BACKEND_ALTCORR") is None)
        corr_op = None if use_volume else AltCorrBlock(buf.flattened_fmaps[None])
        P, V = self._edge_plan(), buf.n_views
        ii_np = self._index.host["ii"]
        assert self._index.host["jj"].max() >= ii_np.max()
        G_, S_, R_ = droid_net_ext.blocked_dims(self.ht, self.wd)[:3]  # the store is padded to G x 64 sources, R x 4 rows, S x 32 columns
        plan = plan_backend_chunks(np.bincount(ii_np), V, (G_ * 64) * (R_ * 4 * S_ * 32) * 2 * (1 + 1 / 4 + 1 / 16 + 1 / 64), steps,
                                   use_volume, float(os.environ.get("VIPE_AMD_BACKEND_VOLUME_GB", BACKEND_VOLUME_GB)) * 2**30,
                                   int(os.environ.get("VIPE_AMD_BACKEND_CHUNK_EDGES", "4096")))
        chunks, kept = {}, _PyramidResidency(plan)
        for step in range(steps):
            # the last pass's masks are kept per chunk until its BA has run ([n_src,h,w,576] f16 each: 3.5 MB per source
            # keyframe and view at 48 x 64); earlier passes do not ask for them
            up = {"want_upmask": True} if self.upsample and step == steps - 1 else {}
            upmasks = []
            coords1, motn = slam_ext.reproject_motion_nhwc(buf.poses, buf.flattened_disps, buf.intrinsics, buf.rig,
                                                           P["pi"], P["qi"], P["pj"], P["qj"], P["di"],
                                                           self.target[0].contiguous(), camera=buf.camera_type)
            for gi in range(len(plan.groups)):
                if gi not in chunks:
                    chunks[gi] = self._backend_chunk(plan, gi, eng)
                c, n = chunks[gi], plan.rows[gi]
                take = (lambda x: x) if c.idx_x is None else (lambda x: x.index_select(0, c.idx_x))  # noqa: E731
                c1 = take(coords1)
                pis, qis, dis, pjs, qjs, djs = c.edges
                if use_volume:
                    vol = kept.get(gi)
                    if vol is None:
                        corr_n = None  # the previous chunk's lookup handle holds its pyramid: back to the allocator BEFORE this build
                        lo, hi = (0, buf.n_frames) if (self.cross_view and V > 1) else (P["base"], P["t1"])
                        vol = CorrBlock.from_buffer(buf.flattened_fmaps, pis * V + qis, pjs * V + qjs, frame_range=(lo * V, hi * V))
                        WORK["pyramids_built"] += n
                        kept.offer(gi, vol)
                    corr_n = vol.lookup_deferred(c1)
                else:
                    corr1 = corr_op(c1[None], dis, djs)  # [1,n,196,h,w] fp32
                    corr_n = torch.zeros((n, self.ht, self.wd, 200), dtype=torch.half, device=self.device)
                    corr_n[..., :196] = corr1[0].permute(0, 2, 3, 1)
                net, dw, eta, upmask = eng.forward_nhwc(take(self.net_n).contiguous(), c.xb, corr_n, take(motn).contiguous(),
                                                        ix=c.dixs, n_src=int(c.du.shape[0]), csr=c.csr, pgate=c.pgate, **up)
                if up:
                    upmasks.append((upmask, c.du))
                WORK["edge_updates"] += n
                self._gate_state = None
                if c.idx_x is None:  # the whole graph
                    self.net_n = net if net.data_ptr() != self.net_n.data_ptr() else net.clone()
                    self._contiguous_targets()
                    slam_ext.update_finish(c1, dw, c.mask, self.target, self.weight, eta, c.du, self.damping)
                else:  # the reference's own ops, not `update_finish`: one form for both would change the launches of this branch
                    weight = dw[..., 2:4].masked_fill(c.mask.unsqueeze(-1), 0.0)
                    self.net_n[c.idx_x] = net
                    self.target[0, c.idx_x] = c1 + dw[..., 0:2]
                    self.weight[0, c.idx_x] = weight
                    self.damping[c.du] = eta
            E = self.target.shape[1]
            self._last_ba = self._ba_flags(1, buf.n_frames, pose_damping=1e-5, pose_ep=1e-2, optimize_intrinsics=optimize_intrinsics,
                                           optimize_rig_rotation=optimize_rig_rotation)
            buf.bundle_adjustment(self.target.view(E, -1, 2), self.weight.view(E, -1, 2), self.damping, self.ii, self.jj,
                                  n_iters=itrs, **self._last_ba, verbose=solver_verbose)
            for upmask, du in upmasks:
                self._upsample_disps(upmask, du)
