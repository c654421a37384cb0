"""Sparse keypoint tracks between a tracker and the dense path - mirror of the `SparseTracks` base class
(vipe/slam/components/sparse_tracks/__init__.py:27-141).  The reference's trackers (cuVSLAM, SuperPoint) are outside the
path: a subclass fills `observations` in `track_image`; `ReplayedSparseTracks` takes them from the caller, and
`KLTSparseTracks` is a tracker of this project (corners + pyramidal Lucas-Kanade in HIP, klt_track.hip).

What the dense path reads: `get_correspondences` / `get_observations` (the motion filter's track score) and
`compute_dense_disp_target_weight` (the second flow term of the BA, buffer.py:422-447): per edge the flow of the keypoints
seen in both frames, splatted bilinearly onto the 1/8 grid.  The reference loops over the edges on the host with eight
`index_add_` launches and two device uploads per edge; here the correspondences of ALL edges are gathered on the host
once, uploaded once, and splatted by two launches of the library's atomic scatter kernel."""
import numpy as np
import torch

from .._lib import upload
from ..ext import scatter_ext


class SparseTracks:
    """Single-camera tracks, as the reference: observations[view][frame] = {keypoint id: (u, v) in image pixels}."""
    enabled = True

    def __init__(self, n_views):
        self.observations = [[] for _ in range(n_views)]

    def track_image(self, frame_data_list):
        raise NotImplementedError("a tracker fills `observations`; see ReplayedSparseTracks")

    def get_correspondences(self, view_idx, source_frame_idx, target_frame_idx):
        """ids of the keypoints observed in both frames (ascending)"""
        a, b = self.observations[view_idx][int(source_frame_idx)], self.observations[view_idx][int(target_frame_idx)]
        return torch.tensor(sorted(a.keys() & b.keys()), dtype=torch.long)

    def get_observations(self, view_idx, frame_idx, keypoint_indices):
        if len(keypoint_indices) == 0:
            return torch.empty(0, 2, device=keypoint_indices.device)
        uvs = self.observations[view_idx][int(frame_idx)]
        return torch.tensor(np.stack([uvs[int(k)] for k in keypoint_indices.cpu().numpy()], 0)).to(keypoint_indices.device).float()

    def compute_dense_disp_target_weight(self, source_view_inds, source_frame_inds, target_view_inds, target_frame_inds,
                                         image_size, dense_disp_size):
        """-> target [E,h,w,2] (grid position + mean track flow of the cell), weight [E,h,w,2] (splatted bilinear weights,
        cells below 0.1 cleared).  sparse_tracks/__init__.py:68-141 with `bilinear_splatting_inplace` (utils/depth.py:123-155):
        corner (floor(u + 0.5), floor(v + 0.5)) and its right / lower neighbours, weights from the offset to that corner -
        which lies in [-0.5, 0.5), so they are not the usual bilinear weights - points whose four corners are not all
        inside the grid are dropped."""
        device = source_view_inds.device
        E, (h, w) = len(source_view_inds), dense_disp_size
        assert E == len(target_view_inds) == len(source_frame_inds) == len(target_frame_inds)
        sv, sf = source_view_inds.cpu().numpy(), source_frame_inds.cpu().numpy()
        tv, tf = target_view_inds.cpu().numpy(), target_frame_inds.cpu().numpy()
        terms, src, flow = [], [], []
        for e in range(E):
            assert sv[e] == tv[e], "Only same view tracking is supported"
            a, b = self.observations[sv[e]][int(sf[e])], self.observations[tv[e]][int(tf[e])]
            ids = sorted(a.keys() & b.keys())
            if ids:
                s = np.asarray([a[k] for k in ids], np.float32).reshape(-1, 2)
                terms.append(np.full(len(ids), e, np.int64))
                src.append(s)
                flow.append(np.asarray([b[k] for k in ids], np.float32).reshape(-1, 2) - s)
        value = torch.zeros(E * h * w, 2, device=device)
        weight = torch.zeros(E * h * w, device=device)
        if terms:
            fac = torch.tensor([w / image_size[1], h / image_size[0]], device=device)
            term = torch.from_numpy(np.concatenate(terms)).to(device)
            uv = torch.from_numpy(np.concatenate(src)).to(device) * fac
            data = torch.from_numpy(np.concatenate(flow)).to(device) * fac
            u, v = uv.unbind(-1)
            x0, y0 = torch.floor(u + 0.5).long(), torch.floor(v + 0.5).long()
            ok = (x0 >= 0) & (x0 + 1 < w) & (y0 >= 0) & (y0 + 1 < h)
            term, data, u, v, x0, y0 = term[ok], data[ok], u[ok], v[ok], x0[ok], y0[ok]
            wx, wy = u - x0.float(), v - y0.float()
            base = term * (h * w) + y0 * w + x0
            idx = torch.cat([base, base + w, base + 1, base + w + 1])                       # (x0,y0) (x0,y1) (x1,y0) (x1,y1)
            cw = torch.cat([(1 - wx) * (1 - wy), (1 - wx) * wy, wx * (1 - wy), wx * wy])
            if idx.numel():
                scatter_ext.scatter_sum(data.repeat(4, 1) * cw[:, None], idx, 0, value, None)
                scatter_ext.scatter_sum(cw.contiguous(), idx, 0, weight, None)
        value = (value / weight[:, None]).view(E, h, w, 2)
        weight = weight.view(E, h, w, 1).repeat(1, 1, 1, 2)
        value[torch.isnan(value)] = 0.0
        value[weight < 0.1] = 0.0
        weight[weight < 0.1] = 0.0
        yy, xx = torch.meshgrid(torch.arange(h, device=device), torch.arange(w, device=device), indexing="ij")
        value[..., 0] += xx
        value[..., 1] += yy
        return value, weight


class DummySparseTracks(SparseTracks):
    """sparse_tracks/__init__.py:144-149: no tracker"""
    enabled = False

    def track_image(self, frame_data_list):
        for obs in self.observations:
            obs.append({})


class KLTSparseTracks(SparseTracks):
    """The project's own tracker: min-eigenvalue corners, one per free cell, followed by pyramidal Lucas-Kanade with a
    forward-backward check (klt_track.hip through `klt_ext`; include/vipe_amd.h states the arithmetic, DESIGN.md 14 the
    choice of the defaults).  Every view is tracked on its own.

    Per view and frame: the pyramid of the new frame; the live points tracked from the previous frame, forward and
    backward; every point with a non-zero status dropped; a new corner in every cell that holds no survivor - unless it
    crowds another point (`_spread`: closer than cell / 4 pixels never, closer than cell / 2 rarely) - with ids rising in
    ascending cell order.
    The work runs on a stream of the tracker's own, ordered after the caller's stream by an event, and the host waits on
    the tracker's event only - never on the device.

    `resize` (a `StandardResize`, or one per view): the frames are tracked at the size they come in and the observations
    are reported in the resized, cropped image (`forward_intrinsics`' scale and crop); points outside the crop are not
    reported.  `_kernels`: an object with klt_ext's `pyramid`, `detect`, `track` (tests drive the class with the numpy
    reference on CPU tensors)."""
    accepts_resize = True  # SLAMSystem.run(native_resolution=True) hands its per-view StandardResize over

    def __init__(self, n_views, levels=4, win_radius=4, n_iters=10, eps=0.01, cell=16, border=8, min_eig=4.0,
                 max_residual=12.0, fb_thresh=0.5, max_flow=64.0, resize=None, device="cuda", _kernels=None):
        super().__init__(n_views)
        if _kernels is None:
            from ..ext import klt_ext as _kernels
            self.device = torch.device(device)
        else:
            self.device = torch.device("cpu")
        self._k = _kernels
        self.levels, self.cell = int(levels), int(cell)
        self.params = dict(win_radius=int(win_radius), n_iters=int(n_iters), eps=float(eps), border=int(border),
                           min_eig=float(min_eig), max_residual=float(max_residual), fb_thresh=float(fb_thresh),
                           max_flow=float(max_flow))
        self.set_resize(resize)
        self.next_id = 0
        self.last_status = [None] * n_views  # status bytes of the points tracked into the newest frame (diagnostics)
        self._state = [None] * n_views       # per view: dict(size, levels, pyr, pts (device [N,2]), ids (host [N]))
        self._stream = self._done = None

    def set_resize(self, resize):
        n = len(self.observations)
        self.resizes = list(resize) if isinstance(resize, (list, tuple)) else [resize] * n
        assert len(self.resizes) == n, "one StandardResize per view"

    def _levels_for(self, H, W):
        """the configured levels, fewer for a small frame: the coarsest level keeps a short side of at least 24 pixels"""
        L = 1
        while L < self.levels and (min(H, W) >> L) >= 24:
            L += 1
        return L

    def _report(self, view, pts):
        """host [N,2] positions in the tracked frame -> ([N,2] in the reported frame, [N] bool inside it)"""
        r = self.resizes[view]
        if r is None:
            return pts, np.ones(len(pts), bool)
        (h0, w0), (h1, w1), (H, W) = r.native_size, r.size, r.out_size
        uv = pts * np.array([w1 / w0, h1 / h0]) - np.array([r.scx, r.scy], np.float64)
        return uv, (uv[:, 0] >= 0) & (uv[:, 0] <= W - 1) & (uv[:, 1] >= 0) & (uv[:, 1] <= H - 1)

    def _launch(self, view, frame):
        """everything of one view that runs on the device -> host copies (fwd [N,2], status [N], cells [n_cells,3])"""
        k, dev = self._k, self.device
        rgb = frame.rgb.to(dev)
        if rgb.dtype not in (torch.uint8, torch.float32):
            rgb = rgb.float()
        rgb = rgb.contiguous()
        H, W = int(rgb.shape[0]), int(rgb.shape[1])
        mask = None if frame.mask is None else frame.mask.to(dev).contiguous().view(torch.uint8)
        st = self._state[view]
        if st is not None and st["size"] != (H, W):
            raise ValueError("the frame size of a view changed between frames")
        L = self._levels_for(H, W) if st is None else st["levels"]
        n_cells = -(-H // self.cell) * -(-W // self.cell)
        pyr = k.pyramid(rgb, L)
        busy = torch.zeros(n_cells, dtype=torch.uint8, device=dev)
        fwd = status = None
        if st is not None and len(st["ids"]):
            fwd, status, _ = k.track(st["pyr"], pyr, H, W, L, st["pts"], mask=mask, **self.params)
            k.track(pyr, st["pyr"], H, W, L, fwd, fb_ref=st["pts"], status=status, cell=self.cell, cell_busy=busy,
                    **self.params)
        cells = k.detect(pyr[:H * W].view(H, W), self.cell, self.params["border"], self.params["min_eig"], mask=mask,
                         cell_busy=busy)
        ids = st["ids"] if st is not None else np.zeros(0, np.int64)
        self._state[view] = dict(size=(H, W), levels=L, pyr=pyr, pts=None, ids=ids)

        def host(t):  # on the device: a pinned staging buffer per result, the copy asynchronous on the tracker's stream
            if t is None or dev.type != "cuda":
                return t
            return torch.empty(t.shape, dtype=t.dtype, pin_memory=True).copy_(t, non_blocking=True)
        return host(fwd), host(status), host(cells)

    def _spread(self, pts, new, H, W):
        """the new corners [M,2] (one per free cell, ascending cell order) that keep their distance from every survivor
        `pts` and from each other (at least cell / 4 pixels; a pair closer than cell / 2 may go).  The detector's cells
        cut a corner region that straddles a cell edge into two corners a few pixels apart, which then travel together;
        without this the number of points creeps up frame by frame.  Blocks of cell / 4 pixels: a corner is taken if no
        point lies in the 3 x 3 blocks around its own.  Corners of cells of one parity (row % 2, column % 2) are more
        than a cell apart, so each of the four parities is decided at once and the result does not depend on the order
        inside it."""
        b = max(self.cell // 4, 1)
        occ = np.zeros((H // b + 3, W // b + 3), bool)  # one block of padding on every side
        by, bx = np.floor(pts[:, 1] + 0.5).astype(np.int64) // b + 1, np.floor(pts[:, 0] + 0.5).astype(np.int64) // b + 1
        occ[np.clip(by, 0, occ.shape[0] - 1), np.clip(bx, 0, occ.shape[1] - 1)] = True
        ny, nx = new[:, 1].astype(np.int64) // b + 1, new[:, 0].astype(np.int64) // b + 1
        cy, cx = new[:, 1].astype(np.int64) // self.cell, new[:, 0].astype(np.int64) // self.cell
        keep = np.zeros(len(new), bool)
        for parity in range(4):
            idx = np.flatnonzero((cy % 2 == parity // 2) & (cx % 2 == parity % 2))
            taken = np.zeros(len(idx), bool)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    taken |= occ[ny[idx] + dy, nx[idx] + dx]
            idx = idx[~taken]
            keep[idx] = True
            occ[ny[idx], nx[idx]] = True
        return new[keep]

    def _collect(self, view, fwd, status, cells):
        """host side of one view: survivors, new corners, ids, the observation dictionary, next frame's points"""
        st = self._state[view]
        ids, pts = st["ids"], np.zeros((0, 2), np.float64)
        if fwd is not None:
            status = status.numpy()
            self.last_status[view] = status.copy()
            fwd = fwd.numpy().astype(np.float64)
            keep = np.flatnonzero(status == 0)
            ids, pts = ids[keep], fwd[keep]
        else:
            self.last_status[view] = None
            ids = ids[:0]
        cells = cells.numpy().astype(np.float64)
        new = self._spread(pts, cells[cells[:, 0] >= 0, :2], *st["size"])  # ascending cell order
        ids = np.concatenate([ids, self.next_id + np.arange(len(new), dtype=np.int64)])
        self.next_id += len(new)
        pts = np.concatenate([pts, new], 0)
        st["ids"] = ids
        st["pts"] = upload(pts.astype(np.float32), self.device, torch.float32)  # staged through pinned memory: no stream drain
        uv, inside = self._report(view, pts)
        uv = np.ascontiguousarray(uv[inside])  # the dictionary's values are the rows of this one array
        self.observations[view].append(dict(zip(ids[inside].tolist(), uv)))

    def track_image(self, frame_data_list):
        frames = frame_data_list if isinstance(frame_data_list, (list, tuple)) else [frame_data_list]
        assert len(frames) == len(self.observations), "one frame per view"
        if self.device.type != "cuda":
            for v, f in enumerate(frames):
                self._collect(v, *self._launch(v, f))
            return
        if self._stream is None:
            self._stream, self._done = torch.cuda.Stream(device=self.device), torch.cuda.Event()
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        self._stream.wait_event(ready)  # the frames are produced on the caller's stream
        with torch.cuda.stream(self._stream):
            pending = [self._launch(v, f) for v, f in enumerate(frames)]
            self._done.record(self._stream)
            self._done.synchronize()  # the tracker's own event: nothing else on the device is waited for
            for v, p in enumerate(pending):
                self._collect(v, *p)  # next frame's points are uploaded on the tracker's stream


class ReplayedSparseTracks(SparseTracks):
    """Tracks computed elsewhere: `tracks[view][frame]` = {keypoint id: (u, v)}, handed over frame by frame."""

    def __init__(self, tracks):
        super().__init__(len(tracks))
        self._tracks = tracks

    def track_image(self, frame_data_list):
        for v, obs in enumerate(self.observations):
            obs.append(dict(self._tracks[v][len(obs)]))
