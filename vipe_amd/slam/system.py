"""`SLAMSystem` - host-side mirror of the reference's top-level driver (vipe/slam/system.py:51-316) over frames that are
already decoded and resident on the device - resized by the caller, or at their native size with
`run(..., native_resolution=True)` (`ingest.py`: the reference's resize / crop step as one fused kernel per view); decoding /
the monocular depth networks / sparse tracks / the rerun visualisation are outside the path, SURVEY 8:

    pass 1  every frame through the motion filter; accepted frames (and the last one) become keyframes - features and
            context into the buffer, sensor disparities from the frame's metric depth or a caller-supplied depth model,
            poses from the frame when given - then `SLAMFrontend.run()`; `SLAMBackend.run_if_necessary(5)` at
            `frontend_backend_iters` keyframes (system.py:236-273).  Scheduled as a two-stage pipeline
            (`SLAMConfig.pipeline_filter`): the filter of frame f+1 - feature encoder + one application of the update
            operator against the last keyframe, which depend on nothing the frontend changes - is enqueued on a side stream
            BEFORE keyframe f is optimised on the main stream and its score is collected afterwards
            (`MotionFilter.prefetch` / `check`); same decisions, same results, the filter fills the chip the frontend's
            single-workgroup solves leave idle
            `SLAMBackend.run(7)`, `SLAMBackend.run(backend_iters)` (system.py:279-282)
    pass 2  every frame appended again behind the keyframes, `InnerFiller` in chunks (system.py:284-294); with
            `SLAMConfig.frame_depth` (an addition) every chunk leaves as depth maps at the frames' native size
            `extract_slam_map`, `SLAMOutput(trajectory = filled poses inverted, intrinsics, rig, map)` (system.py:303-316)
"""
from dataclasses import dataclass, field, replace

import torch

from ..ext.lietorch import SE3
from .backend import BackendArgs, SLAMBackend
from .buffer import GraphBuffer
from .frontend import FrontendArgs, SLAMFrontend
from .ingest import StandardResize, ingest_frames
from .inner_filler import InfillArgs, InnerFiller
from .interface import SLAMOutput
from .motion_filter import DroidNet, MotionFilter


@dataclass
class SLAMConfig:
    """configs/slam/default.yaml (the fields the path reads)"""
    buffer: int = 1024
    filter_thresh: float = 2.4
    init_disp: float = 1.0
    map_filter_thresh: float = 0.05
    frontend_backend_iters: tuple = (16, 64, 256)
    cross_view_idx: object = None
    frontend: FrontendArgs = field(default_factory=FrontendArgs)
    backend: BackendArgs = field(default_factory=BackendArgs)
    infill: InfillArgs = field(default_factory=InfillArgs)
    # not in the reference's configuration - how THIS build schedules pass 1 (results do not depend on either):
    pipeline_filter: bool = True   # motion filter of frame f+1 on a side stream under keyframe f's frontend step
    pause_gc: bool = True          # keep the cyclic collector off during run() (its gen-2 sweeps cost up to 0.4 s per clip)
    release_cached_memory: bool = False  # several clips share this card (one process each): hand the global BA's pyramid
                                         # blocks (~100 GB at 200 keyframes) back to the driver after the second backend pass
                                         # instead of keeping them cached for the next clip of this process
    upsample_disps: bool = False   # full-resolution keyframe disparities (`SLAMOutput.keyframe_disps_up`): the operator's
                                   # convex-upsampling mask applied after every BA of the frontend and after the last
                                   # one of every backend pass; 4 * V * H * W bytes per buffer slot.  Off: nothing changes
    disp_uncertainty: bool = False  # marginal covariances of the last global BA (`SLAMOutput.keyframe_disp_var` /
                                    # `keyframe_pose_cov`): one `FactorGraph.marginals` call per clip after the last backend
                                    # pass, with that pass's BA arguments.  Off: nothing is allocated, no launch differs
    frame_depth: bool = False      # one depth map per FRAME and view (`SLAMOutput.frame_depths`): the buffer gets
                                   # `disps_up` and the keyframe graphs upsample as with `upsample_disps`; pass 2 runs with
                                   # `infill_dense_disp` forced on - that changes it from motion-only to poses AND
                                   # disparities of every frame - and upsamples each chunk's own rows after the last of
                                   # its ten BAs; one `vipe_depth_export` launch per chunk takes them (a keyframe's frame
                                   # takes the keyframe's row) to the native size as depth.  Off: nothing changes
    frame_depth_dtype: torch.dtype = torch.float16   # of `frame_depths` / the sink's maps (float16 or float32)
    frame_depth_sink: object = None  # callable (frame_idx, view_idx, depth [H0,W0] device tensor), called in frame order
                                     # as pass 2's chunks complete (`driver.artifacts.DepthZipWriter`); `frame_depths`
                                     # then stays None: a long clip does not hold T native-size maps on the device
    frame_depth_conf: bool = False  # beside every map of `frame_depth` a uint8 map `SLAMOutput.frame_depth_conf`:
                                    # per pixel, how many of the frame's nearest keyframes (same view) see its point and
                                    # how many confirm its depth; one `vipe_depth_consistency` launch per chunk, right
                                    # after the export and on its rows.  It only reads.  Off: nothing is allocated, no
                                    # launch differs
    frame_depth_conf_neighbours: int = 4   # keyframes per frame (1 to 8), nearest in time (`ingest.nearest_keyframes`)
    frame_depth_conf_tol: float = 0.05     # relative disparity (= depth) difference that still agrees; `map_filter_thresh`'s value
    frame_depth_conf_sink: object = None   # callable (frame_idx, view_idx, conf [H0,W0] uint8 device tensor), in frame order;
                                           # `frame_depth_conf` then stays None
    fused_cloud: bool = False      # one voxel-fused point cloud per clip (`SLAMOutput.fused_cloud`): one
                                   # `vipe_cloud_fuse` launch per chunk behind the consistency launch, on its rows and its
                                   # bytes, into a hash table that stays on the device; one `vipe_cloud_extract` after pass
                                   # 2.  Needs `frame_depth` and `frame_depth_conf`.  It only reads.  Off: nothing is
                                   # allocated, no launch differs
    fused_cloud_voxel: float = 0.02        # voxel edge in the trajectory's units (a default, not a measurement)
    fused_cloud_min_agree: int = 2         # keyframes that must confirm a pixel's depth (0 to 8; `frame_depth_conf`'s low nibble)
    fused_cloud_stride: int = 1            # every stride-th pixel in x and y (1 to 8)
    fused_cloud_capacity: int = 1 << 22    # slots of the table (a power of two; 40 bytes each); a full table drops points
                                           # and `FusedCloud.stats` says how many
    fused_cloud_min_count: int = 2         # points a voxel needs to be extracted
    fused_cloud_color: bool = True         # mean colour per voxel from the frames handed to `run`
    fused_depth: bool = False      # the fused cloud drawn back into every frame and view (`SLAMOutput.fused_depths`, DESIGN
                                   # 19): after the extraction, per pass-2 chunk of frames one `vipe_cloud_render` and one
                                   # `vipe_cloud_resolve` launch with the final poses, on the grid of `frame_depths`.  Needs
                                   # `fused_cloud`.  It only reads.  Off: nothing is allocated, no launch differs
    fused_depth_max_radius: int = 2        # largest footprint radius in pixels (0 to 4); a point covers its voxel's size
    fused_depth_color: bool = False        # `SLAMOutput.fused_rgb` beside the maps (needs `fused_cloud_color`)
    fused_depth_sink: object = None        # callable (frame_idx, view_idx, depth [H0,W0] device tensor), in frame order
                                           # (`driver.artifacts.DepthZipWriter`); `fused_depths` then stays None
    complete_depth: bool = False   # hole-free fused maps (`SLAMOutput.complete_depths`): `fused_depths` where they
                                   # exist, elsewhere the frame's own `frame_depths` aligned to the nearest fused samples
                                   # (scale and shift in the disparity domain, `ingest.depth_complete`); per pass-2 chunk one
                                   # `vipe_depth_anchor_bits` and one `vipe_depth_complete` launch right after the resolve.
                                   # Needs `fused_depth` and both kinds of maps kept (no `frame_depth_sink`, no
                                   # `fused_depth_sink`).  It only reads.  Off: nothing is allocated, no launch differs
    complete_depth_k: int = 5              # fused samples a pixel is aligned to (1 to 8), nearest first
    complete_depth_radius: int = 32        # how far, in pixels, a sample may lie (1 to 64); no sample in reach: the pixel stays 0
    complete_depth_sink: object = None     # callable (frame_idx, view_idx, depth [H0,W0] device tensor), in frame order;
                                           # `complete_depths` then stays None
    sparse_tracks: str = None     # "klt": `run` builds a `KLTSparseTracks(n_views)` (corners + pyramidal Lucas-Kanade in
                                   # HIP) when the caller passed no tracker - the motion filter's track score and the BA's
                                   # track term get real tracks.  None: no tracker is built, nothing is launched or changed
    backend_lock_path: str = None        # ... and let their global-BA phases - each fills the chip by itself and wants the
                                         # pyramid budget to itself - take turns (an advisory file lock held around the two
                                         # backend passes), while the other clips' pass 1 / pass 2 run beside it


@dataclass
class Frame:
    """What the path reads of the reference's `VideoFrame` (one per view): rgb [H,W,3] float 0-1, optional mask [H,W]
    bool (True = usable pixel, system.py:199-211), metric depth [H,W], intrinsics [4] (or [5] MEI) at frame resolution,
    camera->world pose (SE3)."""
    rgb: torch.Tensor
    mask: torch.Tensor = None
    metric_depth: torch.Tensor = None
    intrinsics: torch.Tensor = None
    pose: SE3 = None


class SLAMSystem:
    def __init__(self, device=torch.device("cuda"), config=None, droid_net=None, depth_model=None, sparse_tracks=None,
                 motion_filter_cls=MotionFilter):
        self.device, self.config = device, config or SLAMConfig()
        self.motion_filter_cls = motion_filter_cls  # pluggable keyframe selection (same constructor / check / prefetch)
        self.droid_net = droid_net if droid_net is not None else DroidNet()
        self.metric_depth = depth_model  # system.py:114-127 builds it from `keyframe_depth`; here the caller's
        self.sparse_tracks = sparse_tracks
        assert self.config.sparse_tracks in (None, "klt"), "SLAMConfig.sparse_tracks: None or 'klt'"
        if self.config.frame_depth_conf:
            c = self.config
            assert c.frame_depth, "SLAMConfig.frame_depth_conf rates the maps of frame_depth: set frame_depth=True as well"
            assert 1 <= int(c.frame_depth_conf_neighbours) <= 8, "SLAMConfig.frame_depth_conf_neighbours: 1 to 8"
            assert c.frame_depth_conf_tol > 0, "SLAMConfig.frame_depth_conf_tol must be positive"
        if self.config.fused_cloud:
            c = self.config
            assert c.frame_depth and c.frame_depth_conf, \
                "SLAMConfig.fused_cloud fuses the maps of frame_depth that frame_depth_conf rates: set both as well"
            assert c.fused_cloud_voxel > 0 and c.fused_cloud_voxel < float("inf"), "SLAMConfig.fused_cloud_voxel must be positive and finite"
            assert 0 <= int(c.fused_cloud_min_agree) <= 8, "SLAMConfig.fused_cloud_min_agree: 0 to 8"
            assert 1 <= int(c.fused_cloud_stride) <= 8, "SLAMConfig.fused_cloud_stride: 1 to 8"
            cap = int(c.fused_cloud_capacity)
            assert 0 < cap <= 1 << 30 and cap & (cap - 1) == 0, "SLAMConfig.fused_cloud_capacity: a power of two, at most 2^30"
            assert int(c.fused_cloud_min_count) >= 1, "SLAMConfig.fused_cloud_min_count: at least 1"
        if self.config.fused_depth:
            c = self.config
            assert c.fused_cloud, "SLAMConfig.fused_depth draws the cloud of fused_cloud: set fused_cloud=True as well"
            assert 0 <= int(c.fused_depth_max_radius) <= 4, "SLAMConfig.fused_depth_max_radius: 0 to 4"
            assert not c.fused_depth_color or c.fused_cloud_color, \
                "SLAMConfig.fused_depth_color shows the cloud's colours: set fused_cloud_color=True as well"
        if self.config.complete_depth:
            c = self.config
            assert c.fused_depth, "SLAMConfig.complete_depth fills the holes of fused_depth's maps: set fused_depth=True as well"
            assert c.frame_depth_sink is None, \
                "SLAMConfig.complete_depth reads the frame maps again after the cloud is extracted: they must be kept (no frame_depth_sink)"
            assert c.fused_depth_sink is None, "SLAMConfig.complete_depth needs the fused maps kept (no fused_depth_sink)"
            assert 1 <= int(c.complete_depth_k) <= 8, "SLAMConfig.complete_depth_k: 1 to 8"
            assert 1 <= int(c.complete_depth_radius) <= 64, "SLAMConfig.complete_depth_radius: 1 to 64"
        self._config_tracker = sparse_tracks is None and self.config.sparse_tracks == "klt"  # then a fresh one per run
        self._resizes = None  # one `StandardResize` per view inside `run(..., native_resolution=True)`, None outside it
        # system.py:91 builds a tracker from the config; here the caller's (`track_image(frames)` per frame of pass 1,
        # `enabled`, `compute_dense_disp_target_weight` for the BA's track term) or None = the reference's dummy

    def _build_components(self, height, width, n_views, rig, camera_type):
        c = self.config
        self.buffer = GraphBuffer(height, width, n_views=n_views, buffer_size=c.buffer, init_disp=c.init_disp,
                                  cross_view_idx=c.cross_view_idx, camera_type=camera_type, device=self.device,
                                  **({"upsample_disps": True} if c.upsample_disps or c.frame_depth else {}))
        self.buffer.rig[:] = rig.data.to(self.device)
        self.buffer.sparse_tracks = self.sparse_tracks
        self.motion_filter = self.motion_filter_cls(self.droid_net, sparse_tracks=self.sparse_tracks, thresh=c.filter_thresh,
                                                    device=self.device)
        self.frontend = SLAMFrontend(self.droid_net.update, self.buffer, c.frontend, self.device)
        self.backend = SLAMBackend(self.droid_net.update, self.buffer, c.backend, self.device)
        infill = c.infill
        if c.frame_depth:  # every frame needs a disparity map of its own: pass 2 is no longer motion-only
            assert c.frame_depth_dtype in (torch.float16, torch.float32), "SLAMConfig.frame_depth_dtype: float16 or float32"
            infill = replace(c.infill, infill_dense_disp=True)
        self.inner_filler = InnerFiller(self.droid_net.update, self.buffer, infill, self.device)
        if c.upsample_disps or c.frame_depth:  # the keyframe graphs: their rows are final after the global BA
            self.frontend.graph.upsample = self.backend.upsample = True
        # InnerFiller's graph stays off under `upsample_disps` alone; with `frame_depth` it upsamples the chunk's own
        # rows - the slots behind the keyframes - in the last of its ten updates
        self.inner_filler.upsample_own_rows = bool(c.frame_depth)
        if self.metric_depth is not None:
            assert n_views == 1, "the global scale lies in the null space of a multi-view problem (system.py:115-118)"
        self.backend.depth_model = self.metric_depth

    def _precompute_features(self, frames):
        """system.py:194-218: images [V,3,H,W]; masks [V,h,w] True = INVALID (bilinear 1/8 downsample > 0.9, inverted)."""
        images = torch.stack([f.rgb for f in frames]).permute(0, 3, 1, 2).contiguous().to(self.device).float()
        masks = None
        if all(f.mask is not None for f in frames):
            ms = []
            for f in frames:
                mh, mw = f.mask.shape[0] // 8, f.mask.shape[1] // 8
                m = torch.nn.functional.interpolate(f.mask[None, None].float().to(self.device), (mh, mw), mode="bilinear")[0, 0] > 0.9
                ms.append(~m)
            masks = torch.stack(ms)
        return images, masks

    def _features(self, frames):
        """-> (images, masks, x4, disps_sens) of one time step: `_precompute_features` (x4 and disps_sens None: the
        frames are at SLAM resolution already), or with `native_resolution` the fused resize / crop of `ingest_frames`."""
        if self._resizes is None:
            return self._precompute_features(frames) + (None, None)
        images, x4, masks, disps_sens = ingest_frames(frames, self._resizes, self.device)
        return images, masks, x4, disps_sens

    def _add_keyframe(self, frame_idx, images, buffer_masks, frames, phase, reuse=None, x4=None, disps_sens=None):
        """system.py:131-165.  `reuse`: (fmap, net, inp) the motion filter has just computed for these very images.
        `x4` / `disps_sens`: what `ingest_frames` made of these frames (native resolution) - the encoders' input and the
        sensor disparities [V,h,w] of the views that carry metric depth."""
        b = self.buffer
        k = b.n_frames
        b.tstamp[k] = frame_idx
        b.images[k] = images
        if reuse is not None:
            b.fmaps[k], b.nets[k], b.inps[k] = reuse
        else:
            b.fmaps[k] = self.droid_net.encode_features(images, x4)
            b.nets[k], b.inps[k] = self.droid_net.encode_context(images, x4)
        if buffer_masks is not None:
            b.masks[k] = buffer_masks
        for v, f in enumerate(frames):
            if k == 0:
                assert f.intrinsics is not None, "the first frame must carry intrinsics"
                K = f.intrinsics.to(self.device)
                b.intrinsics[v] = K if self._resizes is None else self._resizes[v].forward_intrinsics(K)
            if f.metric_depth is not None:
                assert not self.config.backend.optimize_intrinsics
                if disps_sens is not None:  # resized, cropped, subsampled and inverted by the ingest kernel
                    b.disps_sens[k, v] = disps_sens[v]
                else:
                    d = f.metric_depth[3::8, 3::8].to(self.device)
                    b.disps_sens[k, v] = torch.where(d > 0, d.reciprocal(), d)
            if f.pose is not None and phase == 1:
                b.poses[k] = (SE3(b.rig[v]) * f.pose.inv()).data
                b.touch()  # geometry of slot k rewritten from outside: prefetched frame distances are stale
        if phase == 1:
            b.update_disps_sens(self.metric_depth, frame_idx=k)
        b.n_frames += 1

    def _run_passes(self, frames, total):
        import time
        b, mf = self.buffer, self.motion_filter
        on_gpu = torch.device(self.device).type == "cuda"
        main = torch.cuda.current_stream(self.device) if on_gpu else None
        side = None
        if on_gpu and self.config.pipeline_filter:
            side = getattr(self, "_filter_stream", None)
            if side is None or side.device != main.device:
                side = self._filter_stream = torch.cuda.Stream(device=self.device)

        def mark(name):  # phase boundaries: three stream drains per clip
            if on_gpu:
                torch.cuda.synchronize(self.device)
            self.timings[name] = time.perf_counter() - t_start

        from . import factor_graph as _fg
        work0 = dict(_fg.WORK)
        self.timings, self.work = {}, {}
        t_start = time.perf_counter()
        native = self._resizes is not None  # then x4 travels with the images: nobody runs vipe_enc_prep
        # the filter gets the `x4` keyword in native mode only: a custom `motion_filter_cls` written against
        # `check(images, masks)` / `prefetch(images, masks, stream=)` keeps working at SLAM resolution
        ready = (lambda x4: {"x4": x4}) if native else (lambda x4: {})
        nxt = self._features(frames[0])
        for frame_idx, fl in enumerate(frames):  # SLAM pass 1/2 (system.py:236-273)
            images, masks, x4, disps = nxt
            if self.sparse_tracks is not None:
                self.sparse_tracks.track_image(fl)
            # collects the prefetched first half when there is one
            kept = mf.check(images, masks, **ready(x4))
            is_keyframe = kept or frame_idx == total - 1
            if is_keyframe:  # a frame the filter kept has its features and context there already
                self._add_keyframe(frame_idx, images, masks, fl, phase=1,
                                   reuse=(mf.f_fmap, mf.f_net, mf.f_inp) if kept else None, x4=x4, disps_sens=disps)
            if frame_idx + 1 < total:
                nxt = self._features(frames[frame_idx + 1])
                if side is not None:  # frame f+1's filter runs beside keyframe f's optimisation
                    mf.prefetch(nxt[0], nxt[1], stream=side, **ready(nxt[2]))
            self.frontend.run()
            # the backend in between corrects intrinsics / extrinsics early (system.py:269-272)
            if is_keyframe and b.n_frames in self.config.frontend_backend_iters:
                self.backend.run_if_necessary(5)
        if side is not None:
            main.wait_stream(side)
        mark("pass1_seconds")
        self.work["pass1"] = {k: _fg.WORK[k] - work0[k] for k in work0}
        self.n_keyframes = int(b.n_frames)
        release = on_gpu and self.config.release_cached_memory
        lock = None
        if self.config.backend_lock_path:
            import fcntl
            lock = open(self.config.backend_lock_path, "a")
            t_wait = time.perf_counter()
            fcntl.flock(lock, fcntl.LOCK_EX)
            self.timings["backend_lock_wait_seconds"] = time.perf_counter() - t_wait
        try:
            self.backend.run(7)
            gb = self.backend.run(self.config.backend.backend_iters, update_depth=False)
            self.backend_edges = int(gb.host_edges()["ii"].shape[0])
            if self.config.disp_uncertainty:  # before pass 2 appends frames behind the keyframes
                self.marginals = gb.marginals()[:2]
            if release:
                del gb
                self.backend.last_graph = None
                torch.cuda.synchronize(self.device)
                torch.cuda.empty_cache()
        finally:
            if lock is not None:
                if on_gpu:
                    torch.cuda.synchronize(self.device)  # the next holder gets the chip and the memory, not a queue behind ours
                fcntl.flock(lock, fcntl.LOCK_UN)
                lock.close()
        mark("global_ba_done_seconds")
        self.inner_filler.set_start_idx(b.n_frames)
        # SLAM pass 2/2 (system.py:284-294): every frame appended behind the keyframes, `InnerFiller.compute` whenever
        # `infill_chunk_size` of them are there (and at the last frame).  The frames of a chunk go through the two encoders
        # in ONE batched call (per image the same arithmetic; instance norm is per image): 39 launches per chunk instead of
        # 39 per frame, and at 16 images the encoder kernels fill the chip
        chunk = max(1, int(self.config.infill.infill_chunk_size))
        pending = []  # frames appended since the last `compute`, in slot order
        kf_slot = None
        self.frame_depths = None
        if self.config.frame_depth:  # keyframe timestamp -> slot: one read-back per clip
            kf_slot = {int(t): k for k, t in enumerate(b.tstamp[:b.n_frames].tolist())}
            if self.config.frame_depth_sink is None:
                size = self._resizes[0].native_size if native else (b.height, b.width)
                self.frame_depths = torch.empty((total, b.n_views) + tuple(size), dtype=self.config.frame_depth_dtype,
                                                device=self.device)
        self.frame_depth_conf = self._kf_times = None
        if self.config.frame_depth_conf:  # the keyframes' timestamps and row flags, final from here on: one more read-back
            self._kf_times = (b.tstamp[:b.n_frames].tolist(), b.disps_up_valid[:b.n_frames].tolist())
            if self.config.frame_depth_conf_sink is None:
                size = self._resizes[0].native_size if native else (b.height, b.width)
                self.frame_depth_conf = torch.zeros((total, b.n_views) + tuple(size), dtype=torch.uint8, device=self.device)
        self._cloud = None
        if self.config.fused_cloud:  # the clip's voxel hash and the frames whose colours go into it
            from .ingest import cloud_table
            self._cloud = (cloud_table(self.config.fused_cloud_capacity, self.device), frames)
        for c0 in range(0, total, chunk):
            idx = range(c0, min(c0 + chunk, total))
            pre = [self._features(frames[i]) for i in idx]
            feats = None
            if on_gpu and len(idx) > 1:
                from .encoders import normalize_images
                imgs = torch.cat([p[0] for p in pre], 0)
                x4 = torch.cat([p[2] for p in pre], 0) if native else normalize_images(imgs)
                fmap = self.droid_net.encode_features(imgs, x4)
                net, inp = self.droid_net.encode_context(imgs, x4)
                V = pre[0][0].shape[0]
                feats = [(fmap[j * V:(j + 1) * V], net[j * V:(j + 1) * V], inp[j * V:(j + 1) * V]) for j in range(len(idx))]
            for j, i in enumerate(idx):
                self._add_keyframe(i, pre[j][0], pre[j][1], frames[i], phase=2, reuse=feats[j] if feats else None,
                                   x4=pre[j][2], disps_sens=pre[j][3])
                pending.append(i)
                if self.inner_filler.check() or i == total - 1:
                    self.inner_filler.compute()
                    if kf_slot is not None:  # the chunk's rows are valid until the next chunk reuses the slots
                        self._export_frame_depths(pending, kf_slot)
                    pending = []
        mark("pass2_done_seconds")
        self.work["total"] = {k: _fg.WORK[k] - work0[k] for k in work0}

    def _export_frame_depths(self, frame_ids, kf_slot):
        """`SLAMConfig.frame_depth`, right after `InnerFiller.compute` of the chunk `frame_ids` (consecutive frame indices,
        in the slots behind the keyframes): ONE `vipe_depth_export` launch (the views share one frame size, hence one
        `StandardResize`) turns `buffer.disps_up` rows into depth at the native size - of a frame that is a keyframe the
        KEYFRAME's row, the global BA's result (in pass 2 such a frame has only a zero-baseline edge to itself and one
        neighbour), of every other frame its own pass-2 row - into `frame_depths[frame_ids]` or, map by map in frame
        order, to the sink.  The chunk's `disps_up_valid` flags are cleared again: the slots belong to the next chunk."""
        from .._lib import upload
        from .ingest import depth_export
        b, c = self.buffer, self.config
        s, V, n = b.n_frames, b.n_views, len(frame_ids)  # `compute` has set n_frames back to the keyframes
        rows = upload([(kf_slot.get(f, s + j)) * V + v for j, f in enumerate(frame_ids) for v in range(V)], self.device)
        out = None
        if self.frame_depths is not None:
            out = self.frame_depths[frame_ids[0]:frame_ids[0] + n].view(n * V, *self.frame_depths.shape[2:])
        out = depth_export(b.flattened_disps_up, self._resizes[0] if self._resizes is not None else None, rows=rows,
                           out=out, dtype=c.frame_depth_dtype)
        conf = self._depth_confidence(frame_ids, rows) if c.frame_depth_conf else None  # reads the rows the export read
        if self._cloud is not None:
            self._fuse_cloud(frame_ids, rows, conf)
        b.disps_up_valid[s:s + n] = False
        if c.frame_depth_sink is not None:
            for j, f in enumerate(frame_ids):
                for v in range(V):
                    c.frame_depth_sink(f, v, out[j * V + v])
        if conf is not None and c.frame_depth_conf_sink is not None:
            for j, f in enumerate(frame_ids):
                for v in range(V):
                    c.frame_depth_conf_sink(f, v, conf[j * V + v])

    def _depth_confidence(self, frame_ids, rows):
        """`SLAMConfig.frame_depth_conf` for the chunk `_export_frame_depths` has just exported, before its slots are
        released: ONE `vipe_depth_consistency` launch over the same `rows` (all views), each map against the rows of
        its frame's nearest keyframes in the same view (`nearest_keyframes`: never the frame's own keyframe, never a
        keyframe without a `disps_up` row).  Neighbours are keyframes only: their rows are final during pass 2, the
        motion filter guarantees their baselines, and the result does not depend on how pass 2 is chunked.
        -> conf [n*V,H0,W0] uint8, a view of `frame_depth_conf[frame_ids]` when that is kept."""
        from .._lib import upload
        from . import ingest
        b, c = self.buffer, self.config
        V, n, K = b.n_views, len(frame_ids), int(c.frame_depth_conf_neighbours)
        kf_t, kf_ok = self._kf_times
        nbr = torch.full((n, V, K), -1, dtype=torch.int64)
        for v in range(V):
            slots = ingest.nearest_keyframes(frame_ids, kf_t, [ok[v] for ok in kf_ok], K)
            nbr[:, v] = torch.where(slots >= 0, slots * V + v, slots)
        out = None
        if self.frame_depth_conf is not None:
            out = self.frame_depth_conf[frame_ids[0]:frame_ids[0] + n].view(n * V, *self.frame_depth_conf.shape[2:])
        return ingest.depth_consistency(b.flattened_disps_up, b.poses, b.rig, b.intrinsics, b.camera_type,
                                        self._resizes[0] if self._resizes is not None else None, rows,
                                        upload(nbr.view(n * V, K), self.device), c.frame_depth_conf_tol, out=out)

    def _fuse_cloud(self, frame_ids, rows, conf):
        """`SLAMConfig.fused_cloud` for the chunk `_depth_confidence` has just rated, before its slots are released: ONE
        `vipe_cloud_fuse` launch over the same `rows`, gated by the bytes just made (whether they are kept or go to a
        sink), coloured by the chunk's frames as they were handed to `run` (stacked on the device: at the native size
        with native_resolution, at SLAM resolution otherwise - the grid of the export either way)."""
        from . import ingest
        b, c = self.buffer, self.config
        table, frames = self._cloud
        rgb = None
        if c.fused_cloud_color:
            rgb = torch.stack([fr.rgb.to(self.device) for f in frame_ids for fr in frames[f]])
            if rgb.dtype not in (torch.uint8, torch.float16, torch.float32):
                rgb = rgb.float()
        ingest.cloud_fuse(b.flattened_disps_up, b.poses, b.rig, b.intrinsics, b.camera_type,
                          self._resizes[0] if self._resizes is not None else None, rows, table, c.fused_cloud_voxel,
                          conf=conf, min_agree=c.fused_cloud_min_agree, rgb=rgb, stride=c.fused_cloud_stride)

    def _extract_cloud(self):
        """After pass 2: ONE `cloud_extract` of the clip's table -> `FusedCloud` (one sort by key; the counters' read-back)."""
        from . import ingest
        from .interface import FusedCloud
        c = self.config
        table, _ = self._cloud
        self._cloud = None
        xyz, rgb, count, key, _ = ingest.cloud_extract(table, c.fused_cloud_voxel, min_count=c.fused_cloud_min_count,
                                                       color=c.fused_cloud_color)
        return FusedCloud(xyz, rgb, count, key, c.fused_cloud_voxel, table[2].tolist())

    def _render_fused_depths(self, cloud, poses, resizes):
        """`SLAMConfig.fused_depth`, after `_extract_cloud`: the cloud drawn into every frame and view with the final
        world -> camera poses rig[v]^-1 G[f] (composed on the device), on the grid of `frame_depths` - the native size
        with native_resolution, SLAM resolution otherwise.  Per pass-2 chunk of frames ONE `cloud_render` and ONE
        `cloud_resolve` launch over a z-buffer of that chunk's images.  -> (fused_depths [T,V,H0,W0] or None when the maps
        went to `fused_depth_sink`, fused_rgb [T,V,H0,W0,3] uint8 or None)"""
        from . import ingest
        b, c = self.buffer, self.config
        V, T = b.n_views, int(poses.data.shape[0])
        cams = torch.stack([(SE3(b.rig[v][None]).inv() * poses).data for v in range(V)], dim=1).float().contiguous()  # [T,V,7]
        geom = ingest.render_params(resizes[0] if resizes is not None else (b.height, b.width))
        H0, W0 = geom[6:]
        chunk = max(1, int(c.infill.infill_chunk_size))
        rgb_points = cloud.rgb.contiguous() if c.fused_depth_color else None
        depths = rgbs = None
        if c.fused_depth_sink is None:
            depths = torch.empty((T, V, H0, W0), dtype=c.frame_depth_dtype, device=self.device)
        if c.fused_depth_color:
            rgbs = torch.empty((T, V, H0, W0, 3), dtype=torch.uint8, device=self.device)
        xyz = cloud.xyz.contiguous()
        # `SLAMConfig.complete_depth`: `run` has left the clip's frame maps in `_complete_pred`; the chunk's fused maps are
        # completed by them right after the resolve - one bits and one complete launch (`ingest.depth_complete`)
        pred, self._complete_pred, self._complete = getattr(self, "_complete_pred", None), None, None
        completes = cstats = None
        if pred is not None:
            cstats = torch.zeros(4, dtype=torch.int64, device=self.device)
            if c.complete_depth_sink is None:
                completes = torch.empty((T, V, H0, W0), dtype=c.frame_depth_dtype, device=self.device)
        for c0 in range(0, T, chunk):
            n = min(chunk, T - c0)
            zbuf = ingest.cloud_zbuffer(n * V, H0, W0, self.device)
            ingest.cloud_render(xyz, cams[c0:c0 + n].view(n * V, 7), b.intrinsics.repeat(n, 1), b.camera_type, geom, zbuf,
                                cloud.voxel, max_radius=c.fused_depth_max_radius)
            depth, rgb, _ = ingest.cloud_resolve(zbuf, rgb_points, dtype=c.frame_depth_dtype)
            if pred is not None:
                done = ingest.depth_complete(depth, pred[c0:c0 + n].view(n * V, H0, W0), K=c.complete_depth_k,
                                             radius=c.complete_depth_radius, domain="depth",
                                             wrap_x=b.camera_type == "panorama", stats=cstats,
                                             out=completes[c0:c0 + n].view(n * V, H0, W0) if completes is not None else None)[0]
                if c.complete_depth_sink is not None:
                    for j in range(n):
                        for v in range(V):
                            c.complete_depth_sink(c0 + j, v, done[j * V + v])
            if depths is not None:
                depths[c0:c0 + n] = depth.view(n, V, H0, W0)
            if rgbs is not None:
                rgbs[c0:c0 + n] = rgb.view(n, V, H0, W0, 3)
            if c.fused_depth_sink is not None:
                for j in range(n):
                    for v in range(V):
                        c.fused_depth_sink(c0 + j, v, depth[j * V + v])
        if pred is not None:  # the clip's four counters: one read-back
            self._complete = (completes, dict(zip(("affine", "scale_only", "unreached", "rejected"), cstats.tolist())))
        return depths, rgbs

    def _check_camera(self, camera_type, frames, native_resolution):
        """What a camera model rules out, before anything is built or touches the device.  The panorama
        (cameras.py:357-396) is the whole sphere on an equirectangular frame: no intrinsics (all-zero rows, as the
        reference asserts), nothing that crops, and none of the parts that are pinhole by construction."""
        from .._lib import CAMERA_CODE
        if camera_type not in CAMERA_CODE:
            raise ValueError(f"unknown camera_type {camera_type!r} (one of {sorted(CAMERA_CODE)})")
        if camera_type != "panorama":
            return
        if native_resolution:
            raise ValueError("camera_type='panorama': native_resolution crops the frame, which breaks the sphere - "
                             "resize the equirectangular frames to multiples of 8 beforehand")
        if self.sparse_tracks is not None or self._config_tracker:
            raise ValueError("camera_type='panorama': the sparse-track term is pinhole only")
        if self.config.backend.optimize_intrinsics:
            raise ValueError("camera_type='panorama': the camera has no intrinsics to optimise")
        if self.metric_depth is not None:
            raise ValueError("camera_type='panorama': depth models estimate pinhole depth; the disparities of this "
                             "camera are inverse ranges")
        if self.config.complete_depth and frames[0][0].rgb.shape[1] < 2 * int(self.config.complete_depth_radius) + 1:
            raise ValueError("camera_type='panorama' with complete_depth: the frames must be at least "
                             "2 * complete_depth_radius + 1 columns wide (the search disc may not meet itself round the seam)")
        for f in frames[0]:
            K = f.intrinsics
            if K is None or tuple(K.shape) != (4,) or bool((K != 0).any()):
                raise ValueError("camera_type='panorama': frames carry all-zero [4] intrinsics (cameras.py:360)")

    @torch.no_grad()
    def run(self, frames, rig=None, camera_type="pinhole", native_resolution=False):
        """frames: sequence (length T) of per-view lists of `Frame` (a single `Frame` per step for one view).

        camera_type: "pinhole", "mei" or "panorama" (the reference's `CameraType` values).  A panorama clip is
        equirectangular frames with all-zero `[4]` intrinsics; disparities are then inverse ranges (`Frame.metric_depth`,
        if given, is the range), and `native_resolution`, a sparse tracker, `backend.optimize_intrinsics` and a depth
        model are rejected (`ValueError`) before anything runs.  `SLAMMap.project_map` stays a pinhole target.

        native_resolution=False: the frames are at SLAM resolution already (sides multiples of 8) and the returned
        intrinsics are at that resolution.  True: frames of any size, as decoded - every view goes through the
        reference's `StandardResizeStreamProcessor` step (system.py:42-77, 215-218: bilinear resize to an area of about
        384 x 512, centre crop to multiples of 8; `ingest_frames`, one fused kernel per view), `Frame.intrinsics` are
        given at the native size and `SLAMOutput.intrinsics` come back recovered to it (system.py:306-309).  A
        `sparse_tracks` tracker is handed the frames as they came (`track_image`), while the reference's sees the
        resized, cropped ones: in native mode its `observations` must be in `StandardResize(...).out_size` pixel
        coordinates (resize its input, or map its tracks with `forward_intrinsics`' scale and crop) - not converted here.
        A tracker with `accepts_resize` (`KLTSparseTracks`) is handed the per-view `StandardResize` (`set_resize`) and
        does that mapping itself.

        With `SLAMConfig.upsample_disps` the output carries `keyframe_disps_up` [N_kf,V,H,W] and
        `keyframe_disps_up_valid` [N_kf,V] (aligned with `keyframe_ids`), at SLAM resolution: with native_resolution=True
        that is the resized and cropped size (`StandardResize(...).out_size`), not the native one.

        With `SLAMConfig.disp_uncertainty` it carries `keyframe_disp_var` [N_kf,V,h,w] (the BA's 1/8 grid) and
        `keyframe_pose_cov` [N_kf,6,6]: marginal covariances of the last global BA's damped, weighted linear system at the
        final keyframe state (`GraphBuffer.ba_marginals`), NaN where a frame / pose was not free (the gauge keyframe's
        pose).  `run` applies no metric rescaling; a caller that rescales the result by a factor s (disparities / s,
        translations * s) passes the two fields through `interface.rescale_marginals`.

        With `SLAMConfig.frame_depth` it carries `frame_depths` [T,V,H0,W0] (`frame_depth_dtype`, fp16 by default): one
        depth map per frame and view, at the native size with native_resolution=True and at SLAM resolution otherwise - or
        hands every map to `SLAMConfig.frame_depth_sink` as pass 2's chunks complete and leaves the field None - and
        `frame_disps_lowres` [T,V,h,w], pass 2's 1/8-grid disparities.  Depth is the reciprocal of the camera model's
        disparity: for camera_type="panorama" the maps are RANGES along the ray, not z.  This changes pass 2 from
        motion-only to poses and disparities (`infill_dense_disp` forced on), and `keyframe_disps_up` comes with it.  Units
        are the trajectory's; no metric rescaling here (`interface.rescale_frame_depths`).

        With `SLAMConfig.frame_depth_conf` on top of it, `frame_depth_conf` [T,V,H0,W0] uint8 lies pixel for pixel beside
        `frame_depths` (or every map goes to `SLAMConfig.frame_depth_conf_sink`): how many of the frame's nearest
        keyframes of the same view see the pixel's point (high nibble) and how many of those confirm its depth within
        `frame_depth_conf_tol` (low nibble; `interface.unpack_depth_conf`).  It only reads: depths and trajectory are
        what they are without it.

        With `SLAMConfig.fused_cloud` on top of both, `fused_cloud` is an `interface.FusedCloud`: every pixel of those
        maps that at least `fused_cloud_min_agree` keyframes confirm, back-projected to the world and merged per voxel of
        `fused_cloud_voxel` (centroid, mean colour of the frames' `rgb`, count), voxels with fewer than
        `fused_cloud_min_count` points left out, sorted by voxel key.  The table has `fused_cloud_capacity` slots and does
        not grow: `fused_cloud.stats` counts what it dropped.  It only reads as well.

        With `SLAMConfig.fused_depth` on top of that, `fused_depths` [T,V,H0,W0] (`frame_depth_dtype`) lies pixel for pixel
        beside `frame_depths`: that cloud drawn back into every frame and view with the final poses (`FusedCloud.render`'s
        rule: the nearest point whose footprint covers the pixel, 0 where none does) - one surface for the whole clip,
        gated by confidence already - and with `fused_depth_color` `fused_rgb` [T,V,H0,W0,3] uint8; or every map goes to
        `SLAMConfig.fused_depth_sink` and `fused_depths` stays None.  It only reads.

        With `SLAMConfig.complete_depth` on top of that, `complete_depths` [T,V,H0,W0] (`frame_depth_dtype`) is the
        hole-free form of those maps: `fused_depths` bit for bit where they are positive (and the frame has a depth
        there: both are needed to anchor a fit); elsewhere the frame's own
        `frame_depths` value, scaled and shifted (in the disparity domain) to agree with the `complete_depth_k` nearest
        fused pixels within `complete_depth_radius`; 0 only where no fused pixel is in reach or the frame has no depth.
        `complete_depth_stats` counts the filled pixels by kind.  Or every map goes to `SLAMConfig.complete_depth_sink`
        and `complete_depths` stays None.  For the panorama the columns are a circle and the frames must be at least
        2 * `complete_depth_radius` + 1 wide (`ValueError`).  It only reads."""
        frames = [f if isinstance(f, (list, tuple)) else [f] for f in frames]
        total, n_views = len(frames), len(frames[0])
        assert total > 0 and all(len(f) == n_views for f in frames)
        if rig is None:
            assert n_views == 1, "Need rig for multiple views"
            rig = SE3.Identity(1)
        height, width = frames[0][0].rgb.shape[:2]
        self._check_camera(camera_type, frames, native_resolution)
        resizes = None
        if native_resolution:
            for f in frames[0]:  # system.py:222-223
                assert tuple(f.rgb.shape[:2]) == (height, width), "all views must share one frame size"
            resizes = [StandardResize(height, width) for _ in range(n_views)]
            height, width = resizes[0].out_size
        if self._config_tracker:
            from .sparse_tracks import KLTSparseTracks
            self.sparse_tracks = KLTSparseTracks(n_views, device=self.device)
        if resizes is not None and getattr(self.sparse_tracks, "accepts_resize", False):
            self.sparse_tracks.set_resize(resizes)  # it tracks at the native size and reports at `out_size`
        self.config.frontend.has_init_pose = frames[0][0].pose is not None
        self._build_components(height, width, n_views, rig, camera_type)
        b = self.buffer
        import gc
        gc_was = self.config.pause_gc and gc.isenabled()
        if gc_was:
            gc.collect()
            gc.disable()
        self._resizes = resizes  # read by `_features`, `_add_keyframe` and `_run_passes`, for the two passes only
        try:
            self._run_passes(frames, total)
        finally:
            self._resizes = None
            if gc_was:
                gc.enable()
        filled = self.inner_filler.get_result()
        if filled.poses.data.shape[0] != total:
            raise ValueError("fewer poses than frames: the frame sequence changed between the passes")
        slam_map = b.extract_slam_map(filter_thresh=self.config.map_filter_thresh)
        intrinsics = b.intrinsics.clone()
        if resizes is not None:
            intrinsics = torch.stack([r.recover_intrinsics(intrinsics[v]) for v, r in enumerate(resizes)])
        up = {}
        if b.disps_up is not None:  # slots [0, n_frames) are the keyframes again (InnerFiller.compute), in keyframe_ids' order
            up = dict(keyframe_disps_up=b.disps_up[:b.n_frames].clone(),
                      keyframe_disps_up_valid=b.disps_up_valid[:b.n_frames].clone())
        if self.config.disp_uncertainty:  # rows by keyframe slot, i.e. in keyframe_ids' order
            n_kf, V = self.n_keyframes, b.n_views
            disp_var, pose_cov = self.marginals
            up.update(keyframe_disp_var=disp_var[:n_kf * V].view(n_kf, V, *disp_var.shape[1:]).clone(),
                      keyframe_pose_cov=pose_cov[:n_kf].clone())
        if self.config.frame_depth:
            up.update(frame_depths=self.frame_depths, frame_disps_lowres=filled.dense_disps)
            self.frame_depths = None
        if self.config.frame_depth_conf:
            up.update(frame_depth_conf=self.frame_depth_conf)
            self.frame_depth_conf = None
        if self.config.fused_cloud:
            up.update(fused_cloud=self._extract_cloud())
        if self.config.fused_depth:
            if self.config.complete_depth:
                self._complete_pred = up["frame_depths"]
            fused_depths, fused_rgb = self._render_fused_depths(up["fused_cloud"], filled.poses, resizes)
            up.update(fused_depths=fused_depths, fused_rgb=fused_rgb)
            if self.config.complete_depth:
                (complete_depths, complete_stats), self._complete = self._complete, None
                up.update(complete_depths=complete_depths, complete_depth_stats=complete_stats)
        return SLAMOutput(trajectory=filled.poses.inv(), intrinsics=intrinsics, rig=SE3(b.rig.clone()), slam_map=slam_map, **up)
