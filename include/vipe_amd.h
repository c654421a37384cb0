/*
 * vipe_amd.h - C ABI of libvipe_amd.so, the MI355X (gfx950) backend for the ViPE dense-SLAM
 * update iteration.  One entry point per function the reference binds through pybind11 in
 * csrc/bind.cpp:28-49 (submodules droid_net_ext, slam_ext, lietorch_ext, scatter_ext, corr_ext),
 * plus the fused entry points the MI355X-first design adds (marked [fused]).
 *
 * Conventions
 *   - every pointer named d_* is DEVICE memory (hipMalloc / torch CUDA tensor .data_ptr());
 *     h_* is host memory.  All tensors are contiguous row-major with the shapes given.
 *   - `stream` is a hipStream_t (pass torch.cuda.current_stream().cuda_stream; 0 = null stream).
 *     Nothing here synchronises the host, allocates device memory or copies D2H: callers pass
 *     workspaces (sizes from the *_workspace_bytes functions), so every call is graph-capturable.
 *   - return value: 0 on success, a negative VIPE_E* code on argument errors (no launch made),
 *     or a positive hipError_t if a launch failed.
 *   - dtype codes: VIPE_F16 / VIPE_F32 / VIPE_F64 (the reference's AT_DISPATCH_FLOATING_TYPES_AND_HALF).
 */
#ifndef VIPE_AMD_H
#define VIPE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIPE_F16 0
#define VIPE_F32 1
#define VIPE_F64 2
#define VIPE_U8 3 /* decoded 8-bit frames (vipe_frame_ingest only) */

#define VIPE_OK 0
#define VIPE_EINVAL (-1)   /* bad shape / null pointer / unsupported dtype */
#define VIPE_ENOSPACE (-2) /* workspace too small */
#define VIPE_EUNSUPPORTED (-3)

/* storage layout of a correlation pyramid (level i of an edge b, source pixel p1 = y1 * w + x1, target (y, x)):
 *   REFERENCE  level i = [B][h*w][h>>i][w>>i] for every level - CorrBlock.corr_pyramid, droid_net.py:56-69.
 *   BLOCKED    levels 0 and 1 regrouped into 64-byte tiles of 4 rows x 8 columns and 16 KiB / 8 KiB runs per 64
 *              source pixels, on the grid PADDED to G = ceil(h w / 64) groups of source pixels, S = ceil(w / 32) strips
 *              of 32 target columns and R = 2 ceil(h / 8) groups of 4 target rows (vipe_corr_blocked_dims):
 *                level0[b][p1/64][(x/32)*R     + y/4][p1%64][(x%32)/8][y%4][x%8]
 *                level1[b][p1/64][(x/16)*(R/2) + y/4][p1%64][(x%16)/8][y%4][x%8]     (x, y level-1 coordinates)
 *                level2[b][G*64][R][8 S]      level3[b][G*64][R/2][round_up(4 S, 8)]  (one slab per source pixel)
 *              For w % 64 == 0, h % 8 == 0 (the DROID maps at 1/8 of 512 x 384 and multiples) nothing is padded: the
 *              same bytes per level as REFERENCE, levels 2 / 3 ARE the reference's.  For every other grid (41 x 73 for
 *              16:9 video, vipe/slam/system.py:46-59) tiles wholly outside the h x w targets are never written or read,
 *              and entries outside the floored (h >> i) x (w >> i) level (droid_net.py:66-68) hold zero.  The internal
 *              layout of pooled pyramids: built by vipe_corr_pyramid_build_indexed / _prepared, read by
 *              vipe_corr_lookup_conv1x1. */
#define VIPE_PYRAMID_REFERENCE 0
#define VIPE_PYRAMID_BLOCKED 1

#define VIPE_CAM_PINHOLE 0 /* vipe/utils/cameras.py:123 */
#define VIPE_CAM_MEI 1     /* vipe/utils/cameras.py:220 */
#define VIPE_CAM_PANORAMA 2 /* CameraType.PANORAMA, vipe/utils/cameras.py:357-396: 360-degree equirectangular grid, pixel-centre
                               convention u_n = (u + 0.5) / wd; disparity is inverse RANGE; no intrinsics (the [V,4] row is all
                               zero and never read, though the pointer is checked like any other; optimize_intrinsics with it is VIPE_EINVAL).  The reference defines the rays
                               (iproj_disp, :366-387) and the projection (vipe/utils/geometry.py:89-120) but no proj_points; the
                               Jacobian, the validity rule (range > 0.1, 1e-3 off the poles) and the wrapping of horizontal
                               differences at the seam are stated in csrc/camera.cuh. */

/* library / build identification ("gfx950", ABI version) */
const char* vipe_amd_version(void);
int vipe_amd_abi_version(void); /* 4 since round 4 (vipe_corr_pyramid_build_prepared.n_prepared, slot-indexed operator state); 3: vipe_ba_params.solver_options; rounds 1-2: 1, 2 */

/* ---------------------------------------------------------------------------------------------
 * droid_net_ext  (csrc/droid_net_ext/droid.cpp:57-63)
 * ------------------------------------------------------------------------------------------- */

/* corr_index_forward: replaces corr_index_cuda_forward, correlation_kernels.cu:115-136.
 * volume [B,h1,w1,h2,w2] dtype; coords [B,2,h1,w1] f32; corr [B,2r+1,2r+1,h1,w1] dtype (fully written). */
int vipe_corr_index_forward(const void* d_volume, const float* d_coords, void* d_corr, int B, int h1, int w1,
                            int h2, int w2, int radius, int dtype, void* stream);

/* corr_index_backward: replaces corr_index_cuda_backward, correlation_kernels.cu:138-159.
 * corr_grad [B,2r+1,2r+1,h1,w1]; volume_grad [B,h1,w1,h2,w2] (fully written, zero outside the windows). */
int vipe_corr_index_backward(const float* d_coords, const void* d_corr_grad, void* d_volume_grad, int B, int h1,
                             int w1, int h2, int w2, int radius, int dtype, void* stream);

/* [fused] CorrBlock.__call__ (droid_net.py:71-82): all pyramid levels in one launch.
 * h_levels: host array of num_levels device pointers, level i is [B,h1,w1,h2>>i,w2>>i];
 * coords [B,h1,w1,2] f32 (level i uses coords / 2^i); out [B,num_levels*(2r+1)^2,h1,w1]. */
int vipe_corr_pyramid_lookup(const void* const* h_levels, const float* d_coords, void* d_out, int B, int h1, int w1,
                             int h2, int w2, int num_levels, int radius, int dtype, void* stream);

/* [fused] same lookup written channels-last for the flow-update operator: out [B,h1,w1,channel_stride],
 * channel = level*(2r+1)^2 + x_off*(2r+1) + y_off, channels beyond num_levels*(2r+1)^2 zero filled. */
int vipe_corr_pyramid_lookup_nhwc(const void* const* h_levels, const float* d_coords, void* d_out, int B, int h1,
                                  int w1, int h2, int w2, int num_levels, int radius, int dtype, int channel_stride,
                                  void* stream);

/* [fused] 4-level radius-3 lookup (droid_net.py:71-82) + the correlation encoder's first layer, Conv2d(196, Cout, 1)
 * + bias + activation (droid_net.py:436-437, 481): out[B,h1,w1,out_ctot] channels [out_coff, out_coff+Cout) fp16.
 * d_w_packed / d_bias as produced by vipe_conv_pack_weights for a [Cout, 200, 1, 1] weight (196 + 4 zero inputs); d_bias
 * readable up to the padded output-channel count of vipe_conv_packed_dims, values behind Cout ignored.
 * fp16 volume levels, Cout == 128; other configurations return VIPE_EUNSUPPORTED (use lookup_nhwc + conv2d).
 * d_slots (optional, [B] int32): edge b reads slot d_slots[b] of the level buffers (a pool of pyramids with capacity
 * >= B whose edges come and go without compaction, factor_graph.py:147-152,194-196); null: slot b.
 * layout: VIPE_PYRAMID_REFERENCE (level widths multiples of 8 down to level 3) or VIPE_PYRAMID_BLOCKED (h1 == h2,
 * w1 == w2; any grid with h, w >= 8). */
int vipe_corr_lookup_conv1x1(const void* const* h_levels, const float* d_coords, const void* d_w_packed,
                             const float* d_bias, void* d_out, int out_ctot, int out_coff, int B, int h1, int w1,
                             int h2, int w2, int Cout, int act, const int* d_slots, int layout, void* stream);

/* [fused] the same with its launch chosen by the caller; vipe_corr_lookup_conv1x1 is this with (0, 0).  The kernel runs
 * as persistent workgroups that each take half a compute unit (registers and LDS).
 * share_cu 0: two per compute unit, for a launch that has the device to itself.  share_cu 1: at most one becomes
 * resident per compute unit, so that kernels of another stream run in the other half while the lookup waits on memory
 * (vipe_update_operator with a side stream).  max_workgroups > 0 caps the grid (each workgroup then walks more pixel
 * groups); 0: no cap.  The output does not depend on either. */
int vipe_corr_lookup_conv1x1_ex(const void* const* h_levels, const float* d_coords, const void* d_w_packed,
                                const float* d_bias, void* d_out, int out_ctot, int out_coff, int B, int h1, int w1,
                                int h2, int w2, int Cout, int act, const int* d_slots, int layout, void* stream,
                                int max_workgroups, int share_cu);

/* [fused] CorrBlock.corr + pyramid (droid_net.py:56-69,94-102): volume = (f1/4)^T (f2/4) on MFMA (fp16 in,
 * fp32 accumulate, stored as dtype), then 2x2 average pooling of the target dims for levels 1..num_levels-1.
 * fmap1, fmap2 [B,C,h,w] f16; h_levels: host array of num_levels device pointers (outputs). C % 32 == 0. */
int vipe_corr_pyramid_build(const void* d_fmap1, const void* d_fmap2, void* const* h_levels, int B, int C, int h,
                            int w, int num_levels, void* stream);

/* [fused] the same for the edges of a factor graph, straight from the keyframe buffer into a pooled store
 * (factor_graph.py:147-152: `CorrBlock(fmaps[ii], fmaps[jj])` then `corr.cat`): edge b correlates frame d_idx1[b]
 * with frame d_idx2[b] of d_fmaps [n_frames,C,h,w] f16 - the gathered [B,C,h,w] copies never exist - and is written
 * to slot d_slots[b] of the level buffers (null: slot b) in `layout` (VIPE_PYRAMID_*). */
int vipe_corr_pyramid_build_indexed(const void* d_fmaps, const int64_t* d_idx1, const int64_t* d_idx2,
                                    const int* d_slots, void* const* h_levels, int B, int C, int h, int w,
                                    int num_levels, int layout, void* stream);

/* [fused] the same for ANY grid (C == 128): the keyframes' maps are first rewritten, once per frame, into the zero-padded
 * operand images the MFMA kernel loads with aligned 16-byte accesses (an h x w map with an odd pixel count has no
 * aligned rows):  vipe_corr_prep(d_fmaps [n,C,h,w] f16 -> d_prep [n][vipe_corr_prep_halves(C,h,w)] f16), then
 * vipe_corr_pyramid_build_prepared with frame indices d_idx1 / d_idx2 counted from `frame_base` (d_prep holds frames
 * frame_base .. frame_base + n_prepared - 1 of the keyframe buffer; an edge one of whose frames lies outside that range
 * is SKIPPED - its slot keeps its old contents - instead of reading outside d_prep).  Output: VIPE_PYRAMID_BLOCKED on the padded grid.
 * vipe_corr_blocked_dims: dims6 = {G, S, R, level-2 row pitch, level-3 row pitch, 1 if vipe_corr_pyramid_build_indexed
 * tiles this grid directly (no preparation needed) else 0}. */
int vipe_corr_blocked_dims(int h, int w, int* dims6);
int64_t vipe_corr_prep_halves(int C, int h, int w);
int vipe_corr_prep(const void* d_fmaps, void* d_prep, int n, int C, int h, int w, void* stream);
int vipe_corr_pyramid_build_prepared(const void* d_prep, int64_t frame_base, int64_t n_prepared, const int64_t* d_idx1, const int64_t* d_idx2,
                                     const int* d_slots, void* const* h_levels, int B, int C, int h, int w, int num_levels,
                                     void* stream);

/* CorrBlock.corr for any dtype / channel count (droid_net.py:94-102): volume[b][p1][p2] = sum_c (f1[b][c][p1] / 4)
 * (f2[b][c][p2] / 4); fmaps [B,C,P] dtype, volume [B,P,P] dtype (plain tiled kernel: what the MFMA kernel of
 * vipe_corr_pyramid_build does not take).  vipe_avg_pool2x2: F.avg_pool2d(x, 2, stride=2) over the last two dims of
 * [n,h,w] -> [n,h>>1,w>>1] (droid_net.py:66-68), at::native rounding. */
int vipe_corr_volume(const void* d_fmap1, const void* d_fmap2, void* d_volume, int B, int C, int P, int dtype, void* stream);
int vipe_avg_pool2x2(const void* d_x, void* d_y, int64_t n, int h, int w, int dtype, void* stream);

/* altcorr_forward: replaces altcorr_cuda_forward, altcorr_kernel.cu:266-290.
 * fmap1 [B,H1,W1,C], fmap2 [B,H2,W2,C] dtype (f16/f32); coords [B,N,H1,W1,2] f32; corr [B,N,(2r+1)^2,H1,W1]. */
int vipe_altcorr_forward(const void* d_fmap1, const void* d_fmap2, const float* d_coords, void* d_corr, int B,
                         int H1, int W1, int H2, int W2, int N, int C, int radius, int dtype, void* stream);

/* altcorr_backward: replaces altcorr_cuda_backward, altcorr_kernel.cu:292-320 (float32 only).
 * fmap1_grad / fmap2_grad are accumulated into (caller zero-initialises), coords receive no gradient. */
int vipe_altcorr_backward(const float* d_fmap1, const float* d_fmap2, const float* d_coords,
                          const float* d_corr_grad, float* d_fmap1_grad, float* d_fmap2_grad, int B, int H1, int W1,
                          int H2, int W2, int N, int C, int radius, void* stream);

/* ---------------------------------------------------------------------------------------------
 * lietorch_ext  (csrc/lietorch_ext/lietorch.cpp:305-336).  group_id 1=SO3 2=RxSO3 3=SE3 4=Sim3
 * (dispatch.h:18-40); dtype VIPE_F32 / VIPE_F64.  `on_device` 0 runs the same closed forms on the
 * host (the reference's lietorch_cpu.cpp path), 1 launches on `stream`.
 * Rows: X [n,N] (N = 4,5,7,8), tangent a [n,K] (K = 3,4,6,7).
 * ------------------------------------------------------------------------------------------- */
int vipe_lie_expm(int group_id, const void* a, void* X, int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_logm(int group_id, const void* X, void* a, int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_inv(int group_id, const void* X, void* Y, int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_mul(int group_id, const void* X, const void* Y, void* Z, int64_t n, int dtype, int on_device,
                 void* stream);
int vipe_lie_adj(int group_id, const void* X, const void* a, void* b, int64_t n, int dtype, int on_device,
                 void* stream);
int vipe_lie_adjT(int group_id, const void* X, const void* a, void* b, int64_t n, int dtype, int on_device,
                  void* stream);
int vipe_lie_act(int group_id, const void* X, const void* p, void* q, int64_t n, int dtype, int on_device,
                 void* stream); /* p,q [n,3] */
int vipe_lie_act4(int group_id, const void* X, const void* p, void* q, int64_t n, int dtype, int on_device,
                  void* stream); /* p,q [n,4] */
int vipe_lie_as_matrix(int group_id, const void* X, void* T, int64_t n, int dtype, int on_device,
                       void* stream); /* T [n,4,4] */
int vipe_lie_projector(int group_id, const void* X, void* P, int64_t n, int dtype, int on_device,
                       void* stream); /* P [n,N,N] */
int vipe_lie_jinv(int group_id, const void* X, const void* a, void* b, int64_t n, int dtype, int on_device,
                  void* stream);
/* [fused] the keyframe frontend's preparation of the NEXT frame's slot (vipe/slam/components/frontend.py:70-76 `_init_pose`,
 * :118-122 / :147-151): poses[t1] = Exp(0.5 Log(G_{t1-1} G_{t1-2}^-1)) G_{t1-1} when init_pose, and disps[t1, v] =
 * mean(disps[t1 - n_mean .. t1 - 1, v]) for every view.  poses [>= t1+1, 7], disps [>= t1+1, n_views, P] f32. */
int vipe_frontend_next_frame(float* d_poses, float* d_disps, int t1, int n_views, int P, int n_mean, int init_pose,
                             void* stream);
/* [fused] broadcast forms: one group element per `rows_per_elem` consecutive rows of a/p (the Python
 * wrapper in the reference replicates X per row, broadcasting.py:32-35). */
int vipe_lie_adjT_bcast(int group_id, const void* X, const void* a, void* b, int64_t n_elem, int64_t rows_per_elem,
                        int dtype, void* stream);
int vipe_lie_act4_bcast(int group_id, const void* X, const void* p, void* q, int64_t n_elem, int64_t rows_per_elem,
                        int dtype, void* stream);
/* backward passes (lietorch.cpp:317-331): grad wrt the op's inputs */
int vipe_lie_expm_backward(int group_id, const void* grad, const void* a, void* da, int64_t n, int dtype,
                           int on_device, void* stream);
int vipe_lie_logm_backward(int group_id, const void* grad, const void* X, void* dX, int64_t n, int dtype,
                           int on_device, void* stream);
int vipe_lie_inv_backward(int group_id, const void* grad, const void* X, void* dX, int64_t n, int dtype,
                          int on_device, void* stream);
int vipe_lie_mul_backward(int group_id, const void* grad, const void* X, const void* Y, void* dX, void* dY,
                          int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_adj_backward(int group_id, const void* grad, const void* X, const void* a, void* dX, void* da,
                          int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_adjT_backward(int group_id, const void* grad, const void* X, const void* a, void* dX, void* da,
                           int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_act_backward(int group_id, const void* grad, const void* X, const void* p, void* dX, void* dp,
                          int64_t n, int dtype, int on_device, void* stream);
int vipe_lie_act4_backward(int group_id, const void* grad, const void* X, const void* p, void* dX, void* dp,
                           int64_t n, int dtype, int on_device, void* stream);

/* ---------------------------------------------------------------------------------------------
 * slam_ext  (csrc/slam_ext/slam.cpp:31-37) and the live dense BA it stands behind
 * ------------------------------------------------------------------------------------------- */

/* [fused] GraphBuffer.reproject_dense_disp (buffer.py:527-548 -> geom.py:187-263, jacobian=False).
 * poses [n_poses,7] world->cam; disps [n_poses*V,ht,wd]; intrinsics [V,4+D] FULL-RES (scaled by
 * 1/intr_factor inside, terms.py:182); rig [V,7]; pi,qi,pj,qj,di [M] int64 (expand_edge_multiview).
 * coords [M,ht,wd,2], valid [M,ht,wd] f32 (valid may be NULL). */
int vipe_reproject(const float* d_poses, const float* d_disps, const float* d_intrinsics, const float* d_rig,
                   const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj, const int64_t* d_qj,
                   const int64_t* d_di, float* d_coords, float* d_valid, int M, int ht, int wd, int n_views,
                   int camera, float intr_factor, void* stream);

/* [fused] FactorGraph.update motion features (factor_graph.py:253-261): coords1 = reproject(ii,jj) and
 * motn = clamp(cat[coords1 - grid, target - coords1], +-64) written as [M,4,ht,wd] in `motn_dtype`. */
int vipe_reproject_motion(const float* d_poses, const float* d_disps, const float* d_intrinsics, const float* d_rig,
                          const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj, const int64_t* d_qj,
                          const int64_t* d_di, const float* d_target, float* d_coords, void* d_motn, int M, int ht,
                          int wd, int n_views, int camera, float intr_factor, int motn_dtype, void* stream);
/* same with motn written channels-last [M,ht,wd,4] fp16 (the layout the MFMA convolutions read) */
int vipe_reproject_motion_nhwc(const float* d_poses, const float* d_disps, const float* d_intrinsics,
                               const float* d_rig, const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj,
                               const int64_t* d_qj, const int64_t* d_di, const float* d_target, float* d_coords,
                               void* d_motn, int M, int ht, int wd, int n_views, int camera, float intr_factor,
                               void* stream);

/* Dense bundle adjustment with the LIVE semantics of GraphBuffer.bundle_adjustment (buffer.py:373-525,
 * solver.py:117-197, terms.py:94-303): Gauss-Newton on SE3 (+) per-pixel inverse depth (+ optional
 * focal/distortion), Schur reduction over the depths, dense block Cholesky (fp64) of the reduced system,
 * back-substitution and retraction, n_iters times, entirely on `stream`.
 *   poses [n_poses,7] (updated in place), disps [n_poses*V,ht,wd] (in place; finally clamped >= 1e-3 over
 *   all n_disp_frames), disps_sens like disps, intrinsics [V,4+D] (in place when optimize_intrinsics),
 *   rig [V,7], target/weight [M,ht*wd,2], disp_damping [n_poses*V,ht,wd] (GraphAgg eta),
 *   pi,qi,pj,qj,di [M] int64.  Pose p is fixed iff it occurs in pi and (p < t0 or p >= t1)
 *   (buffer.py:462-465); t0 == t1 fixes every pose.
 *   d_workspace: vipe_dense_ba_workspace_bytes(...) bytes, contents need not be initialised.
 *   d_info (optional, 8 ints): [n_free_poses, n_free_disp_frames, cholesky_failures, n_regular_unknowns,
 *   band width in 6x6 blocks, the solver of the last iteration (0 global-memory Cholesky, also when nothing was solved;
 *   1 LDS band solver; 2 LDS dense solver), largest source-frame degree, 1 if a pivot of the last tiled factorisation
 *   failed]. */
/* Co-scheduling hook of vipe_dense_ba (optional).  Most of a Gauss-Newton iteration is the reduced-system solve: ONE
 * workgroup busy on a 256-CU part.  A caller with independent work (FactorGraph.update: the hidden-state part of the next
 * iteration's GRU gates, vipe_update_gate_state_piece) hands it over in `n_pieces = max(n_iters, 1)` pieces: piece k is
 * enqueued on `overlap_stream` behind an event recorded after iteration k's accumulate kernels and a few microseconds
 * of delay, i.e. it starts once the solve of iteration k owns its CU and fills the other 255.  overlap_fn is called on
 * the host, from inside vipe_dense_ba, exactly n_pieces times (also when the BA has nothing to do); it must only enqueue
 * work on the stream it is given and return VIPE_OK.  The caller orders overlap_stream after its producers before the
 * call and joins it afterwards. */
typedef int (*vipe_overlap_fn)(void* user, int piece, int n_pieces, void* stream);

typedef struct {
  int n_poses;       /* rows of poses; disps has n_poses*n_views frames */
  int n_views;
  int ht, wd;
  int M;             /* number of terms (edges * views) */
  int t0, t1;
  int n_iters;
  float pose_damping, pose_ep;
  int motion_only;
  int limited_disp;
  int optimize_intrinsics;
  int optimize_rig_rotation; /* rotation-only blocks for the views >= 1 of a rig (view 0 is always fixed, buffer.py:497-506,
                                retractor.py:32-37); no effect for n_views == 1.  Rigs of up to 8 views. */
  int camera;        /* VIPE_CAM_* */
  float alpha;       /* ba.dense_disp_alpha, configs/slam/default.yaml:48-49 */
  float weight_scale;/* 0.001, buffer.py:396 */
  float intr_factor; /* 8.0, buffer.py:415 */
  int reuse_plan;    /* 1: the workspace still holds the plan (term order, pose slots, band, flags) of the previous
                        call with IDENTICAL index arrays and parameters - skip rebuilding it.  The caller owns that
                        guarantee (same workspace, nothing else ran in it); everything data dependent (sensor-depth
                        frames, damping) is re-read every call. */
  int path_hint;     /* 0: unknown - every kernel of both accumulate / solve paths is launched and the inapplicable ones
                        exit at once (the choice depends on the plan, which lives on the device).  A caller that has read
                        d_info[4..7] of an earlier call with the SAME plan may pass what it learnt so that those launches are
                        not made: bit 0 source degree <= 6 (matrix-core accumulate), bit 1 degree > 6 (walk + Schur),
                        bit 2 an LDS solver takes the system (the global-memory Cholesky is not launched), bit 3 the LDS
                        band solver does not take it, bit 4 the LDS dense solver does not take it. */
  void* overlap_stream;        /* co-scheduling hook (see vipe_overlap_fn); NULL / NULL: none */
  vipe_overlap_fn overlap_fn;
  void* overlap_user;
  int solver_options;          /* 0 = the default kernel selection.  VIPE_BA_OPT_* bits pick the equivalent general forms, for
                                  validating the specialised kernels against them (tests/test_gpu_parity.py) */
  void* profile_ev0;           /* optional pair of hipEvent_t (created with timing enabled by the caller): recorded on the BA */
  void* profile_ev1;           /* stream right before / right after the accumulate kernels (ba_accum_mfma_kernel, or the walk +
                                  Schur pair) of Gauss-Newton iteration `profile_iter` - bench.py times that launch with them;
                                  NULL: none */
  int profile_iter;            /* 0 .. n_iters - 1; negative: the last iteration */
} vipe_ba_params;
#define VIPE_BA_OPT_ONE_CHAIN 1           /* band solve: eliminate the pose chain from one end (default: both ends at once) */
#define VIPE_BA_OPT_GENERAL_ACCUMULATE 2  /* accumulate: the walk + Schur kernel pair for every source-frame degree */

int64_t vipe_dense_ba_workspace_bytes(const vipe_ba_params* p);
int vipe_dense_ba(const vipe_ba_params* p, float* d_poses, float* d_disps, const float* d_disps_sens,
                  float* d_intrinsics, float* d_rig, const float* d_target, const float* d_weight,
                  const float* d_disp_damping, const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj,
                  const int64_t* d_qj, const int64_t* d_di, void* d_workspace, int64_t workspace_bytes,
                  int* d_info, void* stream);

/* Marginal covariances of the damped, weighted linear system ONE Gauss-Newton iteration of vipe_dense_ba would solve at
 * the given state: H = [[B, E], [E^T, C]] with C diagonal (per-pixel disparities), S = B - E C^-1 E^T.  The network's
 * confidence weights act as inverse variances; there is no noise scale.  Two calls, with the caller's inverse of S between
 * them (an n x n factorisation, n <= 6 n_poses + tail; the library does not invert):
 *
 * vipe_dense_ba_linearize: the plan, the sensor-prior test and the accumulate kernels of one iteration (reuse_plan,
 *   path_hint and solver_options as in vipe_dense_ba; n_iters is ignored), no solve, no retraction: poses / disps /
 *   intrinsics / rig are only read.  d_S_out [>= n, ld_out] fp64, ld_out >= 6 n_poses + tail: the symmetric reduced system
 *   WITH the Levenberg-Marquardt damping of the pose / intrinsics / rig rows, n = d_info[3] rows and columns written.
 *   The workspace then holds the per-pixel blocks the marginals read; nothing else may run in it before
 *   vipe_dense_ba_marginals has.
 * vipe_dense_ba_marginals: p and d_workspace of that linearize call, d_Sinv [n, ld] fp64 = S^-1, full symmetric
 *   (NULL with ld = 0 when n = 0).
 *   d_disp_var [n_poses*V, ht*wd] f32: var = 1/C + (e^T S^-1 e)/C^2 for every pixel of a FREE disparity frame (e: the
 *   pixel's column of E); d_pose_cov [n_poses, 6, 6] fp64: the diagonal block of S^-1 of every FREE pose, in the solver's
 *   left tangent (X <- Exp(dx) X), order (translation, rotation) of dx.  Rows of frames / poses that are not free in this
 *   problem (fixed, motion_only, limited_disp, without terms) are NOT written: prefill with NaN.  Either output may be
 *   NULL.  On return S and Hd of the workspace are zero again, as a vipe_dense_ba call leaves them, so a later call with
 *   reuse_plan in this workspace stays valid.  Plain stores in a fixed summation order: repeated calls are bitwise equal.
 * Live semantics only (the DROID-signature vipe_ba is not covered). */
int vipe_dense_ba_linearize(const vipe_ba_params* p, const float* d_poses, const float* d_disps, const float* d_disps_sens,
                            const float* d_intrinsics, const float* d_rig, const float* d_target, const float* d_weight,
                            const float* d_disp_damping, const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj,
                            const int64_t* d_qj, const int64_t* d_di, void* d_workspace, int64_t workspace_bytes,
                            double* d_S_out, int ld_out, int* d_info, void* stream);
int vipe_dense_ba_marginals(const vipe_ba_params* p, void* d_workspace, const double* d_Sinv, int ld, float* d_disp_var,
                            double* d_pose_cov, void* stream);

/* slam_ext.ba with the DROID signature (slam.cpp:31, geom_kernels.cu:1273-1404; dormant in the reference):
 * single pinhole intrinsics[4] at 1/8 scale, targets/weights [E,2,ht,wd], eta [t1-t0... see file], poses/disps
 * updated in place; dx [t1-t0,6], dz [K,ht*wd] written for the last iteration. */
int64_t vipe_ba_workspace_bytes(int n_poses, int ht, int wd, int E);
int vipe_ba(float* d_poses, float* d_disps, const float* d_intrinsics, const float* d_disps_sens,
            const float* d_targets, const float* d_weights, const float* d_eta, const int64_t* d_ii,
            const int64_t* d_jj, int n_poses, int ht, int wd, int E, int n_eta, int t0, int t1, int iterations,
            float lm, float ep, int motion_only, float* d_dx, float* d_dz, void* d_workspace,
            int64_t workspace_bytes, void* stream);

/* frame_distance: replaces frame_distance_cuda, geom_kernels.cu:1406-1434 (kernel :521-676).
 * poses [NV,7], disps [NV,ht,wd], intrinsics [V,4] (pinhole, 1/8 scale), pi,pj,qi,qj,di [M] int64, dist [M]. */
int vipe_frame_distance(const float* d_poses, const float* d_disps, const float* d_intrinsics, const int64_t* d_pi,
                        const int64_t* d_pj, const int64_t* d_qi, const int64_t* d_qj, const int64_t* d_di,
                        float* d_dist, int M, int ht, int wd, float beta, void* stream);

/* [fused] GraphBuffer.frame_distance_dense_disp (vipe/slam/components/buffer.py:550-593, geom.py:335-343) in one launch:
 * candidate m = (keyframe pi[m], view qi[m]) -> (pj[m], qj[m]); the per-view poses R_q^-1 G_p and the pinhole intrinsics at
 * 1 / intr_factor scale are formed in the kernel (the reference expands the poses of ALL frames and rescales the
 * intrinsics on the host side, then calls frame_distance twice and averages).  poses [N,7], rig [V,7], disps [N*V,ht,wd],
 * intrinsics [V, intr_dim] at full resolution (intr_dim 4 pinhole, 5 MEI), dist [M]; bidirectional: 0.5 (d_ij + d_ji). */
int vipe_frame_distance_rig(const float* d_poses, const float* d_rig, const float* d_disps, const float* d_intrinsics,
                            int intr_dim, float intr_factor, const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj,
                            const int64_t* d_qj, float* d_dist, int M, int n_views, int ht, int wd, float beta,
                            int bidirectional, void* stream);

/* depth_filter: replaces depth_filter_cuda, geom_kernels.cu:1462-1486 (kernel :678-793).
 * poses [n,7], disps [n,ht,wd], intrinsics [4], inds [num] int64, thresh [num] f32, counter [num,ht,wd] f32. */
int vipe_depth_filter(const float* d_poses, const float* d_disps, const float* d_intrinsics, const int64_t* d_inds,
                      const float* d_thresh, float* d_counter, int n, int num, int ht, int wd, void* stream);

/* The same three operations for VIPE_CAM_PANORAMA (the Sphere family of csrc/geom_ops.hip); there are no intrinsics to pass.
 * vipe_frame_distance_sphere: vipe_frame_distance_rig (buffer.py:550-593, geom_kernels.cu:560-676) on the sphere - flow in
 * pixels of the grid with the horizontal part wrapped at the seam, validity by range and pole distance.
 * vipe_depth_filter_sphere: vipe_depth_filter (geom_kernels.cu:678-793) - the inverse range in the neighbour frame against
 * its four bilinear neighbours, columns wrapped, rows not.
 * vipe_iproj_sphere: vipe_iproj (geom_kernels.cu:795-861) - points act(pose, (ray, d)) / d with the ray of
 * cameras.py:378-386. */
int vipe_frame_distance_sphere(const float* d_poses, const float* d_rig, const float* d_disps, const int64_t* d_pi,
                               const int64_t* d_qi, const int64_t* d_pj, const int64_t* d_qj, float* d_dist, int M,
                               int n_views, int ht, int wd, float beta, int bidirectional, void* stream);
int vipe_depth_filter_sphere(const float* d_poses, const float* d_disps, const int64_t* d_inds, const float* d_thresh,
                             float* d_counter, int n, int num, int ht, int wd, void* stream);
int vipe_iproj_sphere(const float* d_poses, const float* d_disps, float* d_points, int n, int ht, int wd, void* stream);

/* projmap: replaces projmap_cuda, geom_kernels.cu:1436-1460 (kernel :434-519). coords [E,ht,wd,3], valid [E,ht,wd,1]. */
int vipe_projmap(const float* d_poses, const float* d_disps, const float* d_intrinsics, const int64_t* d_ii,
                 const int64_t* d_jj, float* d_coords, float* d_valid, int E, int ht, int wd, void* stream);

/* iproj: replaces iproj_cuda, geom_kernels.cu:1488-1507 (kernel :795-861). points [n,ht,wd,3]. */
int vipe_iproj(const float* d_poses, const float* d_disps, const float* d_intrinsics, float* d_points, int n, int ht,
               int wd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * scatter_ext  (csrc/scatter_ext/scatter.cpp:232-238, cuda/scatter_cuda.cu:57-131)
 * src viewed as [outer, src_dim, inner], out as [outer, out_dim, inner], index broadcast to src's shape
 * (int64, same layout as src).  reduce: 0 sum, 1 mul, 2 mean (sum only - caller divides), 3 min, 4 max.
 * For min/max, d_arg_out [outer,out_dim,inner] int64 receives the arg index (src_dim where none).
 * ------------------------------------------------------------------------------------------- */
int vipe_scatter(const void* d_src, const int64_t* d_index, void* d_out, int64_t* d_arg_out, int64_t outer,
                 int64_t src_dim, int64_t inner, int64_t out_dim, int reduce, int dtype, void* stream);
/* the same with index [src_dim]: one slot per ROW of the scattered dimension (what scatter_mean's callers pass,
 * droid_net.py:420-421) - no int64 copy of src's shape.  Rows with a slot outside [0, out_dim) are skipped by both. */
int vipe_scatter_rows(const void* d_src, const int64_t* d_index, void* d_out, int64_t* d_arg_out, int64_t outer,
                      int64_t src_dim, int64_t inner, int64_t out_dim, int reduce, int dtype, void* stream);

/* The same reductions over HOST memory (float32 / float64), for CPU tensors handed to the Python-level scatter API
 * (vipe/ext/scatter.py:24-63 accepts them through torch.scatter_add_).  Sequential and deterministic; min / max ties
 * resolve to the last source row.  Index values are range-checked (VIPE_EINVAL). */
int vipe_scatter_host(const void* h_src, const int64_t* h_index, void* h_out, int64_t* h_arg_out, int64_t outer,
                      int64_t src_dim, int64_t inner, int64_t out_dim, int reduce, int dtype);

/* [fused] segmented mean of per-edge feature maps onto source nodes (GraphAgg, droid_net.py:420-421):
 * src [E,inner] f16, ix [E] int64 sorted or not, out [n_out,inner] f16 = mean over edges with ix == k. */
int vipe_scatter_mean_rows_f16(const void* d_src, const int64_t* d_ix, void* d_out, int E, int n_out, int64_t inner,
                               void* stream);

/* [fused] deterministic segmented mean (no atomics): out[k] = mean over q in [rowptr[k], rowptr[k+1]) of
 * src[order[q], :, coff:coff+C]; src [E, rows_per_item, src_ctot] f16, out [n_out, rows_per_item, C] f16. */
int vipe_segment_mean_nhwc_f16(const void* d_src, int src_ctot, int src_coff, const int* d_order, const int* d_rowptr,
                               void* d_out, int n_out, int64_t rows_per_item, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * corr_ext  (csrc/corr_ext/correlation_sampler.cpp:82-85, correlation_cuda_kernel.cu:216-330)
 * in1,in2 [B,C,H,W]; out [B,patchH,patchW,oH,oW]; dtype f16/f32.
 * ------------------------------------------------------------------------------------------- */
int vipe_corr_sampler_forward(const void* d_in1, const void* d_in2, void* d_out, int B, int C, int H, int W, int kH,
                              int kW, int patchH, int patchW, int padH, int padW, int dilH, int dilW,
                              int dil_patchH, int dil_patchW, int dH, int dW, int dtype, void* stream);
int vipe_corr_sampler_backward(const void* d_in1, const void* d_in2, const void* d_grad_out, void* d_grad1,
                               void* d_grad2, int B, int C, int H, int W, int kH, int kW, int patchH, int patchW,
                               int padH, int padW, int dilH, int dilW, int dil_patchH, int dil_patchW, int dH,
                               int dW, int dtype, void* stream);

/* The same two operators over HOST memory (float32), for CPU tensors: the reference dispatches those to its CPU
 * implementation (correlation_sampler.cpp:44-58, correlation_cpu.cpp).  grad1 / grad2 are accumulated into. */
int vipe_corr_sampler_forward_host(const float* h_in1, const float* h_in2, float* h_out, int B, int C, int H, int W, int kH,
                                   int kW, int patchH, int patchW, int padH, int padW, int dilH, int dilW, int dil_patchH,
                                   int dil_patchW, int dH, int dW);
int vipe_corr_sampler_backward_host(const float* h_in1, const float* h_in2, const float* h_grad_out, float* h_grad1,
                                    float* h_grad2, int B, int C, int H, int W, int kH, int kW, int patchH, int patchW,
                                    int padH, int padW, int dilH, int dilW, int dil_patchH, int dil_patchW, int dH, int dW);

/* ---------------------------------------------------------------------------------------------
 * utils_ext.nearest_neighbours (csrc/utils_ext/knn.cu:27-67, utils_bind.cpp:23-24): exact k nearest neighbours of every
 * query point among the tree points, squared L2 distance, points of 1..3 coordinates (missing ones count as 0, as the
 * reference's zero padding).  query [M,qdim] f32, tree [N,tdim] f32 -> dist [M,knn] f32 ascending, idx [M,knn] int32.
 * Brute force with the tree staged through LDS (the reference builds a kd-tree per call); 1 <= knn <= 8, knn <= N.
 * Equal distances resolve to the lower index (the reference's kd-tree order is unspecified).  Used by
 * SLAMMap.project_map(infill=True) (interface.py:126-139) - outside the update iteration.
 * ------------------------------------------------------------------------------------------- */
int vipe_nearest_neighbours(const float* d_query, int qdim, const float* d_tree, int tdim, int64_t M, int64_t N, int knn,
                            float* d_dist, int* d_idx, void* stream);

/* ---------------------------------------------------------------------------------------------
 * grounding_dino_ext  (csrc/grounding_dino_ext/vision.cpp:9-33, ms_deform_attn_cuda.cu): multi-scale deformable
 * attention of GroundingDINO's encoder and decoder layers (groundingdino/models/main/ms_deform_attn.py:319-333).
 *   value [bs,Lv,heads,C], spatial_shapes [L,2] int64 (H, W per level), level_start_index [L] int64,
 *   sampling_loc [bs,Lq,heads,L,P,2] normalised (x, y), attn_weight [bs,Lq,heads,L,P]; dtype VIPE_F32 or VIPE_F64.
 * Sample (x W - 0.5, y H - 0.5), bilinear, corners outside the level - or outside [0, Lv) - count as zero: the
 * reference's multi_scale_deformable_attn_pytorch (ms_deform_attn.py:92-134, grid_sample zeros / align_corners=False).
 * The whole batch is one launch (the reference's im2col_step chunks do not change the result).  bs * Lq == 0: VIPE_OK,
 * no launch.  L > 1024 levels: VIPE_EUNSUPPORTED.
 * ------------------------------------------------------------------------------------------- */
/* output [bs,Lq,heads*C] (every element written) */
int vipe_ms_deform_attn_forward(const void* d_value, const int64_t* d_spatial_shapes, const int64_t* d_level_start_index,
                                const void* d_sampling_loc, const void* d_attn_weight, void* d_output, int64_t bs,
                                int64_t Lv, int heads, int C, int L, int64_t Lq, int P, int dtype, void* stream);
/* grad_output [bs,Lq,heads*C] -> grad_value [bs,Lv,heads,C] ACCUMULATED by float atomics (zero it first; last bits
 * order-dependent), grad_sampling_loc / grad_attn_weight in the shapes of their inputs, written (deterministic). */
int vipe_ms_deform_attn_backward(const void* d_value, const int64_t* d_spatial_shapes, const int64_t* d_level_start_index,
                                 const void* d_sampling_loc, const void* d_attn_weight, const void* d_grad_output,
                                 void* d_grad_value, void* d_grad_sampling_loc, void* d_grad_attn_weight, int64_t bs,
                                 int64_t Lv, int heads, int C, int L, int64_t Lq, int P, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * [fused] flow-update operator convolutions (UpdateModule, droid_net.py:432-499): NHWC fp16
 * implicit-GEMM convolution on MFMA, fp32 accumulate, fused bias + activation.
 *   x [B,H,W,Cin_total] f16, reads channels [cin_off, cin_off+Cin); w packed [KH*KW, Cin, Cout] f16
 *   (vipe_conv_pack_weights from the OIHW checkpoint layout); bias [Cout] f32 in a buffer that is READABLE up to
 *   cout_pad floats (vipe_conv_packed_dims): the tile kernels load the bias in the vectors of their padded channel tile;
 *   the values behind Cout are ignored (any bit pattern), only the memory has to exist.  This holds for d_bias of
 *   vipe_conv2d_nhwc_f16, vipe_conv2d_fused and vipe_corr_lookup_conv1x1;
 *   y [B,H,W,Cout_total] f16, writes channels [cout_off, cout_off+Cout).
 *   act: 0 none, 1 relu, 2 sigmoid, 3 tanh.  Stride 1, "same" padding.
 *   extra [B,Cout] f32 (optional, NULL = none): per-image additive term (the *_glo 1x1 of the GRU).
 * ------------------------------------------------------------------------------------------- */
#define VIPE_ACT_NONE 0
#define VIPE_ACT_RELU 1
#define VIPE_ACT_SIGMOID 2
#define VIPE_ACT_TANH 3
int vipe_conv_pack_weights(const void* d_w_oihw, void* d_w_packed, int Cout, int Cin, int KH, int KW, int src_dtype,
                           void* stream);
int vipe_conv2d_nhwc_f16(const void* d_x, const void* d_w_packed, const float* d_bias, const float* d_extra,
                         void* d_y, int B, int H, int W, int Cin, int cin_total, int cin_off, int Cout,
                         int cout_total, int cout_off, int KH, int KW, int act, void* stream);

/* padded sizes of the packed weight tensor [k_pad/64][cout_pad][64] (any pointer may be NULL) */
int vipe_conv_packed_dims(int Cout, int Cin, int KH, int KW, int* cout_pad, int* cin_pad, int* k_pad);

/* [fused] the flow-update operator's fused convolutions (droid_net.py:373-499).  Input channels [0,split)
 * come from x0, [split,Cin) from x1 (the concatenations of the reference are never materialised).  mode:
 *   0 plain   y = act(conv + bias + extra[image])
 *   1 GLO     fout[image,c] += sum_pixels sigmoid(conv+bias)[c] * net[c]          (ConvGRU global context, :392-393)
 *   2 ZR      Cout = 256: y[:, c] = z = sigmoid(.), c < 128;  y2[:, c-128] = sigmoid(.) * net   (:395-397)
 *   3 Q       Cout = 128: y = (1 - z) * net + z * tanh(conv + bias + extra)                   (:397-399)
 *   4 HEADS   Cout = 4: fout[pixel] = (delta_x, delta_y, sigmoid(w_x), sigmoid(w_y)) as float (:486-490)
 *   5 ETA     Cout = 1: fout[pixel] = 0.01 * softplus(conv + bias)                            (:410,429)
 *   6 PARTIAL fout[pixel, y_coff + c] (f32, row pitch y_ctot floats) = accinit + conv: the raw fp32 accumulators, no
 *             bias / extra / activation - a partial sum over THESE input channels that a later launch over the other
 *             channels starts from (d_accinit of that launch, mode | VIPE_CONV_ACCINIT_F32).  Cout % 4 == 0; same shape
 *             support as d_accinit.  Used to compute the hidden-state part of the z|r gates of the NEXT update
 *             iteration on a side stream while the dense BA of the current one leaves the chip idle.
 *   7 HEADS_FUSED  Cin = 128, Cout = 256, 3x3, relu, H % 4 == 0 and W % 64 == 0 (VIPE_EUNSUPPORTED otherwise): the
 *             convolution delta0 | weight0 with the 3x3 flow / weight heads (mode 4 over its output) contracted in its
 *             epilogue - nothing of the 256 channels is stored.  This mode has no hidden state and no second output, and
 *             its two operands travel in their slots - a matter of this positional ABI alone; inside the library they
 *             have names of their own (csrc/conv_call.cuh).  d_net = the heads2 weights as matrix fragments
 *             (fp16 [cout slice s = 2][cout half h = 2][row block rb = 2][ip = 2][lane = 64][e = 8]: the weight
 *             of output 2 s + o, tap t, with 2 t + o = 16 rb + lane % 16 (zero from 18 on), for input channel
 *             128 s + 64 h + 32 ip + 16 (e / 4) + 4 (lane / 16) + e % 4), d_fout = [B*H*W, 4] f32 and
 *             d_y2 = [vipe_heads_border_floats] f32 receive every tile's partial sums; vipe_heads_finish on the same
 *             stream turns d_fout into the output of mode 4.  All sums in a fixed order, no atomics: run to run
 *             bit-identical; against the two launches it replaces, the fp32 summation order before the one fp16
 *             rounding differs.
 * mode may be OR-ed with VIPE_CONV_ACCINIT_F32: d_accinit is then float32 [B*H*W, ai_ctot] instead of fp16.
 */
#define VIPE_CONV_PARTIAL 6
#define VIPE_CONV_HEADS_FUSED 7
#define VIPE_CONV_ACCINIT_F32 0x100
/* d_accinit (optional, fp16 [B*H*W, ai_ctot], channels [ai_coff, ai_coff + Cout)): initial value of the accumulators,
 * i.e. a precomputed partial sum over OTHER input channels (convolution is linear in its input channels).  Used to
 * hoist the context-feature part of the GRU gates, constant per edge, out of the update iteration.  Taken by the tile
 * kernels only: 1x1 / 3x3 with Cout >= 64 on grids made of 4 x 64 tiles (H % 4 == 0 and W % 64 == 0) or, for every other
 * grid, the flat tiling up to 126 columns; VIPE_EUNSUPPORTED otherwise. */
int vipe_conv2d_fused(const void* d_x0, int x0_ctot, int x0_coff, const void* d_x1, int x1_ctot, int x1_coff,
                      int split, const void* d_w_packed, const float* d_bias, const float* d_extra, int extra_stride,
                      int extra_off, void* d_y, int y_ctot, int y_coff, void* d_y2, int y2_ctot, int y2_coff,
                      const void* d_net, int net_ctot, int net_coff, const void* d_z, float* d_fout,
                      const void* d_accinit, int ai_ctot, int ai_coff, int B, int H, int W, int Cin, int Cout, int KH,
                      int KW, int act, int mode, void* stream);

/* [fused] mode 7 of vipe_conv2d_fused and its second half.  vipe_heads_fused_ok: 1 when the operator (in its two-stream form) takes
 * the fused pair on an H x W grid (4 x 64 tiles; VIPE_AMD_FUSED_HEADS=0 in the environment switches it off for A/B runs) - the one
 * predicate of the library and of its Python sequencer.  vipe_heads_border_floats: size of d_border.  vipe_heads_finish:
 * d_dw[m] (the pixel's own partial sums) + its neighbouring tiles' border sums + d_bias[0..3], rounded as mode 4 does. */
int vipe_heads_fused_ok(int H, int W);
int vipe_heads_border_floats(int E, int H, int W, int64_t* n_floats);
int vipe_heads_finish(float* d_dw, const float* d_border, const float* d_bias, int E, int H, int W, void* stream);

/* [fused] the whole flow-update operator (UpdateModule.forward, droid_net.py:467-499) sequenced natively: its fused
 * convolutions above (eleven launches: corr0 - or the fused lookup -, corr2, flow0, flow2, w, z|r, q, heads0, heads2,
 * agg2, eta; twelve with heads0 split by consumer, see vipe_update_weights; one more z|r launch with a partly staged
 * gate state) + vipe_corr_lookup_conv1x1 + vipe_segment_mean_nhwc_f16 + the pooled-context product in ONE call
 * (issued one by one from the host each launch costs more than most of them run for on a frontend window).
 * All tensors channels-last fp16 unless noted; the weight descriptors are `vipe_conv_pack_weights` outputs + fp32 biases
 * (each readable up to its convolution's padded output-channel count, see d_bias above). */
typedef struct {
  const void *corr0_w, *corr2_w, *flow0_w, *flow2_w, *gw_w, *zr_w, *q_w, *zr_s_w, *q_s_w, *heads0_w, *heads2_w, *agg2_w, *eta_w;
  const void *zr_n_w, *zr_x_w; /* z|r gate weights over the hidden state only [256 <- 128] and over (corr | flow) only
                                  [256 <- 192]: the two halves of zr_s_w (vipe_update_gate_state) */
  const float *corr0_b, *corr2_b, *flow0_b, *flow2_b, *gw_b, *zr_b, *q_b, *heads0_b, *heads2_b, *agg2_b, *eta_b;
  const float* glo_wT; /* [128,384] f32: (convz_glo | convr_glo | convq_glo) weights transposed */
  const float* glo_b;  /* [384] */
  /* heads0 packed twice more, by consumer: agg1 [128 <- 128] = its channels 256..383 (GraphAgg's first convolution) and
     heads_dw [256 <- 128] = its channels 0..255 (delta0 | weight0).  Both set, a side stream and n_src > 0: the operator
     runs agg1 first, so that the GraphAgg chain (segmented mean, agg conv 2, eta) starts beside the heads convolution
     instead of behind all 384 channels.  Otherwise: the one 384-channel heads0 launch (three launches of 128 and 256
     channels leave more partly filled workgroup rounds than one of 384), then heads || GraphAgg chain. */
  const void *agg1_w, *heads_dw_w;
  const float *agg1_b, *heads_dw_b;
  const void* heads2_frag; /* optional: heads2_w as the matrix fragments of vipe_conv2d_fused mode 7.  With it (and agg1_w,
                              heads_dw_w, vipe_update_buffers.hborder) the split form takes the fused heads on grids
                              of 4 x 64 tiles: hbuf[..., 0:256] is then not written */
} vipe_update_weights;
typedef struct {
  int E, H, W, n_src;        /* edges, grid, source nodes (0: no GraphAgg / eta) */
  /* correlation features: either a pyramid to look up (levels[0] != NULL; lookup fused with corr_encoder[0]) ... */
  const void* levels[4];
  const float* coords;       /* [E,H,W,2] */
  const int* slots;          /* optional [E] */
  int h2, w2, pyramid_layout;
  const void* corr;          /* ... or the looked-up features [E,H,W,200] */
  const void* motn;          /* [E,H,W,4] */
  const void* net;           /* [E,H,W,128] hidden state (read) */
  void* net_out;             /* [E,H,W,128] new hidden state (must not alias net: 3x3 halo) */
  void* xbuf;                /* [E,H,W,320]: [inp | corr features | flow features], channels >= 128 overwritten */
  const void* pgate;         /* optional [E,H,W,384]: context-feature part of the gate convolutions (gate-context hoisting) */
  void *c1, *f1, *zb, *rnet; /* scratch [E,H,W,128] */
  void* hbuf;                /* scratch [E,H,W,384] */
  float* dw;                 /* out [E,H,W,4] f32: (delta_x, delta_y, weight_x, weight_y) */
  float *glo, *extra;        /* scratch [E,128], [E,384] f32 */
  const int *order, *rowptr; /* CSR of the edges by source node (vipe_segment_mean_nhwc_f16) */
  void *agg, *a2;            /* scratch [n_src,H,W,128] */
  float* eta;                /* out [n_src,H,W] f32 */
  void* side_stream;         /* optional second stream: the operator's two pairs of independent chains - (lookup + corr
                                encoder) || (flow encoder), and (flow / weight heads) || (GraphAgg mean, agg conv 2, eta; from behind agg1 when heads0 is split by consumer) -
                                are issued on `stream` and on this one, forked and joined with events inside the call
                                (a gather-bound kernel next to a matrix-bound one); NULL: everything on `stream` */
  float* pzr;                /* optional [gate_state,H,W,256] f32: hidden-state part of the z|r gates (vipe_update_gate_state) */
  int gate_state;            /* n > 0: `extra` (all edges) and `pzr` (the first n edges) already hold the hidden-state part
                                of the gates for `net` (vipe_update_gate_state ran on it): the operator skips the
                                global-context stage, and the z|r convolution of the first n edges runs over (corr | flow)
                                only, its accumulators starting from pzr; edges [n, E) take the unsplit convolution */
  float* hborder;            /* optional scratch [vipe_heads_border_floats(E, H, W)] f32 for the fused heads */
} vipe_update_buffers;
int vipe_update_operator(const vipe_update_weights* weights, const vipe_update_buffers* buffers, void* stream);

/* Everything of the ConvGRU gates that depends on the hidden state ALONE, for hidden state d_net [E,H,W,128]:
 *   extra[E,384] = the three *_glo terms (droid_net.py:392-399; uses buffers->glo as scratch),
 *   pzr[E,H,W,256] (f32) = pgate[..., 0:256] + conv3x3(d_net; W_{z|r}[:, 0:128])   (no bias).
 * Convolution is linear in its input channels, so the next vipe_update_operator call with gate_state = 1 gives the
 * result of the unsplit operator up to fp32 summation order.  The point: d_net is final as soon as the operator has
 * run, while the dense BA that follows it in an update iteration keeps one workgroup busy - issued on a second stream
 * this stage (18 % of the operator's FLOPs) runs in the BA's shadow.  Needs buffers->pgate and buffers->pzr.
 * parts: 1 = the global-context terms (all E edges), 2 = the z|r partial sums (all E edges of the descriptor handed
 * in: a caller that stages only the first n edges passes a descriptor with E = n), 3 = both. */
int vipe_update_gate_state(const vipe_update_weights* weights, const vipe_update_buffers* buffers, const void* d_net,
                           int parts, void* stream);
/* The z|r partial sums (parts = 2) in pieces, with the signature of vipe_overlap_fn: piece k of n covers edges
 * [bounds[k], bounds[k+1]) (bounds: n + 1 ascending ints from 0 to E; NULL: [E k / n, E (k+1) / n)).
 * `user` points to a vipe_gate_state_job. */
typedef struct {
  const vipe_update_weights* weights;
  const vipe_update_buffers* buffers;
  const void* net;
  const int* bounds;
  int n_bounds;      /* entries of bounds (= pieces + 1); a call with another piece count falls back to the even split */
} vipe_gate_state_job;
int vipe_update_gate_state_piece(void* user, int piece, int n_pieces, void* stream);

/* the ConvGRU's three global-context 1x1 convolutions on the pooled vector (droid_net.py:392-399):
 * extra[E,384] = bias + (glo_sum[E,128] / hw) @ wT[128,384]   (all f32) */
int vipe_glo_context(const float* d_glo_sum, const float* d_wT, const float* d_bias, float* d_extra, int E, int hw,
                     void* stream);

/* Per-edge state of a factor graph in stores with spare capacity (vipe_amd/slam/factor_graph.py `_EdgeState`).  The
 * reference concatenates - i.e. copies - every per-edge tensor in `add_factors` (factor_graph.py:147-173) and compacts each
 * with a boolean mask in `rm_factors` (:175-202).  Both are ONE launch here, for all tensors together (at most 8 jobs):
 *   vipe_rows_gather: for every job, dst row (dst_row0 + r) = src row idx[r] (r itself if idx is NULL), r < n_rows; a row
 *     is n_seg segments of seg_bytes bytes every seg_pitch bytes (a channel slice of a channels-last tensor: one segment
 *     per pixel), rows start every src_row_pitch / dst_row_pitch bytes.  Sizes, pitches and addresses multiples of 4 (copied
 *     in the largest of 16 / 8 / 4 bytes they are all multiples of); src != dst.
 *   vipe_gather_nchw_to_nhwc_f16: dst[dst_row0 + r][p][dst_coff + c] = src[frame[r]][c][p] for c < C <= 128, p < P:
 *     `buffer.nets[ii].permute(0, 2, 3, 1)` / `buffer.inps[ii]...` of the new edges' source frames, written straight into
 *     the tail of the channels-last stores (dst rows of dst_row_pitch halves, dst_ctot channels per pixel). */
typedef struct {
  const void* src;
  void* dst;
  const int64_t* idx;
  int64_t src_row_pitch, dst_row_pitch;
  int64_t seg_bytes, seg_pitch;
  int n_seg;
  int n_rows;
  int dst_row0;
} vipe_rows_job;
int vipe_rows_gather(const vipe_rows_job* jobs, int n_jobs, void* stream);
typedef struct {
  const void* src;          /* [N, C, P] f16 */
  const int64_t* frame;     /* [n_rows] */
  void* dst;
  int64_t dst_row_pitch;    /* halves */
  int dst_ctot, dst_coff;
  int dst_row0;
} vipe_nhwc_job;
int vipe_gather_nchw_to_nhwc_f16(const vipe_nhwc_job* jobs, int n_jobs, int n_rows, int C, int P, void* stream);

/* [fused] MotionFilter's dense score (vipe/slam/components/motion_filter.py:103-110): score[v] = mean over pixels of
 * |(half) delta| (masked: sum(|delta| (1 - invalid)) / P / (mean(1 - invalid) + 1e-6)).  dw [n_views, P, 4] f32 = the update
 * operator's (delta_x, delta_y, weight_x, weight_y); invalid [n_views, P] bytes (bool) or NULL; score [n_views] f32. */
int vipe_flow_score(const float* d_dw, const unsigned char* d_invalid, float* d_score, int n_views, int P, void* stream);

/* [fused] tail of FactorGraph.update (factor_graph.py:270-276): target = coords1 + delta, weight = (masked source frame
 * ? 0 : w), damping[du[k]] = eta[k].  coords1 / target / weight [E,ht,wd,2] f32, dw [E,ht,wd,4] f32, mask [E,ht,wd] bytes
 * (optional), eta [n_src,ht,wd], du [n_src] int64, damping [*,ht,wd]. */
int vipe_update_finish(const float* d_coords1, const float* d_dw, const unsigned char* d_mask, float* d_target,
                       float* d_weight, const float* d_eta, const int64_t* d_du, float* d_damping, int E, int n_src, int ht,
                       int wd, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Frame encoders: BasicEncoder fnet / cnet (vipe/slam/networks/droid_net.py:290-370,
 * DroidNet.encode_features / encode_context :510-527), run per frame by MotionFilter.check
 * (vipe/slam/components/motion_filter.py:58-150).  NHWC fp16 activations, fp32 bias, packed fp16 weights:
 *   conv: [k*k][Cin/32][Cout][32] (tap-major, 32-channel chunks);  stem: [7][32][32] with k = tap*4 + c (c = 3 and
 *   taps >= 49 zero).  Instance-norm statistics are [B, C, 2] fp32 (sum, sum of squares of the fp16 outputs),
 *   accumulated by the producing kernel (zero them first) and applied (x - mean) * rstd, eps 1e-5, + ReLU by the
 *   consumer while it loads.
 * ------------------------------------------------------------------------------------------- */
/* [V,3,H,W] fp32 RGB in [0,1] -> [V,H,W,4] fp16 ((x - mean) / std, 4th channel 0) */
int vipe_enc_prep(const float* d_img, void* d_x4, int V, int H, int W, void* stream);
/* 7x7 stride-2 pad-3 stem, 3(+1) -> 32 channels: y [B,(H-1)/2+1,(W-1)/2+1,32] = conv + bias (+ReLU if relu).
 * d_out_stats != null: the sum and the sum of squares of the fp16-rounded conv + bias are ADDED to it - the value
 * BEFORE the activation, whatever `relu` says (instance norm comes before the ReLU, droid_net.py:355-357). */
int vipe_enc_stem(const void* d_x4, const void* d_w, const float* d_bias, void* d_y, float* d_out_stats, int B, int H,
                  int W, int relu, void* stream);
/* ksize in {1,3} (pad ksize/2), stride in {1,2}, Cin in {32,64,96,128}, Cout a positive multiple of 32 (anything else
 * VIPE_EINVAL, another ksize / stride VIPE_EUNSUPPORTED).
 * d_in_stats != null: the input is relu(instance_norm(x)) formed on load.  d_res != null (NHWC only):
 * y = relu(res + act(conv)).  nchw: y is [B,Cout,Ho,Wo].  tanh_split >= 0: channels < split get tanh, the others
 * ReLU (context net output, droid_net.py:525-527).
 * d_out_stats != null: the sum and the sum of squares of the fp16-rounded conv + bias are ADDED to it - the value
 * BEFORE the activation: before ReLU, tanh and the residual, so `relu` does not change them. */
int vipe_enc_conv(const void* d_x, const float* d_in_stats, const void* d_w, const float* d_bias, const void* d_res,
                  void* d_y, float* d_out_stats, int B, int H, int W, int Cin, int Cout, int ksize, int stride,
                  int relu, int nchw, int tanh_split, void* stream);
/* residual tail of a normalised block: out = relu(xres + relu(IN(raw))); xres = res, or IN(res) if d_res_stats;
 * d_res == null: out = relu(IN(raw)).  All [B,HW,C] fp16. */
int vipe_enc_finish(const void* d_raw, const float* d_raw_stats, const void* d_res, const float* d_res_stats,
                    void* d_out, int B, int HW, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Native-resolution frame ingest: what SLAMSystem.run's StandardResizeStreamProcessor (vipe/slam/system.py:42-77),
 * VideoFrame.resize / crop (vipe/streams/base.py:164-254), _precompute_features (system.py:183-205) and the sensor
 * disparity lines of _add_keyframe (system.py:152-156) make of ONE view of one decoded frame, in one launch.
 * ------------------------------------------------------------------------------------------- */
/* [fused] The frame [H0,W0] is resampled to (h1,w1) - F.interpolate(mode="bilinear", size=(h1,w1)): align_corners=False,
 * no antialiasing, scale = float(in) / float(out), src = max(fma(scale, dst + 0.5, -0.5), 0) (one fused operation, as
 * torch's device kernel evaluates it), i1 = min(i0 + 1, in - 1), every other product and sum rounded on its own - and
 * cropped to rows [top, top + H), columns [left, left + W).  H and W must be multiples of 8 and the crop must lie
 * inside (h1,w1); anything else is VIPE_EINVAL.
 *   d_rgb        [H0,W0,3], rgb_dtype VIPE_U8 (x / 255 before the resample), VIPE_F16 or VIPE_F32, values 0-1
 *   d_mask       [H0,W0] bytes (torch.bool / uint8, non-zero = usable pixel) or NULL
 *   d_depth      [H0,W0] f32 metric depth or NULL
 *   d_images     [3,H,W] f32 planar: the resampled, cropped rgb (GraphBuffer.images)
 *   d_x4         [H,W,4] f16: (images - mean) / std with a zero 4th lane - bit for bit what vipe_enc_prep makes of
 *                d_images, so the encoders are fed without that pass
 *   d_mask8      [H/8,W/8] bytes, 1 = INVALID: the resampled mask thresholded at > 0.9 (VideoFrame.resize), cropped,
 *                resampled to 1/8 and thresholded at > 0.9 again, inverted (_precompute_features).  At exactly 1/8 the
 *                second stage is the mean of the thresholded pixels at rows 8i+3, 8i+4 and columns 8j+3, 8j+4: a cell is
 *                valid iff those four are, and only those four are computed.  Untouched when d_mask is NULL.
 *   d_disps_sens [H/8,W/8] f32: the resampled, cropped depth at [3::8, 3::8], then d > 0 ? 1 / d : d.  Untouched when
 *                d_depth is NULL.
 * One output pixel per thread in 64 x 4 tiles; the 1/8 outputs come from the threads that own pixel (8i+3, 8j+3). */
int vipe_frame_ingest(const void* d_rgb, int rgb_dtype, const unsigned char* d_mask, const float* d_depth, int H0, int W0,
                      int h1, int w1, int top, int left, int H, int W, float* d_images, void* d_x4,
                      unsigned char* d_mask8, float* d_disps_sens, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Full-resolution keyframe disparity: DROID-SLAM's learned convex upsampling (cvx_upsample), the consumer of the
 * update operator's GraphAgg.upmask head.  An addition: the reference computes the mask and discards it
 * (factor_graph.py:269).
 * ------------------------------------------------------------------------------------------- */
/* out[r, 8y+dy, 8x+dx, c] = sum_k softmax_k(mask[s, y, x, k*64 + dy*8 + dx]) * data[r, y+ky-1, x+kx-1, c] with tap
 * k = ky*3 + kx (ky, kx in 0..2), sub-pixel (dy, dx) in 0..7, data read as zero outside the grid, r = d_rows[s] or, with
 * d_rows NULL, r = s.  The softmax runs in f32 with the maximum subtracted.
 *   d_mask  [N,h,w,576] channels-last, mask_dtype VIPE_F16 (what the operator writes) or VIPE_F32
 *   d_data  [R,h,w,C] f32, C in 1..4 (C > 4: VIPE_EUNSUPPORTED)
 *   d_out   [R,8h,8w,C] f32; rows that d_rows does not name are not written
 *   d_rows  [N] int64 or NULL (then N <= R); mask rows whose index lies outside [0, R) are skipped
 * d_mask and d_out must be 16-byte aligned.  N == 0: VIPE_OK, no launch.  One launch, flat over the N*h*w coarse
 * pixels: 16 per workgroup, a thread owns 4 x-adjacent sub-pixels (8- / 16-byte mask loads, 16-byte stores). */
int vipe_convex_upsample(const void* d_mask, int mask_dtype, const float* d_data, float* d_out, const int64_t* d_rows,
                         int N, int R, int h, int w, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Per-frame depth export: the inverse of vipe_frame_ingest's geometry.  An addition: the reference takes per-frame depth
 * from monocular depth networks; here it is the reciprocal of the SLAM disparities, back at the frame's native size.
 * ------------------------------------------------------------------------------------------- */
/* out[n] [H0,W0] is made from d_disp[d_rows[n]] [H,W] (d_rows NULL: from d_disp[n], then N <= R): the map is put back at
 * rows [top, top + H), columns [left, left + W) of the resized frame (h1,w1), the band the centre crop removed taking the
 * edge row / column (replicate padding), resampled to (H0,W0) as F.interpolate(mode="bilinear", align_corners=False)
 * does, and inverted.  Per axis, with n_res = h1 | w1, n_out = H0 | W0, off = top | left, n_in = H | W:
 *   scale = float(n_res) / float(n_out);  src = max(fma(scale, dst + 0.5, -0.5), 0)  (one fused operation, as in
 *   vipe_frame_ingest);  src = clamp(src - off, 0, n_in - 1);  i0 = int(src), i1 = min(i0 + 1, n_in - 1), l1 = src - i0,
 *   l0 = 1 - l1
 *   d = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * e), every product and sum rounded on its own
 *   depth = d > 0 ? depth_scale / d : 0, one correctly rounded division; out_dtype VIPE_F16 stores its
 *   round-to-nearest-even
 * With H0 = h1 = H, W0 = w1 = W, top = left = 0 the map is the identity: out = depth_scale / disp exactly.
 *   d_disp [R,H,W] f32;  d_rows [N] int64 or NULL - an entry outside [0, R) leaves out[n] unwritten;
 *   d_out  [N,H0,W0], out_dtype VIPE_F32 or VIPE_F16
 * Sizes must be positive, top, left >= 0, top + H <= h1, left + W <= w1, N <= 65535 and ceil(H0 / 4) <= 65535 (grid
 * limits), pointers non-null unless N == 0 (then VIPE_OK, no launch); anything else is VIPE_EINVAL.  One output pixel per
 * thread in 64 x 4 tiles, the batch index in grid.z. */
int vipe_depth_export(const float* d_disp, const int64_t* d_rows, void* d_out, int out_dtype, int N, int R, int H, int W,
                      int h1, int w1, int top, int left, int H0, int W0, float depth_scale, void* stream);

/* Per-frame depth confidence (depth_consistency.hip; an addition, the ABI version stays 4): for every pixel of the maps
 * vipe_depth_export writes, how many of K neighbour rows of the same buffer see the pixel's point and how many of those
 * confirm its disparity - the multi-view consistency count of DROID-SLAM's / the reference's depth_filter
 * (geom_kernels.cu:678-793), at native size, relative instead of absolute, any row against any rows.
 *   d_disp [R,H,W] f32: rows of GraphBuffer.disps_up, row r = buffer slot r / n_views, view r % n_views
 *   d_poses [R / n_views,7] world -> camera; d_rig [n_views,7]; d_intrinsics [n_views,intr_dim] at SLAM resolution
 *   (intr_dim 4 for VIPE_CAM_PINHOLE and VIPE_CAM_PANORAMA, whose rows are never read; 5 for VIPE_CAM_MEI)
 *   d_rows [N] int64 or NULL (identity, then N <= R): the source row of out[n]; outside [0, R): out[n] stays unwritten
 *   d_nbr [N,K] int64: neighbour rows of out[n]; entries outside [0, R) (-1: none) or equal to the source row are skipped
 *   d_out [N,H0,W0] u8; (h1, w1, top, left, H0, W0) as for vipe_depth_export
 * Per output pixel: taps and blended disparity d exactly as vipe_depth_export; d <= 0 (or not a number) gives 0.  The
 * pixel's place in the SLAM grid is the clamped source coordinate (u, v) = (ix0 + lx1, iy0 + ly1), so the replicate-padded
 * band repeats its edge pixel's test.  ray = iproj(intrinsics of r's view, u, v); for each neighbour q:
 *   T = (rig[vq]^-1 G[pq]) (rig[vr]^-1 G[pr])^-1;  X1 = R ray + t d;  valid as vipe_reproject's `valid`;  (x', y') its
 *   coordinates with q's view's intrinsics;  d' = d / X1.z (pinhole, MEI) or d / |X1| (panorama: inverse range)
 *   x0 = floor(x'), y0 = floor(y');  visible iff valid, 0 <= y0 <= H - 2 and 0 <= x0 <= W - 2 (panorama: the columns
 *   x0, x0 + 1 wrap modulo W instead)
 *   agrees iff visible and one of disp[q][y0 | y0 + 1][x0 | x0 + 1] is a t > 0 with |d' - t| <= tol * d'
 *   out = agree_count | visible_count << 4
 * 1 <= K <= 8, 1 <= n_views <= 8, R % n_views == 0, intr_dim matching the camera, tol > 0, vipe_depth_export's size and
 * grid conditions, for VIPE_CAM_PANORAMA the identity crop (top = left = 0, h1 = H, w1 = W: a crop breaks the sphere),
 * pointers non-null (d_rows excepted) unless N == 0 (then VIPE_OK, no launch); anything else is VIPE_EINVAL.  One output
 * pixel per thread in 64 x 4 tiles, the map index in grid.z; no atomics. */
int vipe_depth_consistency(const float* d_disp, const float* d_poses, const float* d_rig, const float* d_intrinsics,
                           int intr_dim, int camera, const int64_t* d_rows, const int64_t* d_nbr, unsigned char* d_out,
                           int N, int K, int R, int n_views, int H, int W, int h1, int w1, int top, int left, int H0,
                           int W0, float tol, void* stream);

/* Fused clip point cloud (cloud_fuse.hip; an addition, the ABI version stays 4): the confident pixels of the maps
 * vipe_depth_export writes, back-projected to the world and accumulated into a voxel hash table that the caller keeps on
 * the device; vipe_cloud_extract turns the table into one point per voxel.  Integer accumulators throughout: the table's
 * content does not depend on pixel order, on how the maps are split over launches, or on the run.
 *   d_disp, d_poses, d_rig, d_intrinsics, intr_dim, camera, d_rows, N, R, n_views, (H, W, h1, w1, top, left, H0, W0): as
 *   for vipe_depth_consistency; a d_rows entry outside [0, R) contributes nothing
 *   d_conf [N,H0,W0] u8 (vipe_depth_consistency's bytes) or NULL: a pixel is kept only if (conf & 15) >= min_agree
 *   d_rgb  [N,H0,W0,3] or NULL, rgb_dtype VIPE_U8 / VIPE_F16 / VIPE_F32 (read only with d_rgb); a float c becomes
 *          (int)(clamp(c, 0, 1) * 255 + 0.5f)
 *   stride 1..8: only pixels with x % stride == 0 and y % stride == 0 take part
 *   inv_voxel = 1 / voxel, rounded once by the caller
 *   d_keys [cap] int64, empty slots hold -1;  d_acc [cap,8] int32 = {count, sum qx, sum qy, sum qz, sum r, sum g, sum b,
 *          unused}, 32-bit patterns to be read as UNSIGNED, zero where the slot is empty;  cap a power of two <= 2^30
 *   d_stats [4] int64, added to: points inserted, dropped because the table was full, out of range, dropped because
 *          their voxel is saturated.  Their sum grows by the number of kept pixels.
 * Per pixel that takes part: taps and blended disparity d exactly as vipe_depth_export; d <= 0 (or not a number) skips
 * the pixel.  (u, v) = (ix0 + lx1, iy0 + ly1);  ray = iproj(intrinsics of r's view, u, v);
 *   (Rm, t) = ((rig[v]^-1 G[p])^-1 as a matrix and a translation;  Xw = (Rm ray + t d) / d  (vipe_iproj's convention)
 *   per axis s = Xw * inv_voxel, i = floorf(s): unless |i| < 2^20 on all three (a non-finite s fails) the point is out of
 *   range;  key = (ix + 2^20) | (iy + 2^20) << 21 | (iz + 2^20) << 42;  q = min(255, (int)((s - i) * 256.0f))
 *   slot: linear probing from ((uint64(key) * 0x9E3779B97F4A7C15) >> 32) & (cap - 1), wrapping at cap, one 64-bit
 *   compare-and-swap per empty slot met, at most min(cap, 128) slots - then the point is dropped and counted.  No thread
 *   waits for another.  acc[slot] += {1, qx, qy, qz, r, g, b} unless its count reads >= 2^23 (saturated, counted): a
 *   count overshoots 2^23 by less than the threads in flight (< 2^19), so no sum (<= 255 * count) passes 2^32.
 * Keep the table's load below about 0.7: past that the probe limit starts to drop points.
 * 1 <= n_views <= 8, R % n_views == 0, intr_dim matching the camera, 0 <= min_agree <= 8, inv_voxel positive and finite,
 * vipe_depth_export's size and grid conditions, for VIPE_CAM_PANORAMA the identity crop, pointers non-null (d_rows,
 * d_conf, d_rgb excepted) unless N == 0 (then VIPE_OK, no launch); anything else is VIPE_EINVAL.  One output pixel per
 * thread in 64 x 4 tiles, the map index in grid.z; a workgroup merges its tile in an LDS hash (256 entries) and sends
 * each distinct voxel to the table once; the four counters are summed per workgroup first. */
int vipe_cloud_fuse(const float* d_disp, const float* d_poses, const float* d_rig, const float* d_intrinsics, int intr_dim,
                    int camera, const int64_t* d_rows, const unsigned char* d_conf, int min_agree, const void* d_rgb,
                    int rgb_dtype, int stride, float inv_voxel, int64_t* d_keys, int* d_acc, int64_t cap, int64_t* d_stats,
                    int N, int R, int n_views, int H, int W, int h1, int w1, int top, int left, int H0, int W0,
                    void* stream);

/* The table of vipe_cloud_fuse -> one point per slot with count >= min_count (>= 1), in no particular order:
 *   xyz[m]   = (i + (sum q / count + 0.5) / 256) * voxel per axis, evaluated in double and rounded once
 *   rgb[m]   = (sum c + count / 2) / count in integers (d_rgb NULL: no colour is written)
 *   count[m], key[m]: the slot's count and key
 * d_num_out [1] int64 receives the number of such slots - the total, also when it exceeds max_out; then only max_out
 * points are written (which ones is not defined).  max_out = 0 counts only (the outputs may be NULL).
 *   d_xyz [max_out,3] f32, d_rgb [max_out,3] u8 or NULL, d_count [max_out] int32, d_key [max_out] int64
 * cap a power of two <= 2^30, voxel positive and finite, min_count >= 1, max_out >= 0, pointers non-null as stated;
 * anything else is VIPE_EINVAL.  One memset node (d_num_out) and one launch; one atomic per wave. */
int vipe_cloud_extract(const int64_t* d_keys, const int* d_acc, int64_t cap, float voxel, int min_count, float* d_xyz,
                       unsigned char* d_rgb, int* d_count, int64_t* d_key, int64_t max_out, int64_t* d_num_out,
                       void* stream);

/* The fused cloud seen from cameras again (cloud_render.hip; an addition, the ABI version stays 4): world points are
 * splatted into a 64-bit z-buffer per target image that the caller keeps on the device; vipe_cloud_resolve turns the
 * buffer into depth, colour and index images.  Packed integer minima throughout: the buffer's content depends only on the
 * set of (point, index) pairs drawn - not on point order, on how the cloud is split over launches, on calling twice, or
 * on the run.
 *   d_xyz [M,3] f32 world points; point m carries the index index_base + m; index_base >= 0, index_base + M <= 2^31 - 1
 *   d_cams [B,7] f32 world -> camera of each target image (the caller composes rig[v]^-1 G[f]; the quaternion is
 *          normalised on load); d_intrinsics [B,intr_dim] at SLAM resolution, one row per image (intr_dim 4 for
 *          VIPE_CAM_PINHOLE and VIPE_CAM_PANORAMA, whose rows are never read; 5 for VIPE_CAM_MEI)
 *   (H, W, h1, w1, top, left, H0, W0): the export geometry of vipe_depth_export with its conditions, H0, W0 <= 2^24; the
 *          images are the native-size grid [H0,W0]
 *   point_size >= 0, finite: the points' edge length in world units;  max_radius 0..4
 *   d_zbuf [B,H0,W0] uint64 in int64 storage; an empty pixel holds all ones (-1)
 *   d_stats [3] int64, added to: pairs drawn (at least one pixel written or tested), pairs invalid, pairs outside the
 *          image.  Their sum grows by M * B per launch.
 * Per point m and image b, every product and sum rounded on its own (no contraction):
 *   Xc = R X + t, per row ((R_i0 X0 + R_i1 X1) + R_i2 X2) + t_i.  Unless all of Xc is finite the pair is OUTSIDE (so is
 *   every point with a NaN or an infinite coordinate); else unless Xc.z > 0.1 (pinhole, MEI) or, panorama, |Xc| > 0.1
 *   and |(Xc.x, Xc.z)| > 1e-3 |Xc| (vipe_reproject's `valid`), the pair is INVALID
 *   z = Xc.z (pinhole, MEI) or sqrtf((X X + Z Z) + Y Y) (panorama: a range, as the panorama's frame depths are)
 *   (x, y) = the camera's projection in SLAM-grid coordinates, as vipe_depth_consistency projects
 *   per axis p = floorf(((x + off) + 0.5f) / scale), off = left | top, scale = float(w1) / float(W0) | float(h1) / float(H0):
 *   the forward form of the mapping whose inverse vipe_depth_export evaluates.  The crop band the export replicate-pads is
 *   a real part of the camera's image here: points that project into it are drawn there.  Unless
 *   -max_radius - 1 <= p <= n_out + max_radius on both axes - compared as floats, before anything becomes an integer; a
 *   NaN fails - the pair is OUTSIDE
 *   q = (0.5f * point_size) * foc / z, foc = fx / scale_x (pinhole, MEI; rounded once per image) or float(W0) / (2 pi)
 *   (panorama);  r = q >= max_radius ? max_radius : (int)q
 *   footprint [px - r, px + r] x [py - r, py + r]; rows clipped to [0, H0), columns clipped to [0, W0) - the panorama's
 *   columns are taken modulo W0 instead (its rows are clipped).  No pixel left: OUTSIDE
 *   value = (uint64)float_as_uint(z) << 32 | (uint32)(index_base + m); every footprint pixel takes
 *   min(zbuf[b][y][x], value) atomically.  z > 0, so its bit pattern orders as the number does; equal depths go to the
 *   lower index.  No thread waits for another.
 * camera, intr_dim and the panorama's identity crop as for vipe_depth_consistency; M >= 0, 0 <= B <= 65535; pointers
 * non-null unless M == 0 or B == 0 (then VIPE_OK, no launch); anything else is VIPE_EINVAL.  One thread per point, 256
 * per workgroup, the image in grid.y; the image's matrix and intrinsics are built once per workgroup in LDS; the shipped
 * form loads a pixel and skips the atomic when the stored value is already <= the candidate (values only decrease, so a
 * stale read costs at most an atomic; the always-atomic form of the same source leaves the same bits); the counters are
 * summed per workgroup first. */
int vipe_cloud_render(const float* d_xyz, int64_t M, int index_base, const float* d_cams, const float* d_intrinsics,
                      int intr_dim, int camera, int B, int H, int W, int h1, int w1, int top, int left, int H0, int W0,
                      float point_size, int max_radius, int64_t* d_zbuf, int64_t* d_stats, void* stream);

/* The z-buffer of vipe_cloud_render -> images, one thread per pixel, no atomics:
 *   d_depth [B,H0,W0], depth_dtype VIPE_F32 (the upper word as a float) or VIPE_F16 (its round-to-nearest-even, as
 *          vipe_depth_export rounds); 0 where the pixel is empty
 *   d_index [B,H0,W0] int32 or NULL: the lower word, the winner's index; -1 where empty
 *   d_rgb_out [B,H0,W0,3] u8 or NULL: d_rgb_points[index] with d_rgb_points [M_total,3] u8; 0 where empty.  A winner index
 *          outside [0, M_total) with colour requested is a caller error: the load is guarded and the pixel's colour is 0
 *          (never a fault); so it is when d_rgb_points is NULL, which is accepted only with M_total == 0
 * B >= 0, H0, W0 > 0, M_total >= 0, d_zbuf and d_depth non-null unless B == 0 (then VIPE_OK, no launch); anything else
 * is VIPE_EINVAL. */
int vipe_cloud_resolve(const int64_t* d_zbuf, int B, int H0, int W0, void* d_depth, int depth_dtype,
                       const unsigned char* d_rgb_points, int64_t M_total, unsigned char* d_rgb_out, int* d_index,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hole-free depth maps: grid kNN scale / shift completion (depth_complete.hip).  A sparse map - values at some pixels, 0
 * elsewhere, such as the fused surface vipe_cloud_resolve draws - and a dense prediction of the same size: every pixel
 * without a sparse value takes the prediction there, aligned to the K nearest pixels that hold both by an
 * inverse-distance-weighted least-squares fit of scale and shift in the disparity domain.  It is the network-free first
 * step of the reference's map-prompted depth path (priorda/depth_completion.py:246-379, `kss_completer`), restated for
 * points that are pixels of one grid; tests/depth_complete_reference.py restates it in float64.
 *
 * Per image b of B: sparse[b], pred[b] [H,W] of one dtype (VIPE_F16 / VIPE_F32), mask[b] [H,W] u8 or none.
 *   domain  VIPE_COMPLETE_DISP: the values are disparities.  VIPE_COMPLETE_DEPTH: depths; each value that enters the fit
 *           becomes a disparity by one IEEE 1.0f / x on load, and the result goes back by one 1.0f / r, rounded once to
 *           the output dtype
 *   anchor  sparse and pred are both finite and > 0 at the pixel (both are needed for the fit)
 *   target  not an anchor, pred finite and > 0, and mask NULL or non-zero there
 *   output  an anchor: its sparse value, copied bit for bit;  a target: the completion below;  neither: 0
 * Neighbours of a target (y, x): the anchors at offsets (dy, dx) with d2 = dy^2 + dx^2 <= R^2 - with wrap_x dx is the
 * signed column offset of smallest magnitude, the columns being a circle - of which the k' <= K smallest by the key
 * (d2, dy, dx), compared lexicographically, are taken.  Without wrap_x that is "smaller distance, then lower row-major
 * index", the tie rule of vipe_nearest_neighbours.  The tie rule is part of the result: on a pixel grid ties at the K-th
 * place are common, and the order of the reference's kd-tree is unspecified.
 * Fit, in f32, every product and sum rounded on its own, neighbours in key order, p the prediction's and d the sparse
 * map's disparity at a neighbour, sums starting with the first neighbour:
 *   w = 1.0f / float(d2)      the square of the reference's 1 / dist: the reference scales the ROWS of the system by its
 *                             weights before lstsq, so the squares weigh the residuals; its division by sum(w) cancels
 *   S = sum w;  pm = (sum w p) / S;  dm = (sum w d) / S;  e = p - pm;  f = d - dm
 *   var = sum (w e) e;  cov = sum (w e) f;  thr = ((2^-10 pm) (2^-10 pm)) S
 *   k' >= 2, var > thr and s = cov / var > 0:  affine, t = dm - s pm;   otherwise scale only: s = dm / pm, t = 0
 *   r = s p(y, x) + t
 * The two guards are this library's: the reference adds 1e-5 * rand to the predictions to dodge rank deficiency (so its
 * result is not a function of its input) and accepts negative scales (which turn the prediction's order around).
 * r not finite or <= 0: the output is 0, the pixel is REJECTED.  k' = 0: the output is 0, the pixel is UNREACHED.  In the
 * depth domain 1.0f / r of a subnormal r is +inf, and an f16 output can round to +inf or 0: the value is stored as it is.
 * Not built: a cap on |s|, a search beyond R, a confidence that gates the prediction.
 *   K 1..8;  radius R 1..64;  wrap_x 0 | 1 (the panorama), which needs W >= 2R + 1;  H, W <= 2^24, H W <= 2^31 - 1
 *   d_out [B,H,W] of dtype
 *   d_scale, d_shift [B,H,W] f32 or NULL: (s, t) at an affine or scale-only target, (1, 0) at an anchor, (0, 0) elsewhere
 *          (unreached and rejected targets included)
 *   d_nbr [B,H,W,K] int32 or NULL: at a target the neighbours' row-major pixel indices y W + x in key order, padded
 *          with -1 (a rejected target lists the neighbours it was fitted to); all -1 elsewhere
 *   d_stats [4] int64, added to: targets with an affine fit, with a scale-only fit, unreached, rejected - every target
 *          counts exactly once.  Summed per wave and per workgroup first.
 * Apart from the counters there are no atomics: the outputs are a function of the inputs, bit for bit, whatever the
 * batch split, the run, or what the output buffers held.
 *
 * vipe_depth_anchor_bits packs the anchor test: d_bits [B,H,ceil(W/64)] uint64 in int64 storage, bit (x & 63) of word
 * x >> 6; bits of columns past W are 0.  One wave ballot per word.  vipe_depth_complete reads the anchors from d_bits
 * alone (and masks off what a stale buffer may hold past W): without the pass every workgroup would read a
 * (tile + 2R)^2 window of both value maps.
 * vipe_depth_complete: one thread per pixel, 64 x 4 tiles, the image in grid.y.  The workgroup stages the bits of its
 * rows and a halo of R (columns: the three words around the tile; with wrap_x taken modulo W) in LDS, 3168 bytes at
 * R = 64.  A target scans rows dy = 0, -1, 1, -2, 2, .. until dy^2 exceeds its K-th best d2 (R^2 while it holds fewer
 * than K), in a row only |dx| <= floor(sqrt(kth - dy^2)), walking set bits; the K best keys d2 << 16 | (dy + R) << 8 |
 * (dx + R) stay sorted in registers.  Only the final k' neighbours' values are gathered from memory.
 * Both: B <= 65535; B == 0 is VIPE_OK without a launch; the value maps, d_bits, d_out and d_stats non-null otherwise;
 * anything else is VIPE_EINVAL.
 * ------------------------------------------------------------------------------------------- */
#define VIPE_COMPLETE_DISP 0
#define VIPE_COMPLETE_DEPTH 1

int vipe_depth_anchor_bits(const void* d_sparse, const void* d_pred, int dtype, int B, int H, int W, int64_t* d_bits,
                           void* stream);

int vipe_depth_complete(const void* d_sparse, const void* d_pred, int dtype, const unsigned char* d_mask,
                        const int64_t* d_bits, int B, int H, int W, int domain, int K, int radius, int wrap_x, void* d_out,
                        float* d_scale, float* d_shift, int* d_nbr, int64_t* d_stats, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sparse keypoint tracker: corner detection and pyramidal Lucas-Kanade (klt_track.hip), the producer of the tracks
 * that `SparseTracks` feeds to the motion filter and to the BA's second flow term.  An addition: the reference's only
 * real tracker wraps a closed CUDA package.  tests/klt_reference.py restates this arithmetic in float64.
 *
 * Common rules.  Pixel centres are at integer coordinates, x = column, y = row.  Every read outside an image
 * replicates the border (indices clamped to [0, w-1] / [0, h-1]).  All arithmetic is f32, every product and sum
 * rounded on its own (no contraction).
 *   bilinear sample S(img, x, y): x0 = floor(x), fx = x - x0 (same for y); v00 = img[y0][x0], v01 = img[y0][x0+1],
 *   v10 = img[y0+1][x0], v11 = img[y0+1][x0+1] (clamped indices); top = v00 + fx*(v01 - v00),
 *   bot = v10 + fx*(v11 - v10); S = top + fy*(bot - top).
 *   lambda_min(a, b, c) = 0.5*(a + c) - sqrt((0.5*(a - c))^2 + b^2), the smaller eigenvalue of [a b; b c].
 * A pyramid of an H x W frame with L levels is ONE f32 buffer: level 0 [H,W] first, level l+1 of size
 * ((h_l + 1)/2, (w_l + 1)/2) directly behind level l (`klt_ext.pyramid_layout` gives sizes and offsets).
 * ------------------------------------------------------------------------------------------- */
#define VIPE_KLT_OOB 1          /* a window centre of some level, or the final position, closer than `border` to an edge */
#define VIPE_KLT_LOW_TEXTURE 2  /* lambda_min(G) / (2r+1)^2 at level 0 < min_eig */
#define VIPE_KLT_RESIDUAL 4     /* level-0 mean |e| > max_residual */
#define VIPE_KLT_FB 8           /* forward-backward distance > fb_thresh (or not finite) */
#define VIPE_KLT_MASKED 16      /* mask at the rounded new position is 0 */
#define VIPE_KLT_DIVERGED 32    /* displacement not finite, or |d| > max_flow */

/* d_rgb [H,W,3], rgb_dtype VIPE_U8 or VIPE_F32 (values 0-1) -> d_pyr, L levels (1 <= L <= 6).
 *   level 0: gray = (0.299*R + 0.587*G) + 0.114*B with R, G, B on the 0-255 scale (u8 as they are; f32: the sum of the
 *            0-1 values, then * 255).
 *   level l+1 (y, x): the separable binomial [1 4 6 4 1]/16 of level l at (2y, 2x).  Rows first: for each of the rows
 *            2y-2 .. 2y+2 (clamped) t = (((p[-2] + p[2]) + 4*(p[-1] + p[1])) + 6*p[0]) * 0.0625 over the columns
 *            2x-2 .. 2x+2 (clamped); then the same expression over the five t.
 * d_rgb and d_pyr must be 16-byte aligned.  One launch per level: level 0 reads the frame once (four pixels per thread,
 * 16-byte stores), every further level reads a quarter of the one before. */
int vipe_klt_pyramid(const void* d_rgb, int rgb_dtype, int H, int W, int L, float* d_pyr, void* stream);

/* Corner detection on level 0 (d_img [H,W] f32, the head of a pyramid).  gx = 0.5*(I[y][x+1] - I[y][x-1]),
 * gy = 0.5*(I[y+1][x] - I[y-1][x]) (clamped indices); (a, b, c) = sums of (gx*gx, gx*gy, gy*gy) over the 5 x 5
 * neighbourhood, pixels outside the image contributing zero, summed row by row, left to right;
 * response = lambda_min(a, b, c).  The image is cut into cell x cell cells (4 <= cell <= 32; ncx = ceil(W / cell)
 * columns, ncy = ceil(H / cell) rows of cells, the last ones ragged).  Per cell, d_out [ncy*ncx,3] gets (x, y, response)
 * of the pixel of largest response among those with border <= x <= W-1-border, border <= y <= H-1-border,
 * d_mask[y][x] != 0 (d_mask [H,W] bytes or NULL) and response / 25 >= min_eig; ties go to the lowest row, then the
 * lowest column.  A cell without such a pixel, and every cell with d_cell_busy[cell] != 0 (d_cell_busy [ncy*ncx] bytes
 * or NULL), gets (-1, -1, 0).  One workgroup per cell: the products of the cell and its 2-pixel apron in LDS, an
 * order-fixed argmax (no float atomics; the result does not depend on launch order). */
int vipe_klt_detect(const float* d_img, int H, int W, const unsigned char* d_mask, const unsigned char* d_cell_busy,
                    int cell, int border, float min_eig, float* d_out, void* stream);

/* Tracks N points from pyramid A to pyramid B (both of H x W frames, L levels), coarse to fine, in one launch.
 * For p = d_pts[n], d = 0, and l = L-1 .. 0:
 *   c = p * 2^-l; for every window offset o in [-r, r]^2 (r = win_radius, 2 <= r <= 7):
 *     I(o) = S(A_l, c + o), gx(o) = 0.5*(S(A_l, c + o + (1,0)) - S(A_l, c + o - (1,0))), gy likewise with (0,1);
 *   G = (a, b, c) = sums of (gx*gx, gx*gy, gy*gy), det = a*c - b*b;
 *   n_iters times: e(o) = I(o) - S(B_l, (c + d) + o); (bx, by) = sums of (e*gx, e*gy);
 *     u = ((c*bx - b*by) / det, (a*by - b*bx) / det), or 0 unless det > 0; d += u;
 *     with eps > 0 the iterations of this level stop after the update with |u|^2 < eps^2 (eps = 0: exactly n_iters);
 *   OOB if c or q = c + d is not inside [border * 2^-l, (w_l - 1) - border * 2^-l] x [.., (h_l - 1) - ..];
 *   d *= 2 unless l == 0.
 * Then q = p + d -> d_out[n]; residual = sum |I(o) - S(B_0, q + o)| / (2r+1)^2 -> d_resid[n]; status bits OOB,
 * LOW_TEXTURE (G of level 0), RESIDUAL, DIVERGED (d not finite or |d|^2 > max_flow^2) and, with d_mask (the mask of
 * frame B, [H,W] bytes or NULL) and q rounded (floor(q + 0.5)) inside the image, MASKED.
 *   d_fb_ref == NULL (forward pass): d_status[n] = those bits.  d_cell_busy is not touched.
 *   d_fb_ref != NULL (backward pass: A and B swapped, d_pts the forward results, d_fb_ref [N,2] the original points,
 *     d_mask ignored): d_status[n] is READ, the bits of this pass are not added, VIPE_KLT_FB is added unless
 *     |q - d_fb_ref[n]|^2 <= fb_thresh^2, and the byte is written back.  If it is 0 and d_cell_busy != NULL
 *     ([ncy*ncx] bytes, cells of `cell` pixels as in vipe_klt_detect, 4 <= cell), the cell that holds d_pts[n] rounded
 *     is set to 1 (plain byte stores; racing writers store the same value).
 * d_out [N,2] f32, d_status [N] bytes, d_resid [N] f32.  N == 0: VIPE_OK, no launch.  Null pointers, r outside 2..7,
 * L outside 1..6, n_iters outside 1..100: VIPE_EINVAL.  One wave per point, four points per workgroup: the (2r+1)^2
 * window pixels are spread over the 64 lanes (up to four per lane), template and gradients stay in registers, the sums
 * go through cross-lane butterflies (every lane holds the same total); no LDS. */
int vipe_klt_track(const float* d_pyr_a, const float* d_pyr_b, int H, int W, int L, const float* d_pts, int N,
                   const float* d_fb_ref, const unsigned char* d_mask, int win_radius, int n_iters, float eps, int border,
                   float min_eig, float max_residual, float fb_thresh, float max_flow, int cell, float* d_out,
                   unsigned char* d_status, float* d_resid, unsigned char* d_cell_busy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VIPE_AMD_H */
