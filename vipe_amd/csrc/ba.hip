// Dense bundle adjustment on SE3 (+) per-pixel inverse depth (+ focal / distortion), Gauss-Newton with
// Schur reduction and a dense block Cholesky, entirely on the device.
//
// Replaces the reference's LIVE Python solver: GraphBuffer.bundle_adjustment (components/buffer.py:373-525)
// -> Solver.run_inplace (ba/solver.py:117-197) -> DenseDepthFlowTerm / DispSensRegularizationTerm
// (ba/terms.py:94-303) -> geom.iproj_i_proj_j_disp (maths/geom.py:187-298) -> block-sparse products with
// host round trips (maths/matrix.py:66-81) -> scipy spsolve on the CPU (solver.py:33-44).
//
// MI355X design (one GN iteration = accumulate, solve, retract; no host sync - what depends on the plan is decided on the
// device, so without a path hint the kernels of the paths not taken are launched too and exit at once):
//   ba_accum_mfma_kernel (source frames of <= 6 terms) / ba_walk_kernel + ba_schur_kernel (any degree)
//                     grid (pixel tiles, source frames).  One lane owns pixel p of source frame k and walks
//                     ALL terms (edges) whose source is k (device-built CSR), so the per-pixel quantities
//                     C_k, w_k, E_kk stay in registers and are final when the walk ends; Jacobians never
//                     touch memory.  J^T W J blocks are Gram matrices on the matrix cores (v_mfma_f32_16x16x4_f32),
//                     combined in LDS and added to the dense reduced system in fp64.  The Schur complement of
//                     frame k (all member pairs of k) is formed right after the walk.
//   solve             LM damping, right-looking block Cholesky in fp64 with the rhs carried as an extra matrix row
//                     (forward substitution for free), blocked backward substitution, pose / intrinsics / rig
//                     retraction.  One of four solvers takes the reduced system, by ba_route.cuh: ba_solve_band_kernel
//                     (banded, in LDS, one workgroup), ba_solve_dense_kernel (dense windows, LDS + registers, one
//                     workgroup), ba_solve_kernel (global memory, one workgroup) or the tiled chol_* kernels (chip wide).
//   ba_retract_kernel per pixel dz = (w - sum_a E_ak^T dx_a)/C, d += dz (dz > 10 rejected).
//
// One translation unit in parts, included below in this order inside the one anonymous namespace (the kernels take
// BAArgs by value and have internal linkage):
//   ba_common.cuh        constants, BAWs / BAArgs, carve, load_tw, valid_weight, term_setup, finish_disp, s_add, rsqrt_nr and
//                        what the four solvers share: readlane_f64, tri_index, damped_diag, store_step, apply_retraction
//   ba_route.cuh         which solver takes the reduced system: band_form, dense_takes, global_form and the limits behind them
//   ba_plan.inc          ba_sens_kernel, ba_plan_kernel
//   ba_accumulate.inc    the term walk written once (term_setup_m, walk_pixel, term_point_jacobians, walk_tile, gram_r1,
//                        flush_term_blocks, flush_frame_blocks, store_disp_block), then the three accumulate kernels
//                        that call it and ba_schur_kernel
//   ba_solve_band.inc    the block step over one LDS band image written once (BandImage: band_factor_diag, band_load_rows,
//                        BandPairs / band_pairs_setup, band_panel, band_trailing, band_backsub_block), the one-chain and
//                        two-chain bodies that call it, ba_solve_band_kernel
//   ba_solve_dense.inc   ba_solve_dense_kernel
//   ba_solve_global.inc  ba_solve_kernel + the tiled Cholesky     ba_retract.inc       ba_retract_kernel, clamp_min_kernel
//   ba_marginals.inc     ba_term_slot_kernel, ba_export_reduced_kernel, ba_disp_variance_kernel, ba_marginals_finish_kernel:
//                        marginal covariances from the blocks one linearisation leaves in the workspace
// This file keeps the overlap protocol, the <CAM, F> dispatch, launch_accumulate, run_iters, what the live entry points share
// (live_args, bind_arrays, check_live_call) and the exported entry points.
//
// Comments of the form `// @stamp N`, `// @stampk N`, `// @wstampk N`, `// @bstamp N`, `// @bwave N`, `// @astamp N`,
// `// @kstamp N` / `// @kstampc N` in the parts mark phase boundaries: scratch/make_ba_stamps.py expands the includes and
// turns the markers into s_memtime stores of a VARIANT source for cycle measurements from inside the kernels
// (scratch/README.md).  The product compiles none of it.
#include <stdlib.h>

#include "term_geom.cuh"

namespace {

#include "ba_common.cuh"
#include "ba_route.cuh"
#include "ba_plan.inc"
#include "ba_accumulate.inc"
#include "ba_solve_band.inc"
#include "ba_solve_dense.inc"
#include "ba_solve_global.inc"
#include "ba_retract.inc"
#include "ba_marginals.inc"

// Event `after the accumulate kernels of this iteration` on the BA stream; see overlap_piece
hipEvent_t overlap_event() {
  static thread_local hipEvent_t ev[64] = {};
  int d = 0;
  (void)hipGetDevice(&d);
  hipEvent_t& e = ev[d & 63];
  if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) e = nullptr;
  return e;
}

// vipe_overlap_fn protocol: piece `it` goes to the caller's stream behind the event after this iteration's accumulate
// kernels, i.e. it becomes eligible together with the single-workgroup solve
int overlap_piece(const vipe_ba_params& p, hipEvent_t ev, int piece, int n_pieces, bool gated) {
  hipStream_t side = (hipStream_t)p.overlap_stream;
  // (Rounds 2-3 put a 4 us wall-clock delay kernel behind the event so that the solve kernel would win the race for a free
  // CU.  Round 4 A/B on the headline, three runs each: 256.5 / 256.1 / 256.7 it/s with it, 257.5 / 256.5 / 257.9 without,
  // 254.4 / 253.6 / 254.8 with 16 us - the two-chain band solve and the staged share of 0.5 left nothing for it to fix.
  // Removed: the ordering is the event alone.)
  if (gated && ev && hipStreamWaitEvent(side, ev, 0) != hipSuccess) return VIPE_EINVAL;
  return p.overlap_fn(p.overlap_user, piece, n_pieces, p.overlap_stream);
}

// The <CAM, F> instantiation of a call: camera model and F = shared intrinsics unknowns of a mono system (1 + D when
// optimize_intrinsics, else 0; the panorama has no intrinsics - check_live_call).  fn(CamF<CAM, F>{}) is called with the
// one that applies.
template <int CAM_, int F_>
struct CamF { static constexpr int CAM = CAM_, F = F_; };
template <class Fn>
auto with_cam_f(const BAArgs& a, Fn&& fn) {
  const bool intr = a.p.optimize_intrinsics != 0;
  if (a.p.camera == VIPE_CAM_PINHOLE) return intr ? fn(CamF<VIPE_CAM_PINHOLE, 1>{}) : fn(CamF<VIPE_CAM_PINHOLE, 0>{});
  if (a.p.camera == VIPE_CAM_PANORAMA) return fn(CamF<VIPE_CAM_PANORAMA, 0>{});
  return intr ? fn(CamF<VIPE_CAM_MEI, 2>{}) : fn(CamF<VIPE_CAM_MEI, 0>{});
}

// the accumulate kernels of one linearisation (path_hint: what the caller learnt from an earlier call with this plan; 0
// launches both paths and the inapplicable one exits at once)
void launch_accumulate(const BAArgs& a, hipStream_t s) {
  with_cam_f(a, [&](auto c) {
    constexpr int CAM = decltype(c)::CAM, F = decltype(c)::F;
    const int tiles = (a.P + TILE - 1) / TILE;
    static std::atomic<uint64_t> tmpl_set{0};  // one per <CAM, F> instantiation of this lambda
    vipe_once_per_device(tmpl_set, [] {
      (void)hipFuncSetAttribute((const void*)ba_accum_mfma_kernel<CAM, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)accum_mfma_lds());
      (void)hipFuncSetAttribute((const void*)ba_walk_kernel<CAM, F>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)walk_lds());
      (void)hipFuncSetAttribute((const void*)ba_walk_rig_kernel<CAM, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)walk_rig_lds());
      (void)hipFuncSetAttribute((const void*)ba_walk_rig_kernel<CAM, RG_VMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)walk_rig_lds());
    });
    if (a.mv) {
      // multi-view rigs: local-block walk, Schur Gram over the stacked E rows
      if (a.p.n_views <= 4) ba_walk_rig_kernel<CAM, 4><<<dim3(tiles, a.nF), TILE, walk_rig_lds(), s>>>(a);
      else ba_walk_rig_kernel<CAM, RG_VMAX><<<dim3(tiles, a.nF), TILE, walk_rig_lds(), s>>>(a);
      ba_schur_kernel<0><<<dim3(SC_GRID, a.nF), TILE, 0, s>>>(a);
      return;
    }
    const int hint = a.force_general ? 0 : a.p.path_hint;
    if (!(hint & 2)) ba_accum_mfma_kernel<CAM, F><<<dim3(tiles, a.nF), TILE, accum_mfma_lds(), s>>>(a);
    if (!(hint & 1)) {
      ba_walk_kernel<CAM, F><<<dim3(tiles, a.nF), TILE, walk_lds(), s>>>(a);
      ba_schur_kernel<F><<<dim3(SC_GRID, a.nF), TILE, 0, s>>>(a);
    }
  });
}

int run_iters(const BAArgs& a, hipStream_t s, int* pieces_done) {
  const int tiles = (a.P + TILE - 1) / TILE;
  const size_t sbytes = sizeof(double) * (size_t)a.w.ld * a.w.ld;
  const size_t nmax = (size_t)a.w.ld - 1;
  // LDS panel of the solve kernel: [NB][panel_cap] doubles next to the fixed part, up to ~150 KB.  ba_solve_kernel keeps
  // the n + 1 panel rows of a system there without testing: n <= nmax, and n <= CT_MIN_N by its route
  constexpr size_t fixed = ((sizeof(SolveLds) + 15) / 16) * 16;
  constexpr size_t panel_lds_rows = (150 * 1024 - fixed) / (NB * sizeof(double));
  static_assert(CT_MIN_N + 1 <= panel_lds_rows, "ba_solve_kernel: the panel of its largest system must fit the LDS buffer");
  int panel_cap = (int)std::min<size_t>(nmax + 1, panel_lds_rows);
  panel_cap = (panel_cap + 3) & ~3;
  const size_t solve_lds = fixed + (size_t)NB * panel_cap * sizeof(double);
  const size_t band_lds = SOLVER_LDS_DOUBLES * sizeof(double);  // the size the route (ba_route.cuh) counts on
  static std::atomic<uint64_t> attr_set{0};  // bit d: set on device d
  vipe_once_per_device(attr_set, [] {
    (void)hipFuncSetAttribute((const void*)ba_solve_band_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)ba_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)ba_solve_dense_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipFuncSetAttribute((const void*)chol_backsub_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  });
  // S / Hd start each accumulation zeroed: by ba_retract_kernel of the previous iteration when it runs (not motion_only),
  // also across calls when the caller vouches for the workspace (reuse_plan: same key, hence the same motion_only), else
  // by memsets
  const bool retract_clears = !a.p.motion_only;
  const bool overlap = a.p.overlap_stream && a.p.overlap_fn;
  hipEvent_t ev = overlap ? overlap_event() : nullptr;
  // path_hint (vipe_ba_params): what the caller learnt from an earlier call with this plan; 0 launches everything.
  // Multi-view rigs: the route gives them to the global solver, so only that one is launched
  const int hint = a.mv ? 8 | 16 : (a.force_general ? 0 : a.p.path_hint);
  for (int it = 0; it < a.p.n_iters; ++it) {
    if (!(retract_clears && (it > 0 || a.p.reuse_plan))) {
      hipError_t e1 = hipMemsetAsync(a.w.S, 0, sbytes, s);
      hipError_t e2 = hipMemsetAsync(a.w.Hd, 0, sizeof(double) * nmax, s);
      if (e1 != hipSuccess || e2 != hipSuccess) return (int)(e1 != hipSuccess ? e1 : e2);
    }
    const bool prof = a.p.profile_ev0 && a.p.profile_ev1 &&
                      it == (a.p.profile_iter < 0 || a.p.profile_iter >= a.p.n_iters ? a.p.n_iters - 1 : a.p.profile_iter);
    if (prof && hipEventRecord((hipEvent_t)a.p.profile_ev0, s) != hipSuccess) return VIPE_EINVAL;
    launch_accumulate(a, s);
    if (prof && hipEventRecord((hipEvent_t)a.p.profile_ev1, s) != hipSuccess) return VIPE_EINVAL;
    if (ev && hipEventRecord(ev, s) != hipSuccess) return VIPE_EINVAL;
    if (!(hint & 8)) ba_solve_band_kernel<<<1, 2 * BAND_T, band_lds, s>>>(a, SOLVER_LDS_DOUBLES);
    if (!(hint & 16)) ba_solve_dense_kernel<<<1, DN_T, band_lds, s>>>(a, SOLVER_LDS_DOUBLES);
    if (!(hint & 4)) {
      ba_solve_kernel<<<1, SOLVE_T, solve_lds, s>>>(a, panel_cap);
      launch_tiled_cholesky(a, s);
    }
    if (overlap) {
      const int rc = overlap_piece(a.p, ev, it, a.p.n_iters, true);
      if (rc != VIPE_OK) return rc;
      ++*pieces_done;
    }
    // the tail of a rig is not the F shared intrinsics of a mono system: ba_retract_kernel<0>
    if (!a.p.motion_only)
      with_cam_f(a, [&](auto c) {
        if (a.mv) ba_retract_kernel<0><<<dim3(tiles, a.nF), TILE, 0, s>>>(a);
        else ba_retract_kernel<decltype(c)::F><<<dim3(tiles, a.nF), TILE, 0, s>>>(a);
      });
  }
  return vipe_launch_status();
}

// what the entry points derive from the parameters alone (array pointers and the workspace are the caller's to fill)
void live_args(BAArgs& a, const vipe_ba_params& p) {
  a.p = p;
  a.P = p.ht * p.wd;
  a.nF = p.n_poses * p.n_views;
  a.D = p.camera == VIPE_CAM_MEI ? 1 : 0;
  a.mv = is_multiview(p) ? 1 : 0;
  a.nintr = tail_intr(p);
  a.ntail = a.nintr + tail_rig(p);
  a.force_general = (p.solver_options & VIPE_BA_OPT_GENERAL_ACCUMULATE) != 0;
  a.band2 = !(p.solver_options & VIPE_BA_OPT_ONE_CHAIN);
  a.droid = 0;
  a.dz_out = nullptr;
}

void bind_arrays(BAArgs& a, float* poses, float* disps, float* intr, float* rig, const float* sens, const float* target,
                 const float* weight, const float* eta, const int64_t* pi, const int64_t* qi, const int64_t* pj,
                 const int64_t* qj, const int64_t* di) {
  a.poses = poses; a.disps = disps; a.intr = intr; a.rig = rig;
  a.sens = sens; a.target = target; a.weight = weight; a.eta = eta;
  a.pi = pi; a.qi = qi; a.pj = pj; a.qj = qj; a.di = di;
}

// The parameters of a live call.  a: what bind_arrays bound, for a call that reads the state and the terms (null:
// vipe_dense_ba_marginals); iterates: n_iters counts (vipe_dense_ba)
int check_live_call(const vipe_ba_params& p, const BAArgs* a, bool iterates) {
  VIPE_CHECK_ARG(p.camera == VIPE_CAM_PINHOLE || p.camera == VIPE_CAM_MEI || p.camera == VIPE_CAM_PANORAMA);
  VIPE_CHECK_ARG(!(p.camera == VIPE_CAM_PANORAMA && p.optimize_intrinsics));  // the panorama has none; its row is never read
  VIPE_CHECK_ARG(!a || (a->poses && a->disps && a->sens && a->intr && a->rig && a->eta));
  VIPE_CHECK_ARG(p.n_poses > 0 && p.n_views > 0 && p.ht > 0 && p.wd > 0 && p.M >= 0 && !(iterates && p.n_iters < 0));
  VIPE_CHECK_ARG(!a || (p.t0 <= p.t1 && p.intr_factor > 0));
  VIPE_CHECK_ARG(!a || p.M == 0 || (a->target && a->weight && a->pi && a->qi && a->pj && a->qj && a->di));
  if (is_multiview(p) && p.n_views > RG_VMAX) return VIPE_EUNSUPPORTED;  // rigs of up to 8 cameras
  if ((int64_t)p.n_poses * p.n_views > 65535) return VIPE_EINVAL;
  return VIPE_OK;
}

}  // namespace

VIPE_EXPORT int64_t vipe_dense_ba_workspace_bytes(const vipe_ba_params* p) {
  if (!p || p->n_poses <= 0 || p->n_views <= 0 || p->ht <= 0 || p->wd <= 0 || p->M < 0) return VIPE_EINVAL;
  return (int64_t)carve(*p, nullptr, nullptr);
}

VIPE_EXPORT int vipe_dense_ba(const vipe_ba_params* p, float* d_poses, float* d_disps, const float* d_disps_sens,
                              float* d_intrinsics, float* d_rig, const float* d_target, const float* d_weight,
                              const float* d_disp_damping, const int64_t* d_pi, const int64_t* d_qi,
                              const int64_t* d_pj, const int64_t* d_qj, const int64_t* d_di, void* d_workspace,
                              int64_t workspace_bytes, int* d_info, void* stream) {
  VIPE_CHECK_ARG(p && d_workspace);
  BAArgs a = {};
  bind_arrays(a, d_poses, d_disps, d_intrinsics, d_rig, d_disps_sens, d_target, d_weight, d_disp_damping, d_pi, d_qi, d_pj,
              d_qj, d_di);
  int rc = check_live_call(*p, &a, true);
  if (rc != VIPE_OK) return rc;
  live_args(a, *p);
  if ((int64_t)carve(*p, (char*)d_workspace, &a.w) > workspace_bytes) return VIPE_ENOSPACE;
  hipStream_t s = as_stream(stream);
  int pieces_done = 0;
  if (p->M > 0 && p->n_iters > 0) {
    ba_sens_kernel<<<a.nF, 256, 0, s>>>(d_disps_sens, a.w.sens_sum, a.P, a.w.info);
    if (!p->reuse_plan) ba_plan_kernel<<<1, 1024, 0, s>>>(a);
    rc = run_iters(a, s, &pieces_done);
    if (rc != VIPE_OK) return rc;
    if (d_info) {
      hipError_t e = hipMemcpyAsync(d_info, a.w.info, 8 * sizeof(int), hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) return (int)e;
    }
  }
  // vipe_overlap_fn: exactly max(n_iters, 1) pieces, also when there was nothing to optimise
  if (p->overlap_stream && p->overlap_fn) {
    const int n_pieces = p->n_iters > 0 ? p->n_iters : 1;
    for (; pieces_done < n_pieces; ++pieces_done) {
      rc = overlap_piece(*p, nullptr, pieces_done, n_pieces, false);
      if (rc != VIPE_OK) return rc;
    }
  }
  // buffer.py:525: disps.clamp_(min=1e-3) over the whole buffer handed in
  const int64_t nd = (int64_t)a.nF * a.P;
  clamp_min_kernel<<<(int)std::min<int64_t>((nd + 255) / 256, 2048), 256, 0, s>>>(d_disps, nd, 1e-3f);
  return vipe_launch_status();
}

// ---- marginal covariances of the live dense BA (ba_marginals.inc).  Two calls with the caller's inverse of the reduced
// system in between: linearize leaves C / E_kk / E_j / E_f / E_t and the undamped S, Hd in the workspace and hands out the
// damped symmetric S; marginals reads them with S^-1 and zeroes S / Hd again.
VIPE_EXPORT int vipe_dense_ba_linearize(const vipe_ba_params* p, const float* d_poses, const float* d_disps,
                                        const float* d_disps_sens, const float* d_intrinsics, const float* d_rig,
                                        const float* d_target, const float* d_weight, const float* d_disp_damping,
                                        const int64_t* d_pi, const int64_t* d_qi, const int64_t* d_pj, const int64_t* d_qj,
                                        const int64_t* d_di, void* d_workspace, int64_t workspace_bytes, double* d_S_out,
                                        int ld_out, int* d_info, void* stream) {
  VIPE_CHECK_ARG(p && d_workspace && d_S_out);
  BAArgs a = {};
  // the kernels are shared with the solver and take the state as mutable; nothing launched here writes it
  bind_arrays(a, const_cast<float*>(d_poses), const_cast<float*>(d_disps), const_cast<float*>(d_intrinsics),
              const_cast<float*>(d_rig), d_disps_sens, d_target, d_weight, d_disp_damping, d_pi, d_qi, d_pj, d_qj, d_di);
  const int rc = check_live_call(*p, &a, false);
  if (rc != VIPE_OK) return rc;
  live_args(a, *p);
  if ((int64_t)carve(*p, (char*)d_workspace, &a.w) > workspace_bytes) return VIPE_ENOSPACE;
  VIPE_CHECK_ARG(ld_out >= 6 * p->n_poses + a.ntail);  // the bound carve sizes S by; n = info[INFO_UNKNOWNS] rows are written
  hipStream_t s = as_stream(stream);
  ba_sens_kernel<<<a.nF, 256, 0, s>>>(d_disps_sens, a.w.sens_sum, a.P, a.w.info);
  if (!(p->reuse_plan && p->M > 0)) ba_plan_kernel<<<1, 1024, 0, s>>>(a);
  if (!(p->reuse_plan && !p->motion_only && p->M > 0)) {  // as run_iters: a vouched-for workspace holds S = Hd = 0
    hipError_t e1 = hipMemsetAsync(a.w.S, 0, sizeof(double) * (size_t)a.w.ld * a.w.ld, s);
    hipError_t e2 = hipMemsetAsync(a.w.Hd, 0, sizeof(double) * ((size_t)a.w.ld - 1), s);
    if (e1 != hipSuccess || e2 != hipSuccess) return (int)(e1 != hipSuccess ? e1 : e2);
  }
  if (p->M > 0) {
    ba_term_slot_kernel<<<(p->M + 255) / 256, 256, 0, s>>>(a);
    launch_accumulate(a, s);
  }
  const int64_t nn = (int64_t)(a.w.ld - 1) * (a.w.ld - 1);
  ba_export_reduced_kernel<<<(int)std::min<int64_t>((nn + 255) / 256, 2048), 256, 0, s>>>(a, d_S_out, ld_out);
  if (d_info) {
    hipError_t e = hipMemcpyAsync(d_info, a.w.info, 8 * sizeof(int), hipMemcpyDeviceToDevice, s);
    if (e != hipSuccess) return (int)e;
  }
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_dense_ba_marginals(const vipe_ba_params* p, void* d_workspace, const double* d_Sinv, int ld,
                                        float* d_disp_var, double* d_pose_cov, void* stream) {
  VIPE_CHECK_ARG(p && d_workspace && ld >= 0);
  const int rc = check_live_call(*p, nullptr, false);
  if (rc != VIPE_OK) return rc;
  BAArgs a = {};
  live_args(a, *p);
  carve(*p, (char*)d_workspace, &a.w);
  hipStream_t s = as_stream(stream);
  const int tiles = (a.P + TILE - 1) / TILE;
  // no free disparity without terms or under motion_only; no unknowns (ld == 0): the caller has no inverse to hand in
  if (p->M > 0 && !p->motion_only && d_disp_var) {
    VIPE_CHECK_ARG(d_Sinv || ld == 0);
    ba_disp_variance_kernel<<<dim3(tiles, a.nF), TILE, 0, s>>>(a, d_Sinv, ld, d_disp_var);
  }
  const int64_t ns = (int64_t)a.w.ld * a.w.ld;
  ba_marginals_finish_kernel<<<(int)std::min<int64_t>((ns + 255) / 256, 2048), 256, 0, s>>>(a, ld > 0 ? d_Sinv : nullptr, ld, d_pose_cov);
  return vipe_launch_status();
}

// ---- slam_ext.ba with the DROID signature (dormant in the reference; geom_kernels.cu:1273-1404).  Same kernels as the
// live dense BA with the DROID semantics switched on (BAArgs::droid; oracle/droid_ba.py lists the differences).
namespace {
size_t droid_extra_bytes(int E) { return align_up(8 * (size_t)(E + 1)) + align_up(7 * 4); }
vipe_ba_params droid_params(int n_poses, int ht, int wd, int E, int t0, int t1, int iterations, float lm, float ep,
                            int motion_only) {
  vipe_ba_params p = {};
  p.n_poses = n_poses; p.n_views = 1; p.ht = ht; p.wd = wd; p.M = E; p.t0 = t0; p.t1 = t1; p.n_iters = iterations;
  p.pose_damping = lm; p.pose_ep = ep; p.motion_only = motion_only; p.limited_disp = 0; p.optimize_intrinsics = 0;
  p.optimize_rig_rotation = 0; p.camera = VIPE_CAM_PINHOLE; p.alpha = 0.05f; p.weight_scale = 0.001f; p.intr_factor = 1.0f;
  p.reuse_plan = 0; p.path_hint = 0;
  return p;
}
}  // namespace

VIPE_EXPORT int64_t vipe_ba_workspace_bytes(int n_poses, int ht, int wd, int E) {
  if (n_poses <= 0 || ht <= 0 || wd <= 0 || E < 0) return VIPE_EINVAL;
  const vipe_ba_params p = droid_params(n_poses, ht, wd, E, 0, 0, 0, 0.f, 0.f, 0);
  return (int64_t)(carve(p, nullptr, nullptr) + droid_extra_bytes(E));
}

VIPE_EXPORT int vipe_ba(float* d_poses, float* d_disps, const float* d_intrinsics, const float* d_disps_sens,
                        const float* d_targets, const float* d_weights, const float* d_eta, const int64_t* d_ii,
                        const int64_t* d_jj, int n_poses, int ht, int wd, int E, int n_eta, int t0, int t1,
                        int iterations, float lm, float ep, int motion_only, float* d_dx, float* d_dz,
                        void* d_workspace, int64_t workspace_bytes, void* stream) {
  VIPE_CHECK_ARG(d_poses && d_disps && d_intrinsics && d_disps_sens && d_eta && d_workspace && d_dx && d_dz);
  VIPE_CHECK_ARG(n_poses > 0 && ht > 0 && wd > 0 && E >= 0 && iterations >= 0 && n_eta >= 0);
  VIPE_CHECK_ARG(0 <= t0 && t0 <= t1 && t1 <= n_poses);
  VIPE_CHECK_ARG(E == 0 || (d_targets && d_weights && d_ii && d_jj));
  if (n_poses > 65535) return VIPE_EINVAL;
  // the DROID differences: BAArgs::droid with its dz output; qi = qj = 0 and di = ii (one view), an identity rig
  BAArgs a = {};
  live_args(a, droid_params(n_poses, ht, wd, E, t0, t1, iterations, lm, ep, motion_only));
  a.droid = 1;
  a.dz_out = d_dz;
  const size_t base = carve(a.p, (char*)d_workspace, &a.w);
  if ((int64_t)(base + droid_extra_bytes(E)) > workspace_bytes) return VIPE_ENOSPACE;
  int64_t* zeros = (int64_t*)((char*)d_workspace + base);
  float* rig = (float*)((char*)d_workspace + base + align_up(8 * (size_t)(E + 1)));
  hipStream_t s = as_stream(stream);
  const float rig_id[7] = {0, 0, 0, 0, 0, 0, 1};
  hipError_t e0 = hipMemsetAsync(zeros, 0, 8 * (size_t)(E + 1), s);
  hipError_t e1 = hipMemcpyAsync(rig, rig_id, sizeof(rig_id), hipMemcpyHostToDevice, s);
  const int64_t P = (int64_t)ht * wd;
  hipError_t e2 = hipMemsetAsync(d_dx, 0, sizeof(float) * 6 * (size_t)(t1 - t0), s);
  hipError_t e3 = hipMemsetAsync(d_dz, 0, sizeof(float) * (size_t)n_eta * P, s);
  if (e0 != hipSuccess || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return VIPE_EINVAL;
  bind_arrays(a, d_poses, d_disps, (float*)d_intrinsics, rig, d_disps_sens, d_targets, d_weights, d_eta, d_ii, zeros, d_jj,
              zeros, d_ii);
  if (iterations == 0 || t1 == t0) return VIPE_OK;
  ba_sens_kernel<<<a.nF, 256, 0, s>>>(d_disps_sens, a.w.sens_sum, a.P, a.w.info);
  ba_plan_kernel<<<1, 1024, 0, s>>>(a);
  int pieces_done = 0;
  const int rc = run_iters(a, s, &pieces_done);
  if (rc != VIPE_OK) return rc;
  hipError_t e4 = hipMemcpyAsync(d_dx, a.w.dx, sizeof(float) * 6 * (size_t)(t1 - t0), hipMemcpyDeviceToDevice, s);
  return e4 == hipSuccess ? vipe_launch_status() : (int)e4;
}
