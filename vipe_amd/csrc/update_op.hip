// The flow-update operator (UpdateModule.forward, vipe/slam/networks/droid_net.py:467-499) as ONE library call.
//
// The operator is a dozen fused convolutions + a segmented mean + two small reductions (csrc/conv_mfma.hip, corr_lookup.hip,
// aux_ops.hip).  Issued one by one from Python each launch costs 10-15 us of argument marshalling, more than most of
// these kernels run for on a frontend window (~48 edges): the keyframe frontend was launch bound (GPU idle 15-45 % of
// the time, profiles/r02_video_*).  vipe_update_operator sequences them natively from two descriptor structs the host
// fills once per operator / per edge set; vipe_update_finish is the tail of FactorGraph.update (factor_graph.py:
// 270-276: target = coords1 + delta, weight with masked frames zeroed, damping[source frames] = eta) as one kernel
// instead of five elementwise launches.
#include "common.cuh"
#include "conv_call.cuh"

namespace {

// extra[e, :] = glo_b + (glo_sum[e, :] / HW) @ glo_w   ([E,128] x [128,384]): the three *_glo 1x1 convolutions of the
// ConvGRU applied to the pooled context vector (droid_net.py:392-399)
__global__ __launch_bounds__(384) void glo_gemm_kernel(const float* __restrict__ glo, const float* __restrict__ wT /* [128][384] */,
                                                       const float* __restrict__ b, float* __restrict__ extra, float inv_hw) {
  __shared__ float g[128];
  const int e = blockIdx.x, t = threadIdx.x;
  if (t < 128) g[t] = glo[(int64_t)e * 128 + t] * inv_hw;
  __syncthreads();
  float acc = b[t];
#pragma unroll 8
  for (int k = 0; k < 128; ++k) acc = __builtin_fmaf(g[k], wT[k * 384 + t], acc);
  extra[(int64_t)e * 384 + t] = acc;
}

__global__ __launch_bounds__(256) void update_finish_kernel(const float* __restrict__ coords1, const float* __restrict__ dw,
                                                            const unsigned char* __restrict__ mask, float* __restrict__ target,
                                                            float* __restrict__ weight, const float* __restrict__ eta,
                                                            const int64_t* __restrict__ du, float* __restrict__ damping,
                                                            int64_t n_px, int64_t n_eta, int P) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_px) {
    const float2 c = reinterpret_cast<const float2*>(coords1)[i];
    const float4 d = reinterpret_cast<const float4*>(dw)[i];
    const bool m = mask && mask[i];
    reinterpret_cast<float2*>(target)[i] = make_float2(c.x + d.x, c.y + d.y);
    reinterpret_cast<float2*>(weight)[i] = m ? make_float2(0.f, 0.f) : make_float2(d.z, d.w);
  }
  if (i < n_eta) damping[du[i / P] * P + i % P] = eta[i];
}

// four events per (thread, device) for the fork / join of the operator's two-stream form
hipEvent_t* operator_events() {
  static thread_local hipEvent_t ev[64][4] = {};
  int d = 0;
  (void)hipGetDevice(&d);
  hipEvent_t* e = ev[d & 63];
  for (int i = 0; i < 4; ++i)
    if (!e[i] && hipEventCreateWithFlags(&e[i], hipEventDisableTiming) != hipSuccess) return nullptr;
  return e;
}

// The schedule below is straight-line code over ConvCall descriptors (conv_call.cuh): every launch names the operands it
// has, vipe_conv_run validates and dispatches it.  The launches carry the names of oracle/conv_epilogue_cases.py::LAUNCHES;
// tests/host/operator_trace.cpp prints the whole sequence on a machine without a GPU.
struct Grid { int B, H, W; };
#define RUN(call) \
  do { const int rc_ = (call); if (rc_ != VIPE_OK) return rc_; } while (0)

// k x k, Cin -> Cout over `g`, every input channel from x0: what each launch has; the rest by name at the call site
ConvCall conv(Grid g, ConvView x0, int Cin, const void* w, const float* bias, int Cout, int k) {
  ConvCall c;
  c.x0 = x0; c.w = w; c.bias = bias;
  c.B = g.B; c.H = g.H; c.W = g.W; c.Cin = Cin; c.Cout = Cout; c.KH = c.KW = k;
  return c;
}

// y = relu(conv + bias): the encoders, heads0 and agg2
int relu_conv(Grid g, ConvView x0, int Cin, const void* w, const float* bias, int Cout, int k, ConvView y, hipStream_t st) {
  ConvCall c = conv(g, x0, Cin, w, bias, Cout, k);
  c.y = y; c.act = VIPE_ACT_RELU;
  return vipe_conv_run(c, st);
}

// global context of hidden state `net` (droid_net.py:392-393) and its three 1x1s: glo, extra.  The operator's own stage
// and part 1 of vipe_update_gate_state
int global_context(const vipe_update_weights* wt, const vipe_update_buffers* b, const void* net, hipStream_t s) {
  if (hipMemsetAsync(b->glo, 0, sizeof(float) * 128 * (size_t)b->E, s) != hipSuccess) return VIPE_EINVAL;
  ConvCall c = conv({b->E, b->H, b->W}, {net, 128, 0}, 128, wt->gw_w, wt->gw_b, 128, 1);  // glo_net
  c.epi = EPI_GLO; c.net = c.x0; c.fout = b->glo;
  RUN(vipe_conv_run(c, s));
  glo_gemm_kernel<<<b->E, 384, 0, s>>>(b->glo, wt->glo_wT, wt->glo_b, b->extra, 1.0f / (float)(b->H * b->W));
  return VIPE_OK;
}
}  // namespace

extern "C" {

VIPE_EXPORT int vipe_update_operator(const vipe_update_weights* wt, const vipe_update_buffers* b, void* stream) {
  VIPE_CHECK_ARG(wt && b && b->E >= 0 && b->H > 0 && b->W > 0);
  if (b->E == 0) return VIPE_OK;
  const int E = b->E, H = b->H, W = b->W;
  const Grid g = {E, H, W};
  hipStream_t s = as_stream(stream);
  // two-stream form: s2 carries the flow encoder next to the lookup + correlation encoder, and the GraphAgg chain next to the heads
  hipStream_t s2 = (hipStream_t)b->side_stream;
  hipEvent_t* ev = s2 ? operator_events() : nullptr;
  if (s2 && !ev) return VIPE_EINVAL;
  hipStream_t side = s2 ? s2 : s;
  auto fork = [&](int i) { return !s2 || (hipEventRecord(ev[i], s) == hipSuccess && hipStreamWaitEvent(s2, ev[i], 0) == hipSuccess); };
  auto join = [&](int i) { return !s2 || (hipEventRecord(ev[i], s2) == hipSuccess && hipStreamWaitEvent(s, ev[i], 0) == hipSuccess); };
  VIPE_CHECK_ARG(fork(0));
  // encoders (droid_net.py:481-482)
  if (b->levels[0]) {
    // with a side stream the lookup leaves half of every CU to the flow encoder
    RUN(vipe_corr_lookup_conv1x1_ex(b->levels, b->coords, wt->corr0_w, wt->corr0_b, b->c1, 128, 0, E, H, W, b->h2, b->w2, 128,
                                    VIPE_ACT_RELU, b->slots, b->pyramid_layout, stream, 0, s2 ? 1 : 0));
  } else {
    VIPE_CHECK_ARG(b->corr);
    RUN(relu_conv(g, {b->corr, 200, 0}, 200, wt->corr0_w, wt->corr0_b, 128, 1, {b->c1, 128, 0}, s));
  }
  RUN(relu_conv(g, {b->c1, 128, 0}, 128, wt->corr2_w, wt->corr2_b, 128, 3, {b->xbuf, 320, 128}, s));    // plain_corr2
  RUN(relu_conv(g, {b->motn, 4, 0}, 4, wt->flow0_w, wt->flow0_b, 128, 7, {b->f1, 128, 0}, side));
  RUN(relu_conv(g, {b->f1, 128, 0}, 128, wt->flow2_w, wt->flow2_b, 64, 3, {b->xbuf, 320, 256}, side));  // plain_flow2
  VIPE_CHECK_ARG(join(1));
  const int Es = b->gate_state;  // leading edges with the hidden-state part of z|r computed ahead (vipe_update_gate_state)
  if (Es != 0) VIPE_CHECK_ARG(Es > 0 && Es <= E && b->pgate && b->pzr && wt->zr_x_w);
  else RUN(global_context(wt, b, b->net, s));
  // gates (droid_net.py:395-399): z|r, then q.  Three forms, by what the accumulators start from:
  //   zr, q          nothing: [net or r * net | inp, corr, flow], 448 input channels;
  //   zr_ctx, q_ctx  pgate, the context-feature (inp) part: [net or r * net | corr, flow], 320 channels, their own weights;
  //   zr_staged      pzr (fp32), the inp and the hidden-state part, for edges [0, Es): (corr | flow) alone, 192 channels;
  //                  edges [Es, E) of a partly staged state take zr_ctx, and q is q_ctx.
  const bool ctx = b->pgate != nullptr;
  const int gate_cin = ctx ? 320 : 448, rest_coff = ctx ? 128 : 0;
  auto zr = [&](int e0, int n, bool staged) -> int {  // edges [e0, e0 + n)
    auto at = [&](const void* p, int ctot, int coff) { return ConvView{(const char*)p + (int64_t)e0 * H * W * ctot * 2, ctot, coff}; };
    ConvCall c;
    if (staged) {
      c = conv({n, H, W}, at(b->xbuf, 320, 128), 192, wt->zr_x_w, wt->zr_b, 256, 3);
      c.accinit = {b->pzr + (int64_t)e0 * H * W * 256, 256, 0}; c.accinit_f32 = true;
    } else {
      c = conv({n, H, W}, at(b->net, 128, 0), gate_cin, ctx ? wt->zr_s_w : wt->zr_w, wt->zr_b, 256, 3);
      c.x1 = at(b->xbuf, 320, rest_coff); c.split = 128;
      if (ctx) c.accinit = at(b->pgate, 384, 0);
    }
    c.epi = EPI_ZR; c.extra = b->extra + (int64_t)e0 * 384; c.extra_stride = 384;
    c.y = at(b->zb, 128, 0); c.y2 = at(b->rnet, 128, 0); c.net = at(b->net, 128, 0);
    return vipe_conv_run(c, s);
  };
  if (Es != 0) RUN(zr(0, Es, true));
  if (Es < E) RUN(zr(Es, E - Es, false));
  ConvCall q = conv(g, {b->rnet, 128, 0}, gate_cin, ctx ? wt->q_s_w : wt->q_w, wt->q_b, 128, 3);
  q.x1 = {b->xbuf, 320, rest_coff}; q.split = 128;
  if (ctx) q.accinit = {b->pgate, 384, 256};
  q.epi = EPI_Q; q.extra = b->extra; q.extra_stride = 384; q.extra_off = 256;
  q.y = {b->net_out, 128, 0}; q.net = {b->net, 128, 0}; q.z = b->zb;
  RUN(vipe_conv_run(q, s));
  // heads + first aggregation conv on net' (droid_net.py:486-487, 418): hbuf = relu(delta0 | weight0 | agg1)
  const bool two_tails = s2 && b->n_src > 0;
  const bool by_consumer = wt->agg1_w && wt->agg1_b && wt->heads_dw_w && wt->heads_dw_b;
  auto heads0 = [&](const void* w, const float* bias, int coff, int cout) -> int {  // plain_heads0, or a channel slice of it
    return relu_conv(g, {b->net_out, 128, 0}, 128, w, bias, cout, 3, {b->hbuf, 384, coff}, s);
  };
  // scatter_mean over the edges of each source node (droid_net.py:420-421), agg conv 2, eta (:422-429)
  auto agg_chain = [&](hipStream_t st) -> int {
    if (b->n_src <= 0) return VIPE_OK;
    VIPE_CHECK_ARG(b->order && b->rowptr && b->agg && b->a2 && b->eta);
    const Grid gs = {b->n_src, H, W};
    RUN(vipe_segment_mean_nhwc_f16(b->hbuf, 384, 256, b->order, b->rowptr, b->agg, b->n_src, (int64_t)H * W, 128, st));
    RUN(relu_conv(gs, {b->agg, 128, 0}, 128, wt->agg2_w, wt->agg2_b, 128, 3, {b->a2, 128, 0}, st));
    ConvCall c = conv(gs, {b->a2, 128, 0}, 128, wt->eta_w, wt->eta_b, 1, 3);  // eta
    c.epi = EPI_ETA; c.fout = b->eta;
    return vipe_conv_run(c, st);
  };
  auto heads2 = [&](hipStream_t st) -> int {  // heads
    ConvCall c = conv(g, {b->hbuf, 384, 0}, 256, wt->heads2_w, wt->heads2_b, 4, 3);
    c.epi = EPI_HEADS; c.fout = b->dw;
    return vipe_conv_run(c, st);
  };
  if (by_consumer && two_tails) {
    // heads0 split by consumer.  The GraphAgg chain needs only channels 256..383: they come first, and the chain runs
    // on the side stream beside the 256 channels of the flow / weight heads instead of behind all 384.  Same kernels
    // per 128-channel slice, so every result of the unfused heads is bit-identical to the one 384-channel launch.
    RUN(heads0(wt->agg1_w, wt->agg1_b, 256, 128));
    VIPE_CHECK_ARG(fork(2));
    RUN(agg_chain(side));
    if (wt->heads2_frag && b->hborder && vipe_heads_fused_ok(H, W)) {
      // grids of 4 x 64 tiles: heads2 contracted in the epilogue of delta0 | weight0 - hbuf[..., 0:256] is never written
      ConvCall c = conv(g, {b->net_out, 128, 0}, 128, wt->heads_dw_w, wt->heads_dw_b, 256, 3);
      c.act = VIPE_ACT_RELU; c.epi = EPI_HEADS_FUSED; c.heads2_frag = wt->heads2_frag; c.border = b->hborder; c.fout = b->dw;
      RUN(vipe_conv_run(c, s));
      RUN(vipe_heads_finish(b->dw, b->hborder, wt->heads2_b, E, H, W, stream));
    } else {
      RUN(heads0(wt->heads_dw_w, wt->heads_dw_b, 0, 256));
      RUN(heads2(s));
    }
  } else {
    // one stream (frontend windows, E < 64) or no chain: the one 384-channel launch - three launches of 128 + 256
    // channels leave more partly filled workgroup rounds than one, with nothing to run beside them
    RUN(heads0(wt->heads0_w, wt->heads0_b, 0, 384));
    if (two_tails) VIPE_CHECK_ARG(fork(2));
    RUN(heads2(two_tails ? s2 : s));
    RUN(agg_chain(s));
  }
  if (two_tails) VIPE_CHECK_ARG(join(3));
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_update_gate_state(const vipe_update_weights* wt, const vipe_update_buffers* b, const void* d_net,
                                       int parts, void* stream) {
  VIPE_CHECK_ARG(wt && b && b->E >= 0 && b->H > 0 && b->W > 0 && parts >= 1 && parts <= 3);
  if (b->E == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_net && (!(parts & 1) || (b->glo && b->extra)) && (!(parts & 2) || (b->pgate && b->pzr && wt->zr_n_w)));
  if (parts & 1) RUN(global_context(wt, b, d_net, as_stream(stream)));
  if (parts & 2) {
    // partial: pzr = pgate[..., 0:256] + the z|r convolution over the hidden state alone, raw fp32 sums
    ConvCall c = conv({b->E, b->H, b->W}, {d_net, 128, 0}, 128, wt->zr_n_w, wt->zr_b, 256, 3);
    c.epi = EPI_PARTIAL; c.accinit = {b->pgate, 384, 0};
    c.fout = b->pzr; c.y = {nullptr, 256, 0};  // PARTIAL: pitch and offset of fout
    RUN(vipe_conv_run(c, as_stream(stream)));
  }
  return vipe_launch_status();
}
#undef RUN

VIPE_EXPORT int vipe_update_gate_state_piece(void* user, int piece, int n_pieces, void* stream) {
  const vipe_gate_state_job* j = (const vipe_gate_state_job*)user;
  VIPE_CHECK_ARG(j && j->weights && j->buffers && j->net && n_pieces > 0 && piece >= 0 && piece < n_pieces);
  const vipe_update_buffers* b = j->buffers;
  VIPE_CHECK_ARG(b->E >= 0 && b->H > 0 && b->W > 0 && b->pgate && b->pzr);
  int64_t e0 = (int64_t)b->E * piece / n_pieces, e1 = (int64_t)b->E * (piece + 1) / n_pieces;
  if (j->bounds && j->n_bounds == n_pieces + 1) {
    e0 = j->bounds[piece];
    e1 = j->bounds[piece + 1];
    VIPE_CHECK_ARG(j->bounds[0] == 0 && j->bounds[n_pieces] == b->E && e0 >= 0 && e0 <= e1 && e1 <= b->E);
  }
  if (e1 <= e0) return VIPE_OK;
  const int64_t px = (int64_t)b->H * b->W;
  vipe_update_buffers sub = *b;
  sub.E = (int)(e1 - e0);
  sub.pgate = (const char*)b->pgate + e0 * px * 384 * 2;
  sub.pzr = b->pzr + e0 * px * 256;
  return vipe_update_gate_state(j->weights, &sub, (const char*)j->net + e0 * px * 128 * 2, 2, stream);
}

VIPE_EXPORT int vipe_glo_context(const float* d_glo_sum, const float* d_wT, const float* d_bias, float* d_extra, int E, int hw,
                                 void* stream) {
  VIPE_CHECK_ARG(E >= 0 && hw > 0);
  if (E == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_glo_sum && d_wT && d_bias && d_extra);
  glo_gemm_kernel<<<E, 384, 0, as_stream(stream)>>>(d_glo_sum, d_wT, d_bias, d_extra, 1.0f / (float)hw);
  return vipe_launch_status();
}

VIPE_EXPORT int vipe_update_finish(const float* d_coords1, const float* d_dw, const unsigned char* d_mask, float* d_target,
                                   float* d_weight, const float* d_eta, const int64_t* d_du, float* d_damping, int E,
                                   int n_src, int ht, int wd, void* stream) {
  VIPE_CHECK_ARG(E >= 0 && n_src >= 0 && ht > 0 && wd > 0);
  if (E == 0) return VIPE_OK;
  VIPE_CHECK_ARG(d_coords1 && d_dw && d_target && d_weight && (n_src == 0 || (d_eta && d_du && d_damping)));
  const int P = ht * wd;
  const int64_t n_px = (int64_t)E * P, n_eta = (int64_t)n_src * P;
  const int64_t n = n_px > n_eta ? n_px : n_eta;
  update_finish_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(d_coords1, d_dw, d_mask, d_target, d_weight,
                                                                                  d_eta, d_du, d_damping, n_px, n_eta, P);
  return vipe_launch_status();
}

}  // extern "C"
