// One launch of the fused convolutions (conv_mfma.hip), described by name.  Internal: not part of include/vipe_amd.h.
//
// The sequencer (update_op.hip) fills a ConvCall with the operands a launch has and leaves the rest at their defaults;
// vipe_conv_run is the one route to the kernels: it validates every call, fills the kernels' argument block and dispatches.
// The positional C entry points (vipe_conv2d_fused, vipe_conv2d_nhwc_f16) are translations into this struct.
#pragma once
#include <hip/hip_runtime_api.h>
#include <limits.h>

#include "../../include/vipe_amd.h"

// the `mode` of vipe_conv2d_fused
enum Epi { EPI_PLAIN = 0, EPI_GLO = 1, EPI_ZR = 2, EPI_Q = 3, EPI_HEADS = 4, EPI_ETA = 5, EPI_PARTIAL = 6, EPI_HEADS_FUSED = 7 };

// channels [coff, ...) of a channels-last tensor with `ctot` channels per pixel
struct ConvView {
  const void* p = nullptr;
  int ctot = 0, coff = 0;
};

struct ConvCall {
  ConvView x0, x1;      // fp16 input: channels [0, split) from x0, [split, Cin) from x1
  int split = INT_MAX;  // default: every channel from x0
  const void* w = nullptr;      // vipe_conv_pack_weights
  const float* bias = nullptr;  // readable up to the padded output-channel count
  const float* extra = nullptr;  // [B][extra_stride] f32 per-image additive term, from column extra_off
  int extra_stride = 0, extra_off = 0;
  ConvView y;        // fp16 output (PLAIN, ZR: z, Q).  PARTIAL: p stays null, ctot / coff are the pitch and offset of fout
  ConvView y2;       // ZR: r * net
  ConvView net;      // hidden state (GLO, ZR, Q)
  ConvView accinit;  // optional initial accumulators: fp16, or ...
  bool accinit_f32 = false;  // ... fp32, the output of a PARTIAL launch
  const void* z = nullptr;   // Q: [M,128] fp16
  float* fout = nullptr;     // GLO [B,Cout], HEADS / HEADS_FUSED [M,4], ETA [M], PARTIAL [M, y.ctot]
  const void* heads2_frag = nullptr;  // HEADS_FUSED: the heads2 weights as matrix fragments (include/vipe_amd.h, mode 7)
  float* border = nullptr;            // HEADS_FUSED: [vipe_heads_border_floats] per-tile border sums
  int B = 0, H = 0, W = 0, Cin = 0, Cout = 0, KH = 1, KW = 1;
  int act = VIPE_ACT_NONE, epi = EPI_PLAIN;
};

// VIPE_OK, VIPE_EINVAL (an operand the epilogue needs is missing or mis-aligned) or VIPE_EUNSUPPORTED (no kernel takes
// this call on this grid).  No allocation, no host synchronisation.
int vipe_conv_run(const ConvCall& c, hipStream_t stream);
