// The launch sequence of the flow-update operator, printed on a machine without a GPU.
//
// csrc/update_op.hip and csrc/conv_mfma.hip are compiled host-only and linked with this file, which defines every HIP
// runtime function they call and records what it is asked to do.  Two programs are built from it:
//
//   launches (no TRACE_CALLS)  both objects linked: per configuration the return code and one line per event record /
//                              wait, memset and kernel (registered name, grid, block, dynamic LDS bytes, stream) - what
//                              the dispatcher makes of every call;
//   calls (TRACE_CALLS)        update_op.hip alone, vipe_conv_run defined here: every ConvCall descriptor in canonical
//                              form, one field per name - what the sequencer asks for.  TRACE_CALLS=2 intercepts the
//                              positional vipe_conv2d_fused of a tree from before the descriptor instead and maps its
//                              arguments onto the same form (tests/golden/make_golden_operator_trace_parent.py).
//
// tests/test_operator_trace.py builds and runs both and compares with tests/golden/operator_trace_parent.txt.
// The buffers are fake addresses, never dereferenced; they print as the name of the descriptor member they were given to.
#include <cxxabi.h>
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "../../vipe_amd/csrc/conv_call.cuh"

// ---- fake addresses ---------------------------------------------------------------------------------------------
namespace {
constexpr int SHIFT = 36;  // 64 GiB between two buffers
const char* g_names[128];
int g_n_names = 0;

template <typename T>
void fake(T*& field, const char* name) {
  g_names[g_n_names] = name;
  field = (T*)((uintptr_t)(++g_n_names) << SHIFT);
}

std::string sym(const void* p) {
  if (!p) return "-";
  const uintptr_t a = (uintptr_t)p, i = a >> SHIFT, off = a & (((uintptr_t)1 << SHIFT) - 1);
  char buf[96];
  if (i == 0 || i > (uintptr_t)g_n_names) snprintf(buf, sizeof buf, "?%llx", (unsigned long long)a);
  else if (off) snprintf(buf, sizeof buf, "%s+%llu", g_names[i - 1], (unsigned long long)off);
  else snprintf(buf, sizeof buf, "%s", g_names[i - 1]);
  return buf;
}

// ---- kernels by host function pointer (filled by the objects' static constructors, before main) ------------------
struct Kernel { const void* fn; char name[120]; int max_lds; };
Kernel g_kernels[128];
int g_n_kernels = 0;

Kernel* kernel_of(const void* fn) {
  for (int i = 0; i < g_n_kernels; ++i)
    if (g_kernels[i].fn == fn) return &g_kernels[i];
  return nullptr;
}

// "void (anonymous namespace)::k<1, 2>((anonymous namespace)::ConvArgs, int)" -> "k<1, 2>"
void short_name(const char* mangled, char* out, size_t n) {
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string s = status == 0 && d ? d : mangled;
  free(d);
  for (size_t p; (p = s.find("(anonymous namespace)::")) != std::string::npos;) s.erase(p, 23);
  if (s.compare(0, 5, "void ") == 0) s.erase(0, 5);
  int depth = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] == '<') ++depth;
    if (s[i] == '>') --depth;
    if (s[i] == '(' && depth == 0) { s.erase(i); break; }
  }
  snprintf(out, n, "%s", s.c_str());
}
}  // namespace

// ---- the HIP runtime, as far as the two objects use it -----------------------------------------------------------
extern "C" {
hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  static const char* names[] = {"ev0", "ev1", "ev2", "ev3", "ev4", "ev5", "ev6", "ev7"};
  static int n = 0;
  if (n >= 8) return hipErrorOutOfMemory;
  fake(*e, names[n++]);
  return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
  printf("  record %s on %s\n", sym(e).c_str(), sym(s).c_str());
  return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  printf("  %s waits for %s\n", sym(s).c_str(), sym(e).c_str());
  return hipSuccess;
}
hipError_t hipMemsetAsync(void* p, int v, size_t n, hipStream_t s) {
  printf("  memset %s = %d, %zu bytes on %s\n", sym(p).c_str(), v, n, sym(s).c_str());
  return hipSuccess;
}
hipError_t hipFuncSetAttribute(const void* fn, hipFuncAttribute attr, int value) {
  Kernel* k = kernel_of(fn);
  if (k && attr == hipFuncAttributeMaxDynamicSharedMemorySize && value > k->max_lds) k->max_lds = value;
  return k ? hipSuccess : hipErrorInvalidDeviceFunction;
}
hipError_t hipLaunchKernel(const void* fn, dim3 grid, dim3 block, void**, size_t lds, hipStream_t s) {
  const Kernel* k = kernel_of(fn);
  // a kernel asks for more than 64 KiB of dynamic LDS only after the limit has been raised for it
  const bool over = lds > 65536 && (!k || lds > (size_t)k->max_lds);
  printf("  kernel %s grid=(%u,%u,%u) block=(%u,%u,%u) lds=%zu on %s%s\n", k ? k->name : "?", grid.x, grid.y, grid.z, block.x,
         block.y, block.z, lds, sym(s).c_str(), over ? " LDS LIMIT NOT RAISED" : "");
  return hipSuccess;
}

static struct { dim3 grid, block; size_t lds; hipStream_t s; } g_config;
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t s) {
  g_config = {grid, block, lds, s};
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* s) {
  *grid = g_config.grid; *block = g_config.block; *lds = g_config.lds; *s = g_config.s;
  return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) {
  static void* handle;
  return &handle;
}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*, void*, int*) {
  if (g_n_kernels >= 128) abort();
  Kernel& k = g_kernels[g_n_kernels++];
  k.fn = host_fn;
  k.max_lds = 0;
  short_name(device_name, k.name, sizeof k.name);
}
void __hipUnregisterFatBinary(void**) {}

// ---- the library's other entry points the operator calls ---------------------------------------------------------
int vipe_corr_lookup_conv1x1_ex(const void* const* levels, const float* coords, const void* w, const float* bias, void* out,
                                int out_ctot, int out_coff, int B, int h1, int w1, int h2, int w2, int Cout, int act,
                                const int* slots, int layout, void* stream, int max_workgroups, int share_cu) {
  printf("  corr_lookup_conv1x1 levels=%s,%s,%s,%s coords=%s w=%s bias=%s out=%s/%d+%d %dx%dx%d targets=%dx%d Cout=%d act=%d "
         "slots=%s layout=%d max_wg=%d share_cu=%d on %s\n",
         sym(levels[0]).c_str(), sym(levels[1]).c_str(), sym(levels[2]).c_str(), sym(levels[3]).c_str(), sym(coords).c_str(),
         sym(w).c_str(), sym(bias).c_str(), sym(out).c_str(), out_ctot, out_coff, B, h1, w1, h2, w2, Cout, act,
         sym(slots).c_str(), layout, max_workgroups, share_cu, sym(stream).c_str());
  return VIPE_OK;
}
int vipe_segment_mean_nhwc_f16(const void* src, int src_ctot, int src_coff, const int* order, const int* rowptr, void* out,
                               int n_out, int64_t rows, int C, void* stream) {
  printf("  segment_mean src=%s/%d+%d order=%s rowptr=%s out=%s n=%d rows=%lld C=%d on %s\n", sym(src).c_str(), src_ctot, src_coff,
         sym(order).c_str(), sym(rowptr).c_str(), sym(out).c_str(), n_out, (long long)rows, C, sym(stream).c_str());
  return VIPE_OK;
}
}  // extern "C"

#ifdef TRACE_CALLS
// ---- section "calls": the descriptors, in canonical form ---------------------------------------------------------
namespace {
void view(const char* name, const ConvView& v) {
  if (v.p || v.ctot || v.coff) printf(" %s=%s/%d+%d", name, sym(v.p).c_str(), v.ctot, v.coff);
}
}  // namespace

int vipe_conv_run(const ConvCall& c, hipStream_t s) {
  printf("  conv %dx%dx%d %d->%d %dx%d act=%d epi=%d", c.B, c.H, c.W, c.Cin, c.Cout, c.KH, c.KW, c.act, c.epi);
  view("x0", c.x0);
  view("x1", c.x1.p ? c.x1 : c.x0);  // an absent x1 reads as x0 ...
  printf(" split=%d", c.x1.p && c.split < c.Cin ? c.split : c.Cin);  // ... with every channel before the split
  printf(" w=%s bias=%s", sym(c.w).c_str(), sym(c.bias).c_str());
  if (c.extra || c.extra_stride || c.extra_off) printf(" extra=%s/%d+%d", sym(c.extra).c_str(), c.extra_stride, c.extra_off);
  view("y", c.y);
  view("y2", c.y2);
  view("net", c.net);
  view("accinit", c.accinit);
  if (c.accinit_f32) printf(" accinit_f32");
  if (c.z) printf(" z=%s", sym(c.z).c_str());
  if (c.fout) printf(" fout=%s", sym(c.fout).c_str());
  if (c.heads2_frag) printf(" heads2_frag=%s", sym(c.heads2_frag).c_str());
  if (c.border) printf(" border=%s", sym(c.border).c_str());
  printf(" on %s\n", sym(s).c_str());
  return VIPE_OK;
}

extern "C" {
#if TRACE_CALLS == 2
// a tree from before the descriptor: the positional call, mapped onto it the way the entry point itself reads its slots
int vipe_conv2d_fused(const void* d_x0, int x0_ctot, int x0_coff, const void* d_x1, int x1_ctot, int x1_coff, int split,
                      const void* d_w_packed, const float* d_bias, const float* d_extra, int extra_stride, int extra_off,
                      void* d_y, int y_ctot, int y_coff, void* d_y2, int y2_ctot, int y2_coff, const void* d_net, int net_ctot,
                      int net_coff, const void* d_z, float* d_fout, const void* d_accinit, int ai_ctot, int ai_coff, int B,
                      int H, int W, int Cin, int Cout, int KH, int KW, int act, int mode, void* stream) {
  ConvCall c;
  c.x0 = {d_x0, x0_ctot, x0_coff};
  c.x1 = {d_x1, x1_ctot, x1_coff};
  c.split = split;
  c.w = d_w_packed; c.bias = d_bias; c.extra = d_extra; c.extra_stride = extra_stride; c.extra_off = extra_off;
  c.y = {d_y, y_ctot, y_coff};
  c.y2 = {d_y2, y2_ctot, y2_coff};
  c.net = {d_net, net_ctot, net_coff};
  c.z = d_z; c.fout = d_fout;
  c.accinit = {d_accinit, ai_ctot, ai_coff};
  c.accinit_f32 = (mode & VIPE_CONV_ACCINIT_F32) != 0;  // the mode bit becomes the flag
  c.B = B; c.H = H; c.W = W; c.Cin = Cin; c.Cout = Cout; c.KH = KH; c.KW = KW;
  c.act = act; c.epi = mode & ~VIPE_CONV_ACCINIT_F32;
  if (c.epi == VIPE_CONV_HEADS_FUSED) {  // mode 7 sends its fragments through d_net and its border sums through d_y2
    c.heads2_frag = d_net; c.border = (float*)d_y2;
    c.net.p = c.y2.p = nullptr;
  }
  return vipe_conv_run(c, (hipStream_t)stream);
}
#endif
// conv_mfma.hip is not linked in this section: its three other entry points the sequencer uses
int vipe_heads_fused_ok(int H, int W) {
  const char* v = getenv("VIPE_AMD_FUSED_HEADS");
  return !(v && v[0] == '0') && H > 0 && W > 0 && H % 4 == 0 && W % 64 == 0;
}
int vipe_heads_finish(float* dw, const float* border, const float* bias, int E, int H, int W, void* stream) {
  printf("  heads_finish dw=%s border=%s bias=%s %dx%dx%d on %s\n", sym(dw).c_str(), sym(border).c_str(), sym(bias).c_str(), E, H,
         W, sym(stream).c_str());
  return VIPE_OK;
}
}  // extern "C"
#endif

// ---- configurations ----------------------------------------------------------------------------------------------
namespace {
vipe_update_weights g_wt;
vipe_update_buffers g_bufs;  // everything set; a configuration takes away what it does not have
void* g_main_stream;
void* g_side_stream;

void fill() {
#define W_(f) fake(g_wt.f, #f);
  W_(corr0_w) W_(corr2_w) W_(flow0_w) W_(flow2_w) W_(gw_w) W_(zr_w) W_(q_w) W_(zr_s_w) W_(q_s_w) W_(heads0_w) W_(heads2_w)
  W_(agg2_w) W_(eta_w) W_(zr_n_w) W_(zr_x_w) W_(corr0_b) W_(corr2_b) W_(flow0_b) W_(flow2_b) W_(gw_b) W_(zr_b) W_(q_b)
  W_(heads0_b) W_(heads2_b) W_(agg2_b) W_(eta_b) W_(glo_wT) W_(glo_b) W_(agg1_w) W_(heads_dw_w) W_(agg1_b) W_(heads_dw_b)
  W_(heads2_frag)
#undef W_
#define B_(f) fake(g_bufs.f, #f);
  B_(levels[0]) B_(levels[1]) B_(levels[2]) B_(levels[3]) B_(coords) B_(slots) B_(corr) B_(motn) B_(net) B_(net_out) B_(xbuf)
  B_(pgate) B_(c1) B_(f1) B_(zb) B_(rnet) B_(hbuf) B_(dw) B_(glo) B_(extra) B_(order) B_(rowptr) B_(agg) B_(a2) B_(eta) B_(pzr)
  B_(hborder)
#undef B_
  fake(g_main_stream, "main");
  fake(g_side_stream, "side");
  g_bufs.h2 = 8;
  g_bufs.w2 = 64;
}

struct Config {
  const char* name;
  int H, W;
  int gate;       // 0: no pgate, 1: pgate, 2: staged (the first `staged` edges)
  int staged;
  bool two_streams;
  int n_src;
  bool lookup;    // correlation input: lookup levels (true) or a corr tensor
  bool by_consumer = true, frag = true, hborder = true;
  const char* fused_env = nullptr;
  int E = 5;
};

vipe_update_buffers buffers_of(const Config& c) {
  vipe_update_buffers b = g_bufs;
  b.E = c.E; b.H = c.H; b.W = c.W; b.n_src = c.n_src;
  if (c.lookup) b.corr = nullptr;
  else b.levels[0] = b.levels[1] = b.levels[2] = b.levels[3] = nullptr;
  if (c.gate == 0) b.pgate = nullptr;
  if (c.gate != 2) b.pzr = nullptr;
  b.gate_state = c.gate == 2 ? c.staged : 0;
  b.side_stream = c.two_streams ? g_side_stream : nullptr;
  if (!c.hborder) b.hborder = nullptr;
  return b;
}

void run_operator(const Config& c) {
  vipe_update_weights wt = g_wt;
  if (!c.by_consumer) wt.agg1_w = wt.heads_dw_w = nullptr, wt.agg1_b = wt.heads_dw_b = nullptr;
  if (!c.frag) wt.heads2_frag = nullptr;
  const vipe_update_buffers b = buffers_of(c);
  if (c.fused_env) setenv("VIPE_AMD_FUSED_HEADS", c.fused_env, 1);
  printf("== operator %s\n", c.name);
  const int rc = vipe_update_operator(&wt, &b, g_main_stream);
  printf("  rc=%d\n", rc);
  unsetenv("VIPE_AMD_FUSED_HEADS");
}

// every branch of the sequencer and every dispatch rule it reaches at least once; not the cross product
const Config CONFIGS[] = {
    // name                          H   W  gate staged two  n_src lookup
    {"8x64 fused heads",             8,  64, 1, 0, true,  3, true},
    {"8x64 no pgate, corr tensor",   8,  64, 0, 0, false, 0, false},
    {"8x64 staged 5/5, no fragments", 8, 64, 2, 5, true,  3, true, true, false},
    {"8x64 staged 3/5, one stream",  8,  64, 2, 3, false, 3, true},
    {"8x64 heads not by consumer",   8,  64, 1, 0, true,  3, true, false},
    {"8x64 no hborder",              8,  64, 1, 0, true,  3, false, true, true, false},
    {"8x64 VIPE_AMD_FUSED_HEADS=0",  8,  64, 1, 0, true,  3, true, true, true, true, "0"},
    {"8x64 two streams, no chain",   8,  64, 1, 0, true,  0, true},
    {"5x73 pgate, two streams",      5,  73, 1, 0, true,  3, true},
    {"5x73 no pgate, one stream",    5,  73, 0, 0, false, 3, false},
    {"5x73 staged 3/5, two streams", 5,  73, 2, 3, true,  3, true},
    {"5x73 staged 5/5, no chain",    5,  73, 2, 5, false, 0, false},
    {"8x130 no pgate, one stream",   8, 130, 0, 0, false, 3, false},
    {"8x130 no pgate, two streams",  8, 130, 0, 0, true,  3, true},
    {"8x130 pgate",                  8, 130, 1, 0, false, 3, true},
    {"8x130 staged 3/5",             8, 130, 2, 3, true,  3, true},
    {"E = 0",                        8,  64, 1, 0, true,  3, true, true, true, true, nullptr, 0},
    {"gate_state > E",               8,  64, 2, 6, true,  3, true},
};

void run_gate_state(int H, int W, int parts) {
  Config c = {"", H, W, 2, 5, false, 0, true};
  const vipe_update_buffers b = buffers_of(c);
  const void* net;
  fake(net, "new_net");
  printf("== gate_state %dx%d parts=%d\n", H, W, parts);
  printf("  rc=%d\n", vipe_update_gate_state(&g_wt, &b, net, parts, g_side_stream));
  --g_n_names;
}

void run_pieces(int H, int W, const int* bounds, int n_pieces) {
  Config c = {"", H, W, 2, 5, false, 0, true};
  const vipe_update_buffers b = buffers_of(c);
  vipe_gate_state_job job = {&g_wt, &b, nullptr, bounds, bounds ? n_pieces + 1 : 0};
  fake(job.net, "new_net");
  for (int k = 0; k < n_pieces; ++k) {
    printf("== gate_state_piece %dx%d %s piece %d of %d\n", H, W, bounds ? "bounds 0,2,2,5" : "even split", k, n_pieces);
    printf("  rc=%d\n", vipe_update_gate_state_piece(&job, k, n_pieces, g_side_stream));
  }
  --g_n_names;
}

#ifndef TRACE_CALLS
// ---- direct calls of the positional ABI --------------------------------------------------------------------------
struct Src { const char* buf; int ctot, coff, n; };  // n channels of buffer `buf` from channel coff
struct Launch {
  const char* name;
  int mode, cout, k;
  Src x0, x1;
  int act, extra_off;  // extra_off < 0: no extra
  Src init;            // initial accumulators (pzr: fp32)
  bool net, z;
  int y_ctot, y_coff;  // y_ctot < 0: no y
  bool y2;
};
const Src NONE = {nullptr, 0, 0, 0};
// oracle/conv_epilogue_cases.py::LAUNCHES, entry by entry
const Launch LAUNCHES[] = {
    {"glo_net", 1, 128, 1, {"net", 128, 0, 128}, NONE, 0, -1, NONE, true, false, -1, 0, false},
    {"glo_x", 1, 128, 1, {"x", 128, 0, 128}, NONE, 0, -1, NONE, true, false, -1, 0, false},
    {"zr", 2, 256, 3, {"net", 128, 0, 128}, {"xbuf", 320, 0, 320}, 0, 0, NONE, true, false, 128, 0, true},
    {"zr_ctx", 2, 256, 3, {"net", 128, 0, 128}, {"xbuf", 320, 128, 192}, 0, 0, {"pgate", 384, 0, 0}, true, false, 128, 0, true},
    {"zr_staged", 2, 256, 3, {"xbuf", 320, 128, 192}, NONE, 0, 0, {"pzr", 256, 0, 0}, true, false, 128, 0, true},
    {"partial", 6, 256, 3, {"net", 128, 0, 128}, NONE, 0, -1, {"pgate", 384, 0, 0}, false, false, 256, 0, false},
    {"q", 3, 128, 3, {"rnet", 128, 0, 128}, {"xbuf", 320, 0, 320}, 0, 256, NONE, true, true, 128, 0, false},
    {"q_ctx", 3, 128, 3, {"rnet", 128, 0, 128}, {"xbuf", 320, 128, 192}, 0, 256, {"pgate", 384, 256, 0}, true, true, 128, 0, false},
    {"heads", 4, 4, 3, {"hbuf", 384, 0, 256}, NONE, 0, -1, NONE, false, false, -1, 0, false},
    {"eta", 5, 1, 3, {"a2", 128, 0, 128}, NONE, 0, -1, NONE, false, false, -1, 0, false},
    {"plain_corr2", 0, 128, 3, {"c1", 128, 0, 128}, NONE, 1, -1, NONE, false, false, 320, 128, false},
    {"plain_flow2", 0, 64, 3, {"f1", 128, 0, 128}, NONE, 1, -1, NONE, false, false, 320, 256, false},
    {"plain_heads0", 0, 384, 3, {"net", 128, 0, 128}, NONE, 1, -1, NONE, false, false, 384, 0, false},
    {"plain_upmask", 0, 576, 1, {"a2", 128, 0, 128}, NONE, 0, -1, NONE, false, false, 576, 0, false},
};

const void* named(const char* name) {  // one address per name
  if (!name) return nullptr;
  for (int i = 0; i < g_n_names; ++i)
    if (!strcmp(g_names[i], name)) return (const void*)((uintptr_t)(i + 1) << SHIFT);
  const void* p;
  fake(p, name);
  return p;
}

void run_launch(const Launch& L, int B, int H, int W) {
  const bool partial = L.mode == VIPE_CONV_PARTIAL, fout = L.mode == 1 || L.mode >= 4;
  const int mode = L.mode | (L.init.buf && !strcmp(L.init.buf, "pzr") ? VIPE_CONV_ACCINIT_F32 : 0);
  printf("== conv2d_fused %s %dx%dx%d\n", L.name, B, H, W);
  const int rc = vipe_conv2d_fused(
      named(L.x0.buf), L.x0.ctot, L.x0.coff, named(L.x1.buf), L.x1.ctot, L.x1.coff, L.x0.n, named("w"), (const float*)named("bias"),
      (const float*)(L.extra_off >= 0 ? named("extra") : nullptr), L.extra_off >= 0 ? 384 : 0, L.extra_off >= 0 ? L.extra_off : 0,
      (void*)(L.y_ctot >= 0 && !partial ? named("y") : nullptr), L.y_ctot >= 0 ? L.y_ctot : 0, L.y_coff,
      (void*)(L.y2 ? named("y2") : nullptr), L.y2 ? 128 : 0, 0, L.net ? named("net") : nullptr, L.net ? 128 : 0, 0,
      L.z ? named("z") : nullptr, (float*)(fout ? named("fout") : nullptr), named(L.init.buf), L.init.ctot, L.init.coff, B, H, W,
      L.x0.n + L.x1.n, L.cout, L.k, L.k, L.act, mode, g_main_stream);
  printf("  rc=%d\n", rc);
}

void run_direct() {
  for (const Launch& L : LAUNCHES) {
    run_launch(L, 2, 8, 64);  // conv_epilogue_cases.GRIDS: aligned ...
    run_launch(L, 2, 9, 86);  // ... and flat
  }
  auto plain = [](const char* what, int B, int H, int W, int Cin, int Cout, int k, int cin_off = 0) {
    printf("== conv2d_nhwc_f16 %s %dx%dx%d %d->%d %dx%d\n", what, B, H, W, Cin, Cout, k, k);
    printf("  rc=%d\n", vipe_conv2d_nhwc_f16(named("x"), named("w"), (const float*)named("bias"), nullptr, (void*)named("y"), B, H, W, Cin,
                                             Cin == 4 ? 4 : 128, cin_off, Cout, Cout, 0, k, k, VIPE_ACT_RELU, g_main_stream));
  };
  plain("7x7 aligned", 2, 8, 64, 4, 128, 7);
  plain("7x7 flat", 2, 9, 86, 4, 128, 7);
  plain("7x7 wide", 2, 8, 130, 4, 128, 7);
  plain("upmask", 3, 8, 64, 128, 576, 1);
  plain("mis-aligned channel offset", 2, 8, 64, 64, 128, 3, 4);
  // mode 7 on 8 x 64, and the refusals
  auto fused = [](const char* what, int H, int W) {
    printf("== conv2d_fused heads_fused %s 2x%dx%d\n", what, H, W);
    printf("  rc=%d\n", vipe_conv2d_fused(named("net"), 128, 0, nullptr, 0, 0, 128, named("w"), (const float*)named("bias"), nullptr, 0, 0,
                                          nullptr, 0, 0, (void*)named("border"), 0, 0, named("frag"), 0, 0, nullptr,
                                          (float*)named("fout"), nullptr, 0, 0, 2, H, W, 128, 256, 3, 3, VIPE_ACT_RELU,
                                          VIPE_CONV_HEADS_FUSED, g_main_stream));
  };
  fused("aligned", 8, 64);
  fused("rows not a multiple of 4", 6, 64);
  Launch bad = LAUNCHES[5];  // partial
  bad.name = "partial, Cout % 4 != 0";
  bad.cout = 254;
  run_launch(bad, 2, 8, 64);
  run_launch(LAUNCHES[3], 2, 8, 130);  // initial accumulators, fp16 ...
  run_launch(LAUNCHES[4], 2, 8, 130);  // ... and fp32, on a grid no tile kernel takes
}
#endif
}  // namespace

int main() {
  fill();
  for (const Config& c : CONFIGS) run_operator(c);
  const int grids[3][2] = {{8, 64}, {5, 73}, {8, 130}};
  for (const auto& g : grids)
    for (int parts = 1; parts <= 3; ++parts) run_gate_state(g[0], g[1], parts);
  const int bounds[] = {0, 2, 2, 5};  // the second piece is empty
  for (int i = 0; i < 2; ++i) {
    run_pieces(grids[i][0], grids[i][1], bounds, 3);
    run_pieces(grids[i][0], grids[i][1], nullptr, 2);
  }
#ifndef TRACE_CALLS
  run_direct();
#endif
  return 0;
}
