// api_replay.cpp - the replay entries: one launch of a kernel family, described by an int64 descriptor, run on caller operands in
// their device layout so that tests can hold it to an fp64 reference element-wise (tsd_debug_gemm_run / _norm_run / _attn_run / _chain_run /
// _elem_run, and the recording of the GEMM descriptors the product's graphs launch).  Test infrastructure, not the measured path.  What the five
// entries share - the guarded device operands, the scan for writes outside an output's logical elements (replay_scan.h), the slot
// checks and the scoped option overrides - is written once here; sizing, marshalling and the reported plan stay with each family.
#include <string.h>

#include <algorithm>
#include <vector>

#include "gemm_tiles.h"
#include "graph.h"
#include "replay_scan.h"

namespace {
constexpr size_t GUARD = 4096;  // bytes of NaN pattern before and after every operand

// The device operands of one replayed launch.  Every slot is its extent between two guard bands, the whole of it filled with the NaN
// pattern of its element size, then started from a payload where it has one: the inputs, and an output the launch updates in place.
class GuardedOperands {
 public:
  GuardedOperands(tsd_ctx* ctx, int slots) : st_(ctx->stream), s_((size_t)slots) {}
  ~GuardedOperands() { for (Slot& s : s_) if (s.p) (void)dev_free(s.p); }
  GuardedOperands(const GuardedOperands&) = delete;
  // ext elements of es (2 or 4) bytes; payload: ext host elements to upload, or NULL; out: where read_back copies the extent - what
  // makes the slot an output - whose logical elements are `box`
  int add(int slot, int64_t ext, int es, const void* payload, void* out = nullptr, const replay::Box& box = replay::Box()) {
    Slot& s = s_[(size_t)slot];
    s.ext = ext; s.es = es; s.payload = payload; s.out = out; s.box = box;
    const size_t bytes = 2 * GUARD + (size_t)ext * es;
    HIP_TRY(dev_malloc((void**)&s.p, bytes));
    if (es == 2) HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)s.p, replay::NAN16, bytes / 2, st_));
    else HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)s.p, (int)replay::NAN32, bytes / 4, st_));
    if (payload) HIP_TRY(hipMemcpyAsync(s.p + GUARD, payload, (size_t)ext * es, hipMemcpyHostToDevice, st_));
    return TSD_OK;
  }
  void* at(int slot) const { return s_[(size_t)slot].p ? (void*)(s_[(size_t)slot].p + GUARD) : nullptr; }
  // After the launch: every output's extent to the caller, and the count of elements outside the outputs' logical elements that no
  // longer hold what they held before it (replay_scan.h).  Of an input only the two bands are read: no launch is given its payload to write.
  int read_back(int64_t* changed) {
    *changed = 0;
    std::vector<char> got;
    for (const Slot& s : s_) {
      if (!s.p) continue;
      const size_t body = (size_t)s.ext * s.es;
      got.resize(2 * GUARD + (s.out ? body : 0));
      if (s.out) {
        HIP_TRY(hipMemcpy(got.data(), s.p, got.size(), hipMemcpyDeviceToHost));
        memcpy(s.out, &got[GUARD], body);
      } else {
        HIP_TRY(hipMemcpy(got.data(), s.p, GUARD, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(&got[GUARD], s.p + GUARD + body, GUARD, hipMemcpyDeviceToHost));
      }
      *changed += replay::scan_changed(got.data(), (int64_t)(GUARD / s.es), s.out ? s.ext : 0, s.es, s.box, s.out ? s.payload : nullptr);
    }
    return TSD_OK;
  }

 private:
  struct Slot {
    char* p = nullptr;
    int64_t ext = 0;
    int es = 2;
    const void* payload = nullptr;
    void* out = nullptr;
    replay::Box box;
  };
  hipStream_t st_;
  std::vector<Slot> s_;
};

int check_fields(const char* who, int n, int need) {
  if (n < need) TSD_FAIL(TSD_E_ARG, "%s: %d descriptor fields", who, n);
  return TSD_OK;
}
// every sized slot has its host pointer: inputs [0, first_out) in host_in, the outputs from first_out on in host_out
int check_slots(const char* who, const int64_t* ext, int count, int first_out, const void* const* host_in, void* const* host_out) {
  for (int s = 0; s < count; s++)
    if (ext[s] && (s < first_out ? !host_in[s] : !host_out[s - first_out])) TSD_FAIL(TSD_E_ARG, "%s: operand slot %d is NULL", who, s);
  return TSD_OK;
}
float f32_of(int64_t bits) {
  const uint32_t b = (uint32_t)bits;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
}  // namespace

// ---- GEMM launch descriptors: record and replay (tests/gemm_ref.py holds each launch to an fp64 reference) -------------------
void gemm_describe(const tsd_ctx* ctx, const GemmArgs& a, int64_t* d) {
  for (int i = 0; i < TSD_GD_COUNT; i++) d[i] = 0;
  d[TSD_GD_VERSION] = TSD_GD_VERSION_1;
  d[TSD_GD_CONV] = a.conv; d[TSD_GD_M] = a.M; d[TSD_GD_N] = a.N; d[TSD_GD_K] = a.K;
  d[TSD_GD_K0] = (!a.conv && a.A1) ? a.K0 : a.K;  // what launch_gemm hands the kernel
  d[TSD_GD_LDA0] = a.lda0; d[TSD_GD_LDA1] = a.lda1; d[TSD_GD_LDA2] = a.lda2; d[TSD_GD_LDW] = a.ldw; d[TSD_GD_LDW1] = a.ldw1;
  d[TSD_GD_LDR] = a.ldr; d[TSD_GD_LDC] = a.ldc;
  d[TSD_GD_BATCH] = a.batch; d[TSD_GD_SA] = a.sA; d[TSD_GD_SW] = a.sW; d[TSD_GD_SC] = a.sC; d[TSD_GD_SR] = a.sR;
  if (a.conv) {
    d[TSD_GD_HS] = a.Hs; d[TSD_GD_WS] = a.Ws; d[TSD_GD_HO] = a.Ho; d[TSD_GD_WO] = a.Wo; d[TSD_GD_CIN] = a.Cin;
    d[TSD_GD_STRIDE] = a.stride; d[TSD_GD_PAD] = a.pad; d[TSD_GD_UPS] = a.ups; d[TSD_GD_CIN1] = a.Cin1; d[TSD_GD_CIN2] = a.Cin2;
  }
  d[TSD_GD_W_KTS] = a.w_kts ? 1 : 0;
  d[TSD_GD_EPI] = a.epi;
  uint32_t bits;
  memcpy(&bits, &a.out_scale, 4);
  d[TSD_GD_OUT_SCALE] = bits;
  d[TSD_GD_ROWVEC_LD] = a.rowvec_ld; d[TSD_GD_ROWS_PER_BATCH] = a.rows_per_batch;
  if (a.Vt) { d[TSD_GD_VT] = 1; d[TSD_GD_VT_N0] = a.vt_n0; d[TSD_GD_VT_LD] = a.vt_ld; d[TSD_GD_VT_S] = a.vt_S; d[TSD_GD_VT_SB] = a.vt_sB; }
  d[TSD_GD_GN_GROUPS] = a.gn_groups; d[TSD_GD_GN_RPS] = a.gn_rows_per_sample; d[TSD_GD_GN_NSLAB] = a.gn_nslab;
  d[TSD_GD_RPS_HINT] = a.rows_per_sample_hint; d[TSD_GD_SK_BIG] = ctx->opt.sk_big_graph;
  d[TSD_GD_ALIAS] = (a.R && (const void*)a.R == a.C ? 1 : 0) | (a.A1 && a.A1 == a.A0 ? 2 : 0) | (a.A2 && a.A2 == a.A1 ? 4 : 0);
  d[TSD_GD_CFG] = -1; d[TSD_GD_WAYS] = 0;
}

extern "C" int tsd_debug_gemm_record(tsd_ctx* ctx, int on) {
  NOTNULL(ctx);
  if (on) ctx->gemm_rec.clear();
  ctx->gemm_rec_on = on != 0;
  return (int)(ctx->gemm_rec.size() / TSD_GD_COUNT);
}

extern "C" int tsd_debug_gemm_recorded(tsd_ctx* ctx, int i, int64_t* desc, int n) {
  NOTNULL(ctx); NOTNULL(desc);
  if (n < TSD_GD_COUNT || i < 0 || (size_t)(i + 1) * TSD_GD_COUNT > ctx->gemm_rec.size())
    TSD_FAIL(TSD_E_ARG, "gemm_recorded: no descriptor %d (capacity %d)", i, n);
  memcpy(desc, &ctx->gemm_rec[(size_t)i * TSD_GD_COUNT], TSD_GD_COUNT * sizeof(int64_t));
  return TSD_GD_COUNT;
}

namespace {
int gd_elem_bytes(int slot, const int64_t* d) {
  if (slot == TSD_GO_BIAS || slot == TSD_GO_ROWVEC || slot == TSD_GO_GN) return 4;
  if (slot == TSD_GO_C && (d[TSD_GD_EPI] & EPI_OUT_F32)) return 4;
  return 2;
}
// Columns of C the launch stores (the Vt tail's columns go to Vt instead, GEGLU halves the width)
int64_t gd_c_cols(const int64_t* d) {
  if (d[TSD_GD_VT]) return d[TSD_GD_VT_N0];
  return (d[TSD_GD_EPI] & EPI_GEGLU) ? d[TSD_GD_N] / 2 : d[TSD_GD_N];
}
// Element extent of every operand the descriptor reads or writes, including the kernel's clamped loads (bias / row vector at
// N - 4, residual at N - 8: all inside [0, N)).  Refuses what it cannot size; the combinations launch_gemm itself refuses are left to it.
// allocatable = false (planning only): the extents may exceed what one replay operand may hold.
int gd_extents(const int64_t* d, int64_t* e, bool allocatable = true) {
  for (int i = 0; i < TSD_GO_COUNT; i++) e[i] = 0;
#define GD_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "gemm_run: descriptor cannot be sized (%s)", #cond)
  GD_REQ(d[TSD_GD_VERSION] == TSD_GD_VERSION_1);
  const int64_t M = d[TSD_GD_M], N = d[TSD_GD_N], K = d[TSD_GD_K], K0 = d[TSD_GD_K0], batch = d[TSD_GD_BATCH], epi = d[TSD_GD_EPI];
  const int64_t lim = 1LL << 30;
  GD_REQ(M > 0 && N > 0 && K > 0 && M < (1 << 26) && N <= 65536 && K <= 65536 && N % 4 == 0);
  GD_REQ(batch >= 1 && batch <= 4096 && epi >= 0 && epi < 256);
  for (int f : {TSD_GD_LDA0, TSD_GD_LDA1, TSD_GD_LDA2, TSD_GD_LDW, TSD_GD_LDW1, TSD_GD_LDR, TSD_GD_LDC, TSD_GD_ROWVEC_LD, TSD_GD_VT_LD})
    GD_REQ(d[f] >= 0 && d[f] <= 65536);
  for (int f : {TSD_GD_SA, TSD_GD_SW, TSD_GD_SC, TSD_GD_SR, TSD_GD_VT_SB}) GD_REQ(d[f] >= 0 && d[f] <= lim);
  const int64_t sA = d[TSD_GD_SA], sW = d[TSD_GD_SW], sC = d[TSD_GD_SC], sR = d[TSD_GD_SR];
  int64_t KW = K, B = 1;
  if (d[TSD_GD_CONV]) {
    const int64_t Hs = d[TSD_GD_HS], Ws = d[TSD_GD_WS], Ho = d[TSD_GD_HO], Wo = d[TSD_GD_WO], Cin = d[TSD_GD_CIN];
    const int64_t Cin1 = d[TSD_GD_CIN1], Cin2 = d[TSD_GD_CIN2];
    GD_REQ(Hs > 0 && Ws > 0 && Ho > 0 && Wo > 0 && Hs < 2048 && Ws < 2048 && Ho < 2048 && Wo < 2048 && Cin > 0 && Cin <= 8192);
    GD_REQ(batch == 1 && M % (Ho * Wo) == 0 && d[TSD_GD_LDA0] >= Cin);
    GD_REQ((d[TSD_GD_STRIDE] == 1 || d[TSD_GD_STRIDE] == 2) && (d[TSD_GD_UPS] >= 0 && d[TSD_GD_UPS] <= 2) && d[TSD_GD_PAD] >= 0 && d[TSD_GD_PAD] <= 1);
    {  // Ho / Wo must follow from the source, stride, pad and a bottom / right pad of 0 or 1: the kernel packs each output pixel's
       // first tap (o * stride - pad + 1) into an 11-bit field with the sample index above it, so a larger one would read another image
      const int64_t st = d[TSD_GD_STRIDE], pad = d[TSD_GD_PAD], up = d[TSD_GD_UPS] ? 2 : 1;
      bool geo = false;
      for (int64_t br = 0; br <= 1; br++)
        geo = geo || ((up * Hs + pad + br - 3) / st + 1 == Ho && (up * Ws + pad + br - 3) / st + 1 == Wo && up * Hs + pad + br >= 3 && up * Ws + pad + br >= 3);
      GD_REQ(geo && (Ho - 1) * st - pad + 2 < 2048 && (Wo - 1) * st - pad + 2 < 2048);
    }
    B = M / (Ho * Wo);
    const int64_t px = B * Hs * Ws;
    e[TSD_GO_A0] = (px - 1) * d[TSD_GD_LDA0] + Cin;
    KW = 9 * Cin;
    GD_REQ(Cin1 >= 0 && Cin2 >= 0 && (Cin1 > 0 || Cin2 == 0));
    if (Cin1 > 0) {  // the skip sources are read at the output pixel: same resolution
      GD_REQ(Ho == Hs && Wo == Ws && d[TSD_GD_LDA1] >= Cin1 && d[TSD_GD_LDW1] >= Cin1 + Cin2);
      e[TSD_GO_A1] = (px - 1) * d[TSD_GD_LDA1] + Cin1;
      if (Cin2 > 0) {
        GD_REQ(d[TSD_GD_LDA2] >= Cin2);
        e[TSD_GO_A2] = (px - 1) * d[TSD_GD_LDA2] + Cin2;
      }
      e[TSD_GO_WT1] = (N - 1) * d[TSD_GD_LDW1] + Cin1 + Cin2;
    }
  } else {
    GD_REQ(K0 > 0 && K0 <= K && d[TSD_GD_LDA0] >= K0);
    e[TSD_GO_A0] = (batch - 1) * sA + (M - 1) * d[TSD_GD_LDA0] + K0;
    if (K0 < K) {
      GD_REQ(d[TSD_GD_LDA1] >= K - K0);
      e[TSD_GO_A1] = (batch - 1) * sA + (M - 1) * d[TSD_GD_LDA1] + (K - K0);
    }
  }
  if (d[TSD_GD_W_KTS]) {
    GD_REQ(batch == 1 && KW % 64 == 0);
    e[TSD_GO_W] = N * KW;  // passed row-major [N][KW]
  } else {
    GD_REQ(d[TSD_GD_LDW] >= KW);
    e[TSD_GO_W] = (batch - 1) * sW + (N - 1) * d[TSD_GD_LDW] + KW;
  }
  const int64_t ccols = gd_c_cols(d);
  GD_REQ(ccols > 0 && ccols <= N && d[TSD_GD_LDC] >= ccols);
  e[TSD_GO_C] = (batch - 1) * sC + (M - 1) * d[TSD_GD_LDC] + ccols;
  if (epi & (EPI_BIAS_N | EPI_BIAS_M)) e[TSD_GO_BIAS] = std::max((epi & EPI_BIAS_N) ? N : 0, (epi & EPI_BIAS_M) ? M : 0);
  if (epi & EPI_ROWVEC) {
    GD_REQ(d[TSD_GD_ROWS_PER_BATCH] >= 1 && (d[TSD_GD_ROWVEC_LD] == 0 || d[TSD_GD_ROWVEC_LD] >= N));
    e[TSD_GO_ROWVEC] = ((M - 1) / d[TSD_GD_ROWS_PER_BATCH]) * d[TSD_GD_ROWVEC_LD] + N;
  }
  if (epi & EPI_RESIDUAL) {
    if (d[TSD_GD_ALIAS] & 1) {  // in place: R is C's initial content
      GD_REQ(!(epi & (EPI_RES_UPS | EPI_GEGLU | EPI_OUT_F32)) && !d[TSD_GD_VT] && d[TSD_GD_LDR] == d[TSD_GD_LDC] && sR == sC);
      e[TSD_GO_R] = e[TSD_GO_C];
    } else {
      int64_t rows = M;
      if (d[TSD_GD_CONV] && (epi & EPI_RES_UPS)) {
        GD_REQ(d[TSD_GD_HO] % 2 == 0 && d[TSD_GD_WO] % 2 == 0);
        rows = B * (d[TSD_GD_HO] / 2) * (d[TSD_GD_WO] / 2);
      }
      GD_REQ(d[TSD_GD_LDR] >= N);
      e[TSD_GO_R] = (batch - 1) * sR + (rows - 1) * d[TSD_GD_LDR] + N;
    }
  }
  if (d[TSD_GD_VT]) {
    const int64_t n0 = d[TSD_GD_VT_N0], S = d[TSD_GD_VT_S];
    GD_REQ(n0 > 0 && n0 < N && S > 0 && M % S == 0 && d[TSD_GD_VT_LD] >= S && d[TSD_GD_VT_SB] >= (N - n0 - 1) * d[TSD_GD_VT_LD] + S);
    e[TSD_GO_VT] = (M / S - 1) * d[TSD_GD_VT_SB] + (N - n0 - 1) * d[TSD_GD_VT_LD] + S;
  }
  if (epi & EPI_GNSTATS) {
    const int64_t G = d[TSD_GD_GN_GROUPS], rps = d[TSD_GD_GN_RPS], ns = d[TSD_GD_GN_NSLAB];
    GD_REQ(G > 0 && G <= N && rps > 0 && M % rps == 0 && ns > 0 && ns * 32 <= rps);
    e[TSD_GO_GN] = (M / rps) * ns * G * 2;
  }
  for (int s = 0; s < TSD_GO_COUNT; s++) GD_REQ(e[s] >= 0 && (e[s] <= lim || !allocatable));
#undef GD_REQ
  return TSD_OK;
}
// The launch a descriptor describes, without its operands: every GemmArgs field that is no pointer (what gemm_plan reads)
GemmArgs gd_args(const int64_t* d) {
  GemmArgs g;
  g.conv = (int)d[TSD_GD_CONV]; g.M = (int)d[TSD_GD_M]; g.N = (int)d[TSD_GD_N]; g.K = (int)d[TSD_GD_K];
  g.lda0 = (int)d[TSD_GD_LDA0]; g.lda1 = (int)d[TSD_GD_LDA1]; g.K0 = (int)d[TSD_GD_K0]; g.lda2 = (int)d[TSD_GD_LDA2];
  g.ldw = (int)d[TSD_GD_LDW]; g.ldw1 = (int)d[TSD_GD_LDW1];
  if (d[TSD_GD_W_KTS]) { g.ldw = 64; g.w_kts = g.N * 128; }  // the K-tile-major copy the model path builds for weight-heavy layers
  g.batch = (int)d[TSD_GD_BATCH]; g.sA = d[TSD_GD_SA]; g.sW = d[TSD_GD_SW]; g.sC = d[TSD_GD_SC]; g.sR = d[TSD_GD_SR];
  if (g.conv) {
    g.Hs = (int)d[TSD_GD_HS]; g.Ws = (int)d[TSD_GD_WS]; g.Ho = (int)d[TSD_GD_HO]; g.Wo = (int)d[TSD_GD_WO]; g.Cin = (int)d[TSD_GD_CIN];
    g.stride = (int)d[TSD_GD_STRIDE]; g.pad = (int)d[TSD_GD_PAD]; g.ups = (int)d[TSD_GD_UPS];
    g.Cin1 = (int)d[TSD_GD_CIN1]; g.Cin2 = (int)d[TSD_GD_CIN2];
  }
  g.epi = (int)d[TSD_GD_EPI];
  g.out_scale = f32_of(d[TSD_GD_OUT_SCALE]);
  g.rowvec_ld = (int)d[TSD_GD_ROWVEC_LD]; g.rows_per_batch = (int)d[TSD_GD_ROWS_PER_BATCH];
  g.ldr = (int)d[TSD_GD_LDR]; g.ldc = (int)d[TSD_GD_LDC];
  if (d[TSD_GD_VT]) { g.vt_n0 = (int)d[TSD_GD_VT_N0]; g.vt_ld = (int)d[TSD_GD_VT_LD]; g.vt_S = (int)d[TSD_GD_VT_S]; g.vt_sB = d[TSD_GD_VT_SB]; }
  g.gn_groups = (int)d[TSD_GD_GN_GROUPS]; g.gn_rows_per_sample = (int)d[TSD_GD_GN_RPS]; g.gn_nslab = (int)d[TSD_GD_GN_NSLAB];
  g.rows_per_sample_hint = (int)d[TSD_GD_RPS_HINT];
  return g;
}
}  // namespace

// The plan of the launch desc describes, without a device: ctx == NULL plans under the options of the environment
extern "C" int tsd_debug_gemm_plan(tsd_ctx* ctx, const int64_t* desc, int n, int cfg, int64_t* plan) {
  NOTNULL(desc); NOTNULL(plan);
  TSD_TRY(check_fields("gemm_plan", n, TSD_GD_COUNT));
  int64_t ext[TSD_GO_COUNT];
  TSD_TRY(gd_extents(desc, ext, false));  // a well-formed launch, of any size
  TsdOptions opt;
  if (ctx) opt = ctx->opt; else options_from_env(opt);
  opt.force_cfg = cfg >= 0 ? cfg : -1;
  if (cfg < 0) opt.sk_big_graph = (int)desc[TSD_GD_SK_BIG];
  const GemmPlan p = gemm_plan(opt, gd_args(desc));
  if (p.refused) TSD_FAIL(TSD_E_ARG, "gemm_plan: %s (tile configuration %d)", p.refused, p.cfg);
  plan[TSD_GP_CFG] = p.cfg; plan[TSD_GP_WAYS] = p.ways; plan[TSD_GP_VARIANT] = p.variant;
  plan[TSD_GP_BM] = p.BM; plan[TSD_GP_BN] = p.BN; plan[TSD_GP_BMW] = p.BMw; plan[TSD_GP_BNW] = p.BNw;
  plan[TSD_GP_K] = p.K; plan[TSD_GP_WS_FLOATS] = p.ws_floats; plan[TSD_GP_LDS_BYTES] = p.lds_bytes;
  plan[TSD_GP_GN_NSLAB] = p.gn_slabs((int)desc[TSD_GD_GN_RPS], (int)desc[TSD_GD_GN_GROUPS]);
  return TSD_OK;
}

extern "C" int tsd_debug_gemm_run(tsd_ctx* ctx, const int64_t* desc, int n, int cfg, const void* const* host_in,
                                  void* const* host_out, int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  if (cfg >= 0 && !gemm_tile(cfg)) TSD_FAIL(TSD_E_ARG, "gemm_run: unknown tile configuration %d", cfg);
  TSD_TRY(check_fields("gemm_run", n, TSD_GD_COUNT));
  TSD_TRY(gd_extents(desc, ext));
  if (!host_in) return TSD_OK;  // sizing only: no context or device needed
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("gemm_run", ext, TSD_GO_COUNT, TSD_GO_C, host_in, host_out));
  const int64_t* d = desc;
  const bool alias = (d[TSD_GD_EPI] & EPI_RESIDUAL) && (d[TSD_GD_ALIAS] & 1);  // in place: C starts as R, which gets no buffer of its own
  HIP_TRY(hipSetDevice(ctx->device));
  enum { W_TILE_MAJOR = TSD_GO_COUNT, W_UPS_FOLDED, SLOTS };  // the two weight copies the model path would have made: inputs like the others
  GuardedOperands ops(ctx, SLOTS);
  for (int s = 0; s < TSD_GO_C; s++)
    if (ext[s] && !(s == TSD_GO_R && alias)) TSD_TRY(ops.add(s, ext[s], gd_elem_bytes(s, d), host_in[s]));
  const replay::Box logical[] = {{d[TSD_GD_BATCH], d[TSD_GD_SC], d[TSD_GD_M], d[TSD_GD_LDC], gd_c_cols(d)},
                                 {d[TSD_GD_VT] ? d[TSD_GD_M] / d[TSD_GD_VT_S] : 0, d[TSD_GD_VT_SB], d[TSD_GD_N] - d[TSD_GD_VT_N0], d[TSD_GD_VT_LD], d[TSD_GD_VT_S]},
                                 replay::Box::dense(ext[TSD_GO_GN])};
  for (int s = TSD_GO_C; s < TSD_GO_COUNT; s++)
    if (ext[s])
      TSD_TRY(ops.add(s, ext[s], gd_elem_bytes(s, d), s == TSD_GO_C && alias ? host_in[TSD_GO_R] : nullptr, host_out[s - TSD_GO_C], logical[s - TSD_GO_C]));
  GemmArgs g = gd_args(d);
  g.A0 = (const half_t*)ops.at(TSD_GO_A0); g.A1 = (const half_t*)ops.at(TSD_GO_A1); g.A2 = (const half_t*)ops.at(TSD_GO_A2);
  g.Wt = (const half_t*)ops.at(TSD_GO_W); g.Wt1 = (const half_t*)ops.at(TSD_GO_WT1);
  g.bias = (const float*)ops.at(TSD_GO_BIAS); g.rowvec = (const float*)ops.at(TSD_GO_ROWVEC);
  g.R = (const half_t*)(alias ? ops.at(TSD_GO_C) : ops.at(TSD_GO_R));
  g.C = ops.at(TSD_GO_C);
  if (d[TSD_GD_VT]) g.Vt = (half_t*)ops.at(TSD_GO_VT);
  g.gn_part = (float*)ops.at(TSD_GO_GN);
  if (d[TSD_GD_W_KTS]) {  // the K-tile-major copy, made from the row-major W the caller passed
    const int KW = g.conv ? 9 * g.Cin : g.K;
    TSD_TRY(ops.add(W_TILE_MAJOR, (int64_t)g.N * KW, 2, nullptr));
    half_t* tm = (half_t*)ops.at(W_TILE_MAJOR);
    TSD_TRY(launch_pack_tile_major(ctx, g.Wt, g.N, KW, tm));
    g.Wt = tm;
  }
  if (g.conv && g.ups == 2 && g.Cin % 64 == 0 && host_in[TSD_GO_W]) {
    // the folded parity copies, made from the row-major W the caller passed by the routine tsd_model_prepare uses (model.cpp); whether the
    // launch may run them is launch_gemm's decision
    const int ld = d[TSD_GD_W_KTS] ? 9 * g.Cin : (int)d[TSD_GD_LDW];
    std::vector<uint16_t> folded((size_t)16 * g.N * g.Cin);
    (void)ups_fold_pack_host((const uint16_t*)host_in[TSD_GO_W], g.N, g.Cin, ld, folded.data());
    TSD_TRY(ops.add(W_UPS_FOLDED, (int64_t)folded.size(), 2, folded.data()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));  // the upload reads `folded`
    g.Wuf = (const half_t*)ops.at(W_UPS_FOLDED);
  }
  ctx->gemm_last = GemmPlan();
  int r;
  {  // the dispatcher's choice (with the recorded graph's long-K split) or a forced tile; a replay is not recorded
    Override<int> force(ctx->opt.force_cfg, cfg >= 0 ? cfg : -1);
    Override<int> big(ctx->opt.sk_big_graph, cfg < 0 ? (int)d[TSD_GD_SK_BIG] : ctx->opt.sk_big_graph);
    Override<bool> rec(ctx->gemm_rec_on, false);
    r = run_planned(ctx, [&]() -> int { return launch_gemm(ctx, g); });
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  info[0] = ctx->gemm_last.cfg; info[1] = ctx->gemm_last.cfg >= 0 ? ctx->gemm_last.ways : 0;
  TSD_TRY(ops.read_back(&info[2]));
  return r;
}

// ---- GroupNorm / LayerNorm launches on caller operands (tests/norm_ref.py holds every statistics path to an fp64 reference) ------
namespace {
// Element extent of every operand the described launch reads or writes.  Refuses what it cannot size; the shapes the launches
// themselves refuse (C % 8, C % groups, widths, pitches that are no multiple of 8) are sized and left to them.
int nd_extents(const int64_t* d, int64_t* e) {
  for (int i = 0; i < TSD_NO_COUNT; i++) e[i] = 0;
#define ND_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "norm_run: descriptor cannot be sized (%s)", #cond)
  ND_REQ(d[TSD_ND_VERSION] == TSD_ND_VERSION_1);
  const int64_t mode = d[TSD_ND_MODE], C = d[TSD_ND_C], lim = 1LL << 28;
  ND_REQ(mode >= TSD_NM_GROUPNORM && mode <= TSD_NM_LAYERNORM);
  ND_REQ(C > 0 && C <= 65536);
  for (int f : {TSD_ND_LD0, TSD_ND_LD1, TSD_ND_LDY}) ND_REQ(d[f] >= 0 && d[f] <= 65536);
  for (int f : {TSD_ND_SILU, TSD_ND_HAS_W, TSD_ND_HAS_B, TSD_ND_TORCH_RSTD}) ND_REQ(d[f] == 0 || d[f] == 1);
  if (d[TSD_ND_HAS_W]) e[TSD_NO_W] = C;
  if (d[TSD_ND_HAS_B]) e[TSD_NO_BIAS] = C;
  if (mode == TSD_NM_LAYERNORM) {
    const int64_t rows = d[TSD_ND_ROWS];
    ND_REQ(rows > 0 && rows < lim && d[TSD_ND_LD0] >= C && d[TSD_ND_LDY] >= C);
    e[TSD_NO_X0] = (rows - 1) * d[TSD_ND_LD0] + C;
    e[TSD_NO_Y] = (rows - 1) * d[TSD_ND_LDY] + C;
  } else {
    const int64_t B = d[TSD_ND_B], HW = d[TSD_ND_HW], G = d[TSD_ND_GROUPS], C0 = d[TSD_ND_C0], ns = d[TSD_ND_NSLAB];
    ND_REQ(B > 0 && B <= 4096 && HW > 0 && HW < lim && B * HW < lim && G > 0 && G <= C);
    if (mode == TSD_NM_GN_FINALIZE) {
      ND_REQ(ns > 0 && ns <= 65536);
      e[TSD_NO_PART0] = B * ns * G * 2;
      e[TSD_NO_STATS] = B * G * 2;
    } else {
      const int64_t px = B * HW;
      ND_REQ(C0 > 0 && C0 <= C && d[TSD_ND_LD0] >= C0);
      ND_REQ(mode == TSD_NM_GROUPNORM || C0 == C);
      e[TSD_NO_X0] = (px - 1) * d[TSD_ND_LD0] + C0;
      if (C0 < C) {
        ND_REQ(d[TSD_ND_LD1] >= C - C0);
        e[TSD_NO_X1] = (px - 1) * d[TSD_ND_LD1] + (C - C0);
      }
      if (mode == TSD_NM_GN_STATS) e[TSD_NO_STATS] = B * G * 2;
      else {
        ND_REQ(d[TSD_ND_LDY] >= C);
        e[TSD_NO_Y] = (px - 1) * d[TSD_ND_LDY] + C;
        const int64_t st = d[TSD_ND_STATS];
        ND_REQ(st >= 0 && st <= 2);
        if (st == 1) {
          ND_REQ(ns > 0 && ns <= 65536);
          e[TSD_NO_PART0] = B * ns * G * 2;
        } else if (st == 2) {
          const int64_t G0 = d[TSD_ND_G0], G1 = d[TSD_ND_G1];
          ND_REQ(ns > 0 && ns <= 65536 && G0 > 0 && G0 <= 65536 && G1 >= 0 && G1 <= 65536 && d[TSD_ND_COMB] >= 0 && d[TSD_ND_COMB] <= 65536);
          e[TSD_NO_PART0] = B * ns * G0 * 2;
          e[TSD_NO_PART1] = B * ns * G1 * 2;
        }
      }
    }
  }
  for (int s = 0; s < TSD_NO_COUNT; s++) ND_REQ(e[s] >= 0 && e[s] <= lim);
#undef ND_REQ
  return TSD_OK;
}
int nd_elem_bytes(int slot) { return slot == TSD_NO_X0 || slot == TSD_NO_X1 || slot == TSD_NO_Y ? 2 : 4; }
void nd_plan_info(const GnPlan& p, int64_t* info) {
  info[TSD_NI_NSLAB] = p.nslab; info[TSD_NI_OWN_PASS] = p.nslab > 0 && !p.have_stats ? 1 : 0; info[TSD_NI_PREREDUCE] = p.prereduce ? 1 : 0;
  info[TSD_NI_FINALIZE] = p.stats_ready; info[TSD_NI_COMPOSITE] = p.composite ? 1 : 0; info[TSD_NI_SLAB_PIXELS] = p.slab_pixels;
  info[TSD_NI_APPLY_PIXELS] = p.apply_pixels; info[TSD_NI_PL] = p.PL;
}
}  // namespace

extern "C" int tsd_debug_norm_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                  int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  TSD_TRY(check_fields("norm_run", n, TSD_ND_COUNT));
  TSD_TRY(nd_extents(desc, ext));
  const int64_t* d = desc;
  const int mode = (int)d[TSD_ND_MODE], B = (int)d[TSD_ND_B], HW = (int)d[TSD_ND_HW], C = (int)d[TSD_ND_C], G = (int)d[TSD_ND_GROUPS];
  const int ns = (int)d[TSD_ND_NSLAB];
  if (info) for (int i = 0; i < TSD_NI_COUNT; i++) info[i] = 0;
  // a non-NULL marker stands for the tables: the plan looks at which pointers are given, never through them
  static const float marker = 0.f;
  auto composite_of = [&](const float* p0, const float* p1) {
    GnComposite gc;
    gc.part0 = p0; gc.G0 = (int)d[TSD_ND_G0]; gc.part1 = d[TSD_ND_G1] > 0 ? p1 : nullptr; gc.G1 = (int)d[TSD_ND_G1];
    gc.nslab = ns; gc.comb = (int)d[TSD_ND_COMB];
    return gc;
  };
  if (!host_in) {  // sizing only: no context or device needed; the plan under the default options
    if (info && (mode == TSD_NM_GROUPNORM || mode == TSD_NM_GN_STATS) && C % 8 == 0 && C % G == 0 && C <= 4096) {
      const int st = mode == TSD_NM_GROUPNORM ? (int)d[TSD_ND_STATS] : 0;
      const GnComposite gc = composite_of(&marker, &marker);
      GnPlan p = gn_plan(TsdOptions(), HW, C, G, st == 1 ? &marker : nullptr, st == 1 ? ns : 0, st == 2 ? &gc : nullptr);
      if (mode == TSD_NM_GN_STATS) p.stats_ready = 1;
      nd_plan_info(p, info);
    }
    return TSD_OK;
  }
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("norm_run", ext, TSD_NO_COUNT, TSD_NO_Y, host_in, host_out));
  HIP_TRY(hipSetDevice(ctx->device));
  GuardedOperands ops(ctx, TSD_NO_COUNT);
  for (int s = 0; s < TSD_NO_Y; s++)
    if (ext[s]) TSD_TRY(ops.add(s, ext[s], nd_elem_bytes(s), host_in[s]));
  const int64_t rows = mode == TSD_NM_LAYERNORM ? d[TSD_ND_ROWS] : (int64_t)B * HW;
  if (ext[TSD_NO_Y]) TSD_TRY(ops.add(TSD_NO_Y, ext[TSD_NO_Y], 2, nullptr, host_out[0], replay::Box{1, 0, rows, d[TSD_ND_LDY], C}));
  if (ext[TSD_NO_STATS]) TSD_TRY(ops.add(TSD_NO_STATS, ext[TSD_NO_STATS], 4, nullptr, host_out[1], replay::Box::dense(ext[TSD_NO_STATS])));
  const float eps = f32_of(d[TSD_ND_EPS]), gamma = f32_of(d[TSD_ND_GAMMA]);
  NormAffine aff;
  aff.w = (const float*)ops.at(TSD_NO_W); aff.b = (const float*)ops.at(TSD_NO_BIAS); aff.torch_rstd = (int)d[TSD_ND_TORCH_RSTD];
  const NormAffine* affp = (aff.w || aff.b || aff.torch_rstd) ? &aff : nullptr;
  ctx->gn_last = GnPlan();
  const int r = run_planned(ctx, [&]() -> int {
    if (mode == TSD_NM_LAYERNORM)
      return launch_layernorm(ctx, (const half_t*)ops.at(TSD_NO_X0), d[TSD_ND_ROWS], C, (int)d[TSD_ND_LD0], eps, (half_t*)ops.at(TSD_NO_Y),
                              (int)d[TSD_ND_LDY], affp);
    if (mode == TSD_NM_GN_FINALIZE)
      return launch_gn_finalize(ctx, (const float*)ops.at(TSD_NO_PART0), ns, B, HW, C, G, eps, gamma, (float*)ops.at(TSD_NO_STATS));
    if (mode == TSD_NM_GN_STATS)
      return launch_gn_stats(ctx, (const half_t*)ops.at(TSD_NO_X0), (int)d[TSD_ND_LD0], B, HW, C, G, eps, gamma, (float*)ops.at(TSD_NO_STATS));
    NormSrc src;
    src.x0 = (const half_t*)ops.at(TSD_NO_X0); src.ld0 = (int)d[TSD_ND_LD0]; src.C0 = (int)d[TSD_ND_C0];
    src.x1 = (const half_t*)ops.at(TSD_NO_X1); src.ld1 = (int)d[TSD_ND_LD1];
    const int sm = (int)d[TSD_ND_STATS];
    const GnComposite gc = composite_of((const float*)ops.at(TSD_NO_PART0), (const float*)ops.at(TSD_NO_PART1));
    return launch_groupnorm(ctx, src, B, HW, C, G, eps, gamma, (int)d[TSD_ND_SILU], (half_t*)ops.at(TSD_NO_Y), (int)d[TSD_ND_LDY],
                            sm == 1 ? (const float*)ops.at(TSD_NO_PART0) : nullptr, sm == 1 ? ns : 0, affp, sm == 2 ? &gc : nullptr);
  });
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  nd_plan_info(ctx->gn_last, info);  // what the launch itself planned (zeros when it was refused)
  TSD_TRY(ops.read_back(&info[TSD_NI_CHANGED]));
  return r;
}

// ---- attention core / row softmax on caller operands (tests/attn_ref.py holds every kernel to an fp64 reference) ---------------------
namespace {
int ad_elem_bytes(int slot, const int64_t* d) {
  return d[TSD_AD_MODE] == TSD_AM_SOFTMAX_ROWS && d[TSD_AD_DTYPE] == 0 && (slot == TSD_AO_X || slot == TSD_AO_O) ? 4 : 2;
}
// Element extent of every operand the described launch reads or writes.  An empty sequence is sized as one row (the launcher refuses it).
int ad_extents(const int64_t* d, int64_t* e) {
  for (int i = 0; i < TSD_AO_COUNT; i++) e[i] = 0;
#define AD_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "attn_run: descriptor cannot be sized (%s)", #cond)
  AD_REQ(d[TSD_AD_VERSION] == TSD_AD_VERSION_1 || d[TSD_AD_VERSION] == TSD_AD_VERSION_2);
  const int64_t mode = d[TSD_AD_MODE], lim = 1LL << 28;
  AD_REQ(mode == TSD_AM_ATTN || mode == TSD_AM_SOFTMAX_ROWS);
  if (mode == TSD_AM_ATTN) {
    const int64_t B = d[TSD_AD_B], H = d[TSD_AD_H], hd = d[TSD_AD_D];
    const int64_t Sq = std::max<int64_t>(d[TSD_AD_SQ], 1), Sk = std::max<int64_t>(d[TSD_AD_SK], 1);
    AD_REQ(B > 0 && B <= 4096 && H > 0 && H <= 4096 && hd > 0 && hd <= 4096 && H * hd <= 65536);
    AD_REQ(d[TSD_AD_SQ] >= 0 && d[TSD_AD_SK] >= 0 && Sq <= (1 << 20) && Sk <= (1 << 20));
    AD_REQ(d[TSD_AD_KERNEL] >= 0 && d[TSD_AD_KERNEL] <= 3 && (d[TSD_AD_DIAG] == 0 || d[TSD_AD_DIAG] == 1));
    const int64_t C = H * hd;
    for (int f : {TSD_AD_LDQ, TSD_AD_LDK, TSD_AD_LDO}) AD_REQ(d[f] >= C && d[f] <= (1 << 20));
    AD_REQ(d[TSD_AD_LDVT] >= Sk && d[TSD_AD_LDVT] <= (1 << 21));
    const int64_t Skv = std::min((Sk + 7) / 8 * 8, d[TSD_AD_LDVT]);
    AD_REQ(d[TSD_AD_SQB] >= Sq * d[TSD_AD_LDQ] && d[TSD_AD_SKB] >= Sk * d[TSD_AD_LDK] && d[TSD_AD_SVTB] >= C * d[TSD_AD_LDVT] &&
           d[TSD_AD_SOB] >= Sq * d[TSD_AD_LDO]);
    for (int f : {TSD_AD_SQB, TSD_AD_SKB, TSD_AD_SVTB, TSD_AD_SOB}) AD_REQ(d[f] < lim);
    e[TSD_AO_Q] = (B - 1) * d[TSD_AD_SQB] + (Sq - 1) * d[TSD_AD_LDQ] + C;
    e[TSD_AO_K] = (B - 1) * d[TSD_AD_SKB] + (Sk - 1) * d[TSD_AD_LDK] + C;
    e[TSD_AO_VT] = (B - 1) * d[TSD_AD_SVTB] + (C - 1) * d[TSD_AD_LDVT] + Skv;
    e[TSD_AO_O] = (B - 1) * d[TSD_AD_SOB] + (Sq - 1) * d[TSD_AD_LDO] + C;
  } else {
    const int64_t rows = d[TSD_AD_ROWS], cols = d[TSD_AD_COLS], ld = d[TSD_AD_LD], zt = d[TSD_AD_ZERO_TO];
    AD_REQ(rows > 0 && rows <= (1 << 20) && cols > 0 && cols <= (1 << 20) && ld >= cols && ld <= (1 << 20));
    AD_REQ(d[TSD_AD_DTYPE] == 0 || d[TSD_AD_DTYPE] == 1);
    AD_REQ(d[TSD_AD_CAUSAL] >= 0 && d[TSD_AD_CAUSAL] <= (1 << 20) && zt >= 0);
    if (d[TSD_AD_DTYPE] == 0) AD_REQ(ld == cols && d[TSD_AD_CAUSAL] == 0 && zt == 0);  // launch_softmax_rows_f32 is dense and never causal
    if (d[TSD_AD_CAUSAL] == 0) AD_REQ(zt == 0);
    AD_REQ(zt <= ld);  // a wider ZERO_TO would be written outside the operand; launch_softmax_rows_f16_causal refuses it as well
    e[TSD_AO_X] = e[TSD_AO_O] = (rows - 1) * ld + std::max(cols, zt);
  }
  for (int s = 0; s < TSD_AO_COUNT; s++) AD_REQ(e[s] >= 0 && e[s] <= lim);
#undef AD_REQ
  return TSD_OK;
}
}  // namespace

extern "C" int tsd_debug_attn_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                  int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  TSD_TRY(check_fields("attn_run", n, TSD_AD_COUNT));
  TSD_TRY(ad_extents(desc, ext));
  const int64_t* d = desc;
  const bool attn = d[TSD_AD_MODE] == TSD_AM_ATTN;
  // head dimension 64 came with version 2: a version-1 descriptor is sized and refused as it was before the d = 64 kernel existed
  const bool v1_d64 = attn && d[TSD_AD_VERSION] == TSD_AD_VERSION_1 && d[TSD_AD_D] == 64;
  if (info) for (int i = 0; i < TSD_AI_COUNT; i++) info[i] = 0;
  if (!host_in) {  // sizing only: no context or device needed; the dispatcher's choice under the default options
    if (info && attn && !v1_d64 && attn_fused_supported((int)d[TSD_AD_D]) && d[TSD_AD_SQ] > 0 && d[TSD_AD_SK] > 0) {
      TsdOptions o;
      o.attn_qb_force = (int)d[TSD_AD_KERNEL]; o.attn_diag = (int)d[TSD_AD_DIAG];
      const AttnPlan p = attn_plan(o, (int)d[TSD_AD_B], (int)d[TSD_AD_H], (int)d[TSD_AD_D], (int)d[TSD_AD_SQ], (int)d[TSD_AD_SK]);
      info[TSD_AI_KERNEL] = p.kernel; info[TSD_AI_DIAG] = p.diag; info[TSD_AI_XCD_MAP] = p.xcd_map;
    }
    return TSD_OK;
  }
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("attn_run", ext, TSD_AO_COUNT, TSD_AO_O, host_in, host_out));
  HIP_TRY(hipSetDevice(ctx->device));
  GuardedOperands ops(ctx, TSD_AO_COUNT);
  for (int s = 0; s < TSD_AO_O; s++)
    if (ext[s]) TSD_TRY(ops.add(s, ext[s], ad_elem_bytes(s, d), host_in[s]));
  const bool inplace = !attn && d[TSD_AD_DTYPE] == 1;  // fp16 rows are overwritten in place: O starts as X
  const replay::Box logical = attn ? replay::Box{d[TSD_AD_B], d[TSD_AD_SOB], d[TSD_AD_SQ], d[TSD_AD_LDO], d[TSD_AD_H] * d[TSD_AD_D]}
                                   : replay::Box{1, 0, d[TSD_AD_ROWS], d[TSD_AD_LD], std::max(d[TSD_AD_COLS], d[TSD_AD_ZERO_TO])};
  TSD_TRY(ops.add(TSD_AO_O, ext[TSD_AO_O], ad_elem_bytes(TSD_AO_O, d), inplace ? host_in[TSD_AO_X] : nullptr, host_out[0], logical));
  int exact0 = 0, exact1 = 0;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(&exact0, ctx->status + 2, sizeof(int), hipMemcpyDeviceToHost));
  ctx->attn_last = AttnPlan();
  int r;
  if (attn) {
    Override<int> force(ctx->opt.attn_qb_force, (int)d[TSD_AD_KERNEL]), diag(ctx->opt.attn_diag, (int)d[TSD_AD_DIAG]);
    AttnArgs a;
    a.Q = (const half_t*)ops.at(TSD_AO_Q); a.ldq = (int)d[TSD_AD_LDQ]; a.sQ = d[TSD_AD_SQB];
    a.K = (const half_t*)ops.at(TSD_AO_K); a.ldk = (int)d[TSD_AD_LDK]; a.sK = d[TSD_AD_SKB];
    a.Vt = (const half_t*)ops.at(TSD_AO_VT); a.ldvt = (int)d[TSD_AD_LDVT]; a.sVt = d[TSD_AD_SVTB];
    a.O = (half_t*)ops.at(TSD_AO_O); a.ldo = (int)d[TSD_AD_LDO]; a.sO = d[TSD_AD_SOB];
    a.B = (int)d[TSD_AD_B]; a.H = (int)d[TSD_AD_H]; a.d = (int)d[TSD_AD_D]; a.Sq = (int)d[TSD_AD_SQ]; a.Sk = (int)d[TSD_AD_SK];
    a.scale = f32_of(d[TSD_AD_SCALE]);
    r = run_planned(ctx, [&]() -> int {
      if (v1_d64) TSD_FAIL(TSD_E_SHAPE, "flash attention: head dim %d unsupported", a.d);
      return launch_flash_attention(ctx, a);
    });
  } else {
    const int64_t rows = d[TSD_AD_ROWS];
    const int cols = (int)d[TSD_AD_COLS], ld = (int)d[TSD_AD_LD];
    r = run_planned(ctx, [&]() -> int {
      if (d[TSD_AD_DTYPE] == 0) return launch_softmax_rows_f32(ctx, (const float*)ops.at(TSD_AO_X), rows, cols, (float*)ops.at(TSD_AO_O));
      if (d[TSD_AD_CAUSAL] > 0)
        return launch_softmax_rows_f16_causal(ctx, (half_t*)ops.at(TSD_AO_O), rows, cols, ld, (int)d[TSD_AD_CAUSAL], (int)d[TSD_AD_ZERO_TO]);
      return launch_softmax_rows_f16(ctx, (half_t*)ops.at(TSD_AO_O), rows, cols, ld);
    });
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(&exact1, ctx->status + 2, sizeof(int), hipMemcpyDeviceToHost));
  info[TSD_AI_KERNEL] = attn ? ctx->attn_last.kernel : ctx->attn_last.softmax;
  info[TSD_AI_DIAG] = ctx->attn_last.diag; info[TSD_AI_XCD_MAP] = ctx->attn_last.xcd_map;
  info[TSD_AI_EXACT_WGS] = exact1 - exact0;
  TSD_TRY(ops.read_back(&info[TSD_AI_CHANGED]));
  return r;
}

// ---- fused attention-block head / tail on caller operands (tests/chain_ref.py holds both kernels and the packers to an fp64 reference) ----
// (The tail's pad contract for the context operands is stated beside the entry's declaration, include/tsd.h.)
namespace {
int cd_elem_bytes(int slot) {
  return (slot >= TSD_CO_BSO && slot <= TSD_CO_GN_STATS) || slot == TSD_CO_B_IN || slot == TSD_CO_GN_PART ? 4 : 2;
}
// Element extent of every operand the described launch reads or writes.  Refuses what it cannot size; what the launchers refuse (S % 64,
// T outside 1 .. 80 - sized as one key -, narrow or misaligned pitches, other C / d / heads, the fused path switched off) is left to them.
int cd_extents(const int64_t* d, int64_t* e) {
  for (int i = 0; i < TSD_CO_COUNT; i++) e[i] = 0;
#define CD_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "chain_run: descriptor cannot be sized (%s)", #cond)
  CD_REQ(d[TSD_CD_VERSION] == TSD_CD_VERSION_1);
  const int64_t mode = d[TSD_CD_MODE], B = d[TSD_CD_B], S = d[TSD_CD_S], C = d[TSD_CD_C], lim = 1LL << 28;
  CD_REQ(mode == TSD_CM_HEAD || mode == TSD_CM_TAIL);
  CD_REQ(B > 0 && B <= 4096 && S > 0 && S <= (1 << 20) && B * S < (1 << 24));
  CD_REQ(C > 0 && C <= 4096 && d[TSD_CD_D] > 0 && d[TSD_CD_D] <= 4096 && d[TSD_CD_HEADS] > 0 && d[TSD_CD_HEADS] <= 4096);
  const int64_t M = B * S, ld_max = 1 << 21;  // one cap for every pitch: the head's V^T pitch spans a sample's S <= 2^20 tokens
  auto rows = [&](int64_t n, int f, int64_t width) { return (n - 1) * d[f] + width; };
  if (mode == TSD_CM_TAIL) {
    const int64_t T = d[TSD_CD_T], Tk = std::max<int64_t>(T, 1);
    CD_REQ(T >= 0 && T <= 4096 && (d[TSD_CD_GN] == 0 || d[TSD_CD_GN] == 1));
    for (int f : {TSD_CD_LD_AO, TSD_CD_LD_TOK, TSD_CD_LD_X, TSD_CD_LD_OUT, TSD_CD_LDK, TSD_CD_LDVT, TSD_CD_LDW_SO, TSD_CD_LDW_Q, TSD_CD_LDW_CO,
                  TSD_CD_LDW_1, TSD_CD_LDW_2, TSD_CD_LDW_OUT})
      CD_REQ(d[f] > 0 && d[f] <= ld_max);
    const int64_t Tv = std::min((Tk + 7) / 8 * 8, d[TSD_CD_LDVT]);
    CD_REQ(d[TSD_CD_SKB] >= Tk * d[TSD_CD_LDK] && d[TSD_CD_SVTB] >= C * d[TSD_CD_LDVT] && d[TSD_CD_SKB] < lim && d[TSD_CD_SVTB] < lim);
    e[TSD_CO_AO] = rows(M, TSD_CD_LD_AO, C); e[TSD_CO_TOK] = rows(M, TSD_CD_LD_TOK, C); e[TSD_CO_X] = rows(M, TSD_CD_LD_X, C);
    e[TSD_CO_KC] = (B - 1) * d[TSD_CD_SKB] + rows(Tk, TSD_CD_LDK, C);
    e[TSD_CO_VT] = (B - 1) * d[TSD_CD_SVTB] + rows(C, TSD_CD_LDVT, Tv);
    e[TSD_CO_WSO] = rows(C, TSD_CD_LDW_SO, C); e[TSD_CO_WQ] = rows(C, TSD_CD_LDW_Q, C); e[TSD_CO_WCO] = rows(C, TSD_CD_LDW_CO, C);
    e[TSD_CO_W1] = rows(8 * C, TSD_CD_LDW_1, C); e[TSD_CO_W2] = rows(C, TSD_CD_LDW_2, 4 * C); e[TSD_CO_WOUT] = rows(C, TSD_CD_LDW_OUT, C);
    e[TSD_CO_BSO] = e[TSD_CO_BCO] = e[TSD_CO_B2] = e[TSD_CO_BOUT] = C;
    e[TSD_CO_B1] = 8 * C;
    e[TSD_CO_OUT] = rows(M, TSD_CD_LD_OUT, C);
    if (d[TSD_CD_GN]) e[TSD_CO_GN_PART] = B * (S / 32) * 32 * 2;  // nslab = S / 32, as the launch is given it
  } else {
    for (int f : {TSD_CD_LD_X, TSD_CD_LD_TOK, TSD_CD_LD_QK, TSD_CD_LD_VT, TSD_CD_LDW_C, TSD_CD_LDW_IN}) CD_REQ(d[f] > 0 && d[f] <= ld_max);
    CD_REQ(d[TSD_CD_S_VT] >= C * d[TSD_CD_LD_VT] && d[TSD_CD_S_VT] < lim);
    e[TSD_CO_X] = rows(M, TSD_CD_LD_X, C);
    e[TSD_CO_GN_STATS] = B * 32 * 2;
    e[TSD_CO_WC] = rows(C, TSD_CD_LDW_C, C); e[TSD_CO_WIN] = rows(3 * C, TSD_CD_LDW_IN, C);
    e[TSD_CO_B_IN] = C;
    e[TSD_CO_HTOK] = rows(M, TSD_CD_LD_TOK, C); e[TSD_CO_QK] = rows(M, TSD_CD_LD_QK, 2 * C);
    e[TSD_CO_HVT] = (B - 1) * d[TSD_CD_S_VT] + rows(C, TSD_CD_LD_VT, S);
  }
  for (int s = 0; s < TSD_CO_COUNT; s++) CD_REQ(e[s] >= 0 && e[s] <= lim);
#undef CD_REQ
  return TSD_OK;
}
}  // namespace

extern "C" int tsd_debug_chain_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                   int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  TSD_TRY(check_fields("chain_run", n, TSD_CD_COUNT));
  TSD_TRY(cd_extents(desc, ext));
  const int64_t* d = desc;
  if (info) for (int i = 0; i < TSD_CI_COUNT; i++) info[i] = 0;
  if (!host_in) return TSD_OK;  // sizing only: no context or device needed
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("chain_run", ext, TSD_CO_COUNT, TSD_CO_OUT, host_in, host_out));
  HIP_TRY(hipSetDevice(ctx->device));
  const bool tail = d[TSD_CD_MODE] == TSD_CM_TAIL;
  const int64_t B = d[TSD_CD_B], S = d[TSD_CD_S], M = B * S, C = d[TSD_CD_C];
  enum { W_STREAM = TSD_CO_COUNT, SLOTS };  // the packed weight stream the model path would have made: an input like the others
  GuardedOperands ops(ctx, SLOTS);
  for (int s = 0; s < TSD_CO_OUT; s++)
    if (ext[s]) TSD_TRY(ops.add(s, ext[s], cd_elem_bytes(s), host_in[s]));
  const replay::Box logical[] = {{1, 0, M, d[TSD_CD_LD_OUT], C},
                                 replay::Box::dense(ext[TSD_CO_GN_PART]),
                                 {1, 0, M, d[TSD_CD_LD_TOK], C},
                                 {1, 0, M, d[TSD_CD_LD_QK], 2 * C},
                                 {B, d[TSD_CD_S_VT], C, d[TSD_CD_LD_VT], S}};
  for (int s = TSD_CO_OUT; s < TSD_CO_COUNT; s++)
    if (ext[s]) TSD_TRY(ops.add(s, ext[s], cd_elem_bytes(s), nullptr, host_out[s - TSD_CO_OUT], logical[s - TSD_CO_OUT]));
  auto h = [&](int s) { return (const half_t*)ops.at(s); };
  auto f = [&](int s) { return (const float*)ops.at(s); };
  // the packers read fixed 320-wide shapes: they see the caller's weights only when those have that shape (every other C is refused by
  // the launch below, with the stream left as the fill)
  const bool packable = C == 320;
  TSD_TRY(ops.add(W_STREAM, (int64_t)((tail ? attn_tail_stream_bytes() : attn_head_stream_bytes()) / 2), 2, nullptr));
  half_t* ws = (half_t*)ops.at(W_STREAM);
  int r = TSD_OK;
  if (packable)
    r = tail ? launch_attn_tail_pack(ctx, h(TSD_CO_WSO), (int)d[TSD_CD_LDW_SO], h(TSD_CO_WQ), (int)d[TSD_CD_LDW_Q], h(TSD_CO_WCO),
                                     (int)d[TSD_CD_LDW_CO], h(TSD_CO_W1), (int)d[TSD_CD_LDW_1], h(TSD_CO_W2), (int)d[TSD_CD_LDW_2],
                                     h(TSD_CO_WOUT), (int)d[TSD_CD_LDW_OUT], ws)
             : launch_attn_head_pack(ctx, h(TSD_CO_WC), (int)d[TSD_CD_LDW_C], h(TSD_CO_WIN), (int)d[TSD_CD_LDW_IN], ws);
  bool ran = false;
  if (r == TSD_OK)
    r = run_planned(ctx, [&]() -> int {
      if (tail) {
        AttnTailArgs a;
        a.ao = h(TSD_CO_AO); a.ld_ao = (int)d[TSD_CD_LD_AO]; a.tok = h(TSD_CO_TOK); a.ld_tok = (int)d[TSD_CD_LD_TOK];
        a.x = h(TSD_CO_X); a.ld_x = (int)d[TSD_CD_LD_X]; a.out = (half_t*)ops.at(TSD_CO_OUT); a.ld_out = (int)d[TSD_CD_LD_OUT];
        a.wstream = ws;
        a.bso = f(TSD_CO_BSO); a.bco = f(TSD_CO_BCO); a.b1 = f(TSD_CO_B1); a.b2 = f(TSD_CO_B2); a.bout = f(TSD_CO_BOUT);
        a.Kc = h(TSD_CO_KC); a.ldk = (int)d[TSD_CD_LDK]; a.sK = d[TSD_CD_SKB];
        a.Vt = h(TSD_CO_VT); a.ldvt = (int)d[TSD_CD_LDVT]; a.sVt = d[TSD_CD_SVTB];
        a.C = (int)C; a.d = (int)d[TSD_CD_D]; a.heads = (int)d[TSD_CD_HEADS]; a.T = (int)d[TSD_CD_T]; a.S = (int)S; a.M = M;
        a.scale = f32_of(d[TSD_CD_SCALE]); a.eps = f32_of(d[TSD_CD_EPS]);
        if (d[TSD_CD_GN]) { a.gn_part = (float*)ops.at(TSD_CO_GN_PART); a.gn_nslab = (int)(S / 32); }
        TSD_TRY(launch_attn_tail(ctx, a));
      } else {
        // launch_attn_head takes no width: its callers ask attn_tail_supported first (g_unet_attn), and so does this one
        if (!attn_tail_supported(ctx, (int)C, (int)d[TSD_CD_D], (int)d[TSD_CD_HEADS], 1, M, (int)S))
          TSD_FAIL(TSD_E_SHAPE, "attention head: unsupported shape");
        AttnHeadArgs a;
        a.x = h(TSD_CO_X); a.ld_x = (int)d[TSD_CD_LD_X]; a.gn_stats = f(TSD_CO_GN_STATS); a.wstream = ws; a.b_in = f(TSD_CO_B_IN);
        a.tok = (half_t*)ops.at(TSD_CO_HTOK); a.ld_tok = (int)d[TSD_CD_LD_TOK]; a.qk = (half_t*)ops.at(TSD_CO_QK); a.ld_qk = (int)d[TSD_CD_LD_QK];
        a.vt = (half_t*)ops.at(TSD_CO_HVT); a.ld_vt = (int)d[TSD_CD_LD_VT]; a.s_vt = d[TSD_CD_S_VT];
        a.M = M; a.S = (int)S; a.eps = f32_of(d[TSD_CD_EPS]);
        TSD_TRY(launch_attn_head(ctx, a));
      }
      ran = ctx->launch();
      return TSD_OK;
    });
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  info[TSD_CI_RAN] = ran ? 1 : 0;
  TSD_TRY(ops.read_back(&info[TSD_CI_CHANGED]));
  return r;
}

// ---- time path / activations / layout conversions / packers on caller operands (tests/elem_ref.py holds each to an fp64 reference) ----
namespace {
int ed_elem_bytes(int mode, int slot, const int64_t* d) {
  const bool y = slot == TSD_EO_Y;
  switch (mode) {
    case TSD_EM_SMALL_LINEAR: return slot == TSD_EO_W ? 2 : 4;
    case TSD_EM_GEGLU_ERF: case TSD_EM_QUICK_GELU: case TSD_EM_PACK_IM2COL_W: return 2;
    case TSD_EM_CLIP_EMBED: return slot == TSD_EO_W || y ? 2 : 4;
    case TSD_EM_CHW_TO_NHWC: case TSD_EM_IM2COL3X3: case TSD_EM_F32_TO_F16_ROWS: case TSD_EM_TRANSPOSE_TO_F16: case TSD_EM_PACK_CONV:
    case TSD_EM_PACK_LINEAR: return y ? 2 : 4;
    case TSD_EM_NHWC_TO_CHW: return !y && d[TSD_ED_DTYPE] == 1 ? 2 : 4;
    case TSD_EM_F16_TO_F32_ROWS: return y ? 4 : 2;
    default: return 4;  // TIME_EMBEDDING, UNARY, PACK_BIAS, ENCODER_SAMPLE
  }
}
// Element extent of every operand the described launch reads or writes, and the output's logical elements.  Refuses what it cannot size;
// the shapes the launchers themselves refuse are sized and left to them.
int ed_extents(const int64_t* d, int64_t* e, replay::Box* box) {
  for (int i = 0; i < TSD_EO_COUNT; i++) e[i] = 0;
#define ED_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "elem_run: descriptor cannot be sized (%s)", #cond)
  ED_REQ(d[TSD_ED_VERSION] == TSD_ED_VERSION_1);
  const int64_t mode = d[TSD_ED_MODE], lim = 1LL << 26, dim = 1 << 20;
  ED_REQ(mode >= 0 && mode < TSD_EM_COUNT);
  for (int f = TSD_ED_B; f < TSD_ED_COUNT; f++)
    if (f != TSD_ED_SCALE && f != TSD_ED_T_BITS) ED_REQ(d[f] >= 0 && d[f] <= (f == TSD_ED_N ? lim : dim));
  for (int f : {TSD_ED_SILU, TSD_ED_HAS_BIAS, TSD_ED_HAS_T, TSD_ED_INTERLEAVE, TSD_ED_DTYPE}) ED_REQ(d[f] == 0 || d[f] == 1);
  const int64_t B = d[TSD_ED_B], K = d[TSD_ED_K], N = d[TSD_ED_N], C = d[TSD_ED_C], HW = d[TSD_ED_H] * d[TSD_ED_W];
  const int64_t rows = d[TSD_ED_ROWS], cols = d[TSD_ED_COLS], ld = d[TSD_ED_LD];
  int64_t &x = e[TSD_EO_X], &w = e[TSD_EO_W], &bias = e[TSD_EO_BIAS], &y = e[TSD_EO_Y];
  *box = replay::Box();
  switch (mode) {
    case TSD_EM_SMALL_LINEAR:
      ED_REQ(B > 0 && B <= 64 && K > 0 && K <= 65536 && N > 0 && N <= 65536);
      ED_REQ(d[TSD_ED_LDX] >= K && d[TSD_ED_LDW] >= K && d[TSD_ED_LDY] >= N);
      x = (B - 1) * d[TSD_ED_LDX] + K; w = (N - 1) * d[TSD_ED_LDW] + K; bias = d[TSD_ED_HAS_BIAS] ? N : 0;
      y = (B - 1) * d[TSD_ED_LDY] + N;
      *box = replay::Box{1, 0, B, d[TSD_ED_LDY], N};
      break;
    case TSD_EM_TIME_EMBEDDING:
      ED_REQ(B > 0 && B <= 4096);
      x = d[TSD_ED_HAS_T] ? B : 0; y = B * 320;
      break;
    case TSD_EM_GEGLU_ERF:
      ED_REQ(rows > 0 && cols > 0);
      x = rows * 2 * cols; y = rows * cols;
      break;
    case TSD_EM_QUICK_GELU:
      ED_REQ(N > 0);
      x = y = N;
      break;
    case TSD_EM_UNARY:
      ED_REQ(N > 0 && d[TSD_ED_OP] <= 2);
      x = y = N;
      break;
    case TSD_EM_CLIP_EMBED:
      ED_REQ(B > 0 && d[TSD_ED_T] > 0 && d[TSD_ED_V] > 0 && d[TSD_ED_D] > 0 && B * d[TSD_ED_T] <= dim);
      x = B * d[TSD_ED_T]; w = d[TSD_ED_V] * d[TSD_ED_D]; bias = d[TSD_ED_T] * d[TSD_ED_D]; y = x * d[TSD_ED_D];
      break;
    case TSD_EM_CHW_TO_NHWC:
      ED_REQ(B > 0 && C > 0 && HW > 0 && HW <= lim && d[TSD_ED_CUSE] <= C && d[TSD_ED_CDST] > 0);
      x = B * C * HW; y = B * HW * d[TSD_ED_CDST];
      break;
    case TSD_EM_IM2COL3X3:
      ED_REQ(B > 0 && C > 0 && HW > 0 && HW <= lim);
      x = B * C * HW; y = B * HW * 64;
      break;
    case TSD_EM_NHWC_TO_CHW:
      ED_REQ(B > 0 && C > 0 && HW > 0 && HW <= lim && B * HW <= lim && ld >= C);
      x = (B * HW - 1) * ld + C; y = B * C * HW;
      break;
    case TSD_EM_F32_TO_F16_ROWS:
      ED_REQ(rows > 0 && cols > 0 && ld >= cols && d[TSD_ED_ROWS_DST] >= rows);
      x = rows * cols; y = d[TSD_ED_ROWS_DST] * ld;
      break;
    case TSD_EM_F16_TO_F32_ROWS:
      ED_REQ(rows > 0 && cols > 0 && ld >= cols);
      x = (rows - 1) * ld + cols; y = rows * cols;
      break;
    case TSD_EM_TRANSPOSE_TO_F16:
      ED_REQ(B > 0 && B <= 4096 && K > 0 && K <= 65536 && N > 0 && N <= 65536 && d[TSD_ED_KPAD] >= K && d[TSD_ED_NPAD] >= N && d[TSD_ED_KPAD] <= 65536 &&
             d[TSD_ED_NPAD] <= 65536);
      x = B * K * N; y = B * d[TSD_ED_NPAD] * d[TSD_ED_KPAD];
      break;
    case TSD_EM_PACK_CONV: {
      const int64_t O = d[TSD_ED_O], I = d[TSD_ED_I], k = d[TSD_ED_KSIZE];
      ED_REQ(O > 0 && O <= 65536 && I > 0 && I <= 65536 && k > 0 && k <= 7 && d[TSD_ED_OPAD] >= O && d[TSD_ED_OPAD] <= 65536 && d[TSD_ED_IPAD] >= I &&
             d[TSD_ED_IPAD] <= 65536);
      x = O * I * k * k; y = d[TSD_ED_OPAD] * k * k * d[TSD_ED_IPAD];
      break;
    }
    case TSD_EM_PACK_LINEAR:
      ED_REQ(N > 0 && N <= 65536 && K > 0 && K <= 65536 && d[TSD_ED_KPAD] >= K && d[TSD_ED_KPAD] <= 65536 && (!d[TSD_ED_INTERLEAVE] || N % 2 == 0));
      x = N * K; y = N * d[TSD_ED_KPAD];
      break;
    case TSD_EM_PACK_BIAS:
      ED_REQ(N > 0 && N <= dim && d[TSD_ED_NPAD] >= N && (!d[TSD_ED_INTERLEAVE] || N % 2 == 0));
      x = N; y = d[TSD_ED_NPAD];
      break;
    case TSD_EM_PACK_IM2COL_W:
      ED_REQ(d[TSD_ED_O] > 0 && d[TSD_ED_O] <= 65536 && d[TSD_ED_IPAD] > 0 && d[TSD_ED_IPAD] <= 65536 && C > 0);
      x = d[TSD_ED_O] * 9 * d[TSD_ED_IPAD]; y = d[TSD_ED_O] * 64;
      break;
    default: {  // TSD_EM_ENCODER_SAMPLE
      const int64_t hw = d[TSD_ED_HW];
      ED_REQ(B > 0 && B <= 4096 && hw > 0 && B * hw <= lim && ld >= 8);
      x = (B * hw - 1) * ld + 8; w = y = B * 4 * hw;
      break;
    }
  }
  if (mode != TSD_EM_SMALL_LINEAR) *box = replay::Box::dense(y);
  for (int s = 0; s < TSD_EO_COUNT; s++) ED_REQ(e[s] >= 0 && e[s] <= lim);
#undef ED_REQ
  return TSD_OK;
}
}  // namespace

extern "C" int tsd_debug_elem_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out, int64_t* ext,
                                  int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  TSD_TRY(check_fields("elem_run", n, TSD_ED_COUNT));
  replay::Box logical;
  TSD_TRY(ed_extents(desc, ext, &logical));
  const int64_t* d = desc;
  if (info) for (int i = 0; i < TSD_EI_COUNT; i++) info[i] = 0;
  if (!host_in) return TSD_OK;  // sizing only: no context or device needed
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("elem_run", ext, TSD_EO_COUNT, TSD_EO_Y, host_in, host_out));
  HIP_TRY(hipSetDevice(ctx->device));
  const int mode = (int)d[TSD_ED_MODE];
  GuardedOperands ops(ctx, TSD_EO_COUNT);
  for (int s = 0; s < TSD_EO_Y; s++)
    if (ext[s]) TSD_TRY(ops.add(s, ext[s], ed_elem_bytes(mode, s, d), host_in[s]));
  // quick-GELU overwrites its rows in place: Y starts as X
  TSD_TRY(ops.add(TSD_EO_Y, ext[TSD_EO_Y], ed_elem_bytes(mode, TSD_EO_Y, d), mode == TSD_EM_QUICK_GELU ? host_in[TSD_EO_X] : nullptr, host_out[0], logical));
  int bad0 = 0, bad1 = 0;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(&bad0, ctx->status, sizeof(int), hipMemcpyDeviceToHost));
  ctx->sl_last = SmallLinearPlan();
  const int B = (int)d[TSD_ED_B], K = (int)d[TSD_ED_K], C = (int)d[TSD_ED_C], H = (int)d[TSD_ED_H], W = (int)d[TSD_ED_W];
  const int64_t N = d[TSD_ED_N], rows = d[TSD_ED_ROWS];
  const int cols = (int)d[TSD_ED_COLS], ld = (int)d[TSD_ED_LD], inter = (int)d[TSD_ED_INTERLEAVE];
  const float scale = f32_of(d[TSD_ED_SCALE]);
  const void* x = ops.at(TSD_EO_X);
  const void* w = ops.at(TSD_EO_W);
  const void* bias = ops.at(TSD_EO_BIAS);
  void* y = ops.at(TSD_EO_Y);
  const int r = run_planned(ctx, [&]() -> int {
    switch (mode) {
      case TSD_EM_SMALL_LINEAR:
        return launch_small_linear(ctx, (const float*)x, B, K, (int)d[TSD_ED_LDX], (const half_t*)w, (int)d[TSD_ED_LDW], (const float*)bias, (int)N,
                                   (int)d[TSD_ED_SILU], (float*)y, (int)d[TSD_ED_LDY]);
      case TSD_EM_TIME_EMBEDDING: return launch_time_embedding(ctx, (const float*)x, f32_of(d[TSD_ED_T_BITS]), B, (float*)y);
      case TSD_EM_GEGLU_ERF: return launch_geglu_erf_f16(ctx, (const half_t*)x, rows, cols, (half_t*)y);
      case TSD_EM_QUICK_GELU: return launch_quick_gelu_f16(ctx, (half_t*)y, N);
      case TSD_EM_UNARY: return launch_unary_f32(ctx, (int)d[TSD_ED_OP], (const float*)x, N, (float*)y);
      case TSD_EM_CLIP_EMBED:
        return launch_clip_embed(ctx, (const int*)x, (const half_t*)w, (int)d[TSD_ED_V], (int)d[TSD_ED_D], (const float*)bias, B, (int)d[TSD_ED_T], (half_t*)y);
      case TSD_EM_CHW_TO_NHWC:
        return launch_chw_f32_to_nhwc_f16(ctx, (const float*)x, B, C, H, W, (int)d[TSD_ED_CUSE], scale, (half_t*)y, (int)d[TSD_ED_CDST]);
      case TSD_EM_IM2COL3X3: return launch_chw_f32_to_im2col3x3_f16(ctx, (const float*)x, B, C, H, W, (half_t*)y, scale);
      case TSD_EM_NHWC_TO_CHW:
        return d[TSD_ED_DTYPE] == 1 ? launch_nhwc_f16_to_chw_f32(ctx, (const half_t*)x, B, C, H, W, ld, (float*)y)
                                    : launch_nhwc_f32_to_chw_f32(ctx, (const float*)x, B, C, H, W, ld, (float*)y);
      case TSD_EM_F32_TO_F16_ROWS: return launch_f32_to_f16_rows(ctx, (const float*)x, rows, cols, (half_t*)y, ld, d[TSD_ED_ROWS_DST]);
      case TSD_EM_F16_TO_F32_ROWS: return launch_f16_to_f32_rows(ctx, (const half_t*)x, rows, cols, ld, (float*)y);
      case TSD_EM_TRANSPOSE_TO_F16:
        return launch_transpose_f32_to_f16(ctx, (const float*)x, B, K, (int)N, (half_t*)y, (int)d[TSD_ED_KPAD], (int)d[TSD_ED_NPAD]);
      case TSD_EM_PACK_CONV:
        return launch_pack_conv(ctx, (const float*)x, (int)d[TSD_ED_O], (int)d[TSD_ED_I], (int)d[TSD_ED_KSIZE], (half_t*)y, (int)d[TSD_ED_OPAD],
                                (int)d[TSD_ED_IPAD]);
      case TSD_EM_PACK_LINEAR: return launch_pack_linear(ctx, (const float*)x, (int)N, K, (half_t*)y, (int)d[TSD_ED_KPAD], inter);
      case TSD_EM_PACK_BIAS: return launch_pack_bias(ctx, (const float*)x, (int)N, (float*)y, (int)d[TSD_ED_NPAD], inter);
      case TSD_EM_PACK_IM2COL_W: return launch_pack_im2col_w(ctx, (const half_t*)x, (int)d[TSD_ED_O], (int)d[TSD_ED_IPAD], C, (half_t*)y);
      default: return launch_encoder_sample(ctx, (const float*)x, B, (int)d[TSD_ED_HW], ld, (const float*)w, (float*)y);
    }
  });
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  HIP_TRY(hipMemcpy(&bad1, ctx->status, sizeof(int), hipMemcpyDeviceToHost));
  if (bad1) {  // counted, not reported: the context stays usable
    const int zero = 0;
    HIP_TRY(hipMemcpy(ctx->status, &zero, sizeof(int), hipMemcpyHostToDevice));
  }
  info[TSD_EI_NONFINITE] = bad1 - bad0;
  info[TSD_EI_NB] = ctx->sl_last.nb; info[TSD_EI_PASSES] = ctx->sl_last.passes;
  TSD_TRY(ops.read_back(&info[TSD_EI_CHANGED]));
  return r;
}

// ---- IP-Adapter's decoupled cross attention on caller operands (tests/ipadapter_ref.py holds k_ip_attn_add to an fp64 reference) -------
namespace {
int pd_elem_bytes(int slot) { return slot == TSD_PO_S ? 4 : 2; }
// Element extent of every operand.  K is sized with all 16 token rows and V^T with 16 columns, whatever N is: rows / columns >= N exist in
// the product's buffers (they hold W . 0) and must not reach the result.
int pd_extents(const int64_t* d, int64_t* e) {
  for (int i = 0; i < TSD_PO_COUNT; i++) e[i] = 0;
#define PD_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "ip_attn_run: descriptor cannot be sized (%s)", #cond)
  PD_REQ(d[TSD_PD_VERSION] == TSD_PD_VERSION_1);
  const int64_t B = d[TSD_PD_B], H = d[TSD_PD_H], hd = d[TSD_PD_D], lim = 1LL << 28;
  const int64_t S = std::max<int64_t>(d[TSD_PD_S], 1);
  PD_REQ(B > 0 && B <= 16 && H > 0 && H <= 4096 && hd > 0 && hd <= 4096 && H * hd <= 65536);
  PD_REQ(d[TSD_PD_S] >= 0 && S <= (1 << 20) && d[TSD_PD_N] >= 0 && d[TSD_PD_N] <= 4096);
  const int64_t C = H * hd;
  for (int f : {TSD_PD_LDQ, TSD_PD_LDK, TSD_PD_LDO}) PD_REQ(d[f] >= C && d[f] <= (1 << 20));
  PD_REQ(d[TSD_PD_LDVT] >= IP_MAX_TOKENS && d[TSD_PD_LDVT] <= (1 << 20));
  PD_REQ(d[TSD_PD_SQB] >= S * d[TSD_PD_LDQ] && d[TSD_PD_SKB] >= IP_MAX_TOKENS * d[TSD_PD_LDK] && d[TSD_PD_SVTB] >= C * d[TSD_PD_LDVT] &&
         d[TSD_PD_SOB] >= S * d[TSD_PD_LDO]);
  for (int f : {TSD_PD_SQB, TSD_PD_SKB, TSD_PD_SVTB, TSD_PD_SOB}) PD_REQ(d[f] < lim);
  e[TSD_PO_Q] = (B - 1) * d[TSD_PD_SQB] + (S - 1) * d[TSD_PD_LDQ] + C;
  e[TSD_PO_K] = (B - 1) * d[TSD_PD_SKB] + (IP_MAX_TOKENS - 1) * d[TSD_PD_LDK] + C;
  e[TSD_PO_VT] = (B - 1) * d[TSD_PD_SVTB] + (C - 1) * d[TSD_PD_LDVT] + IP_MAX_TOKENS;
  e[TSD_PO_S] = B;
  e[TSD_PO_OIN] = e[TSD_PO_O] = (B - 1) * d[TSD_PD_SOB] + (S - 1) * d[TSD_PD_LDO] + C;
  for (int s = 0; s < TSD_PO_COUNT; s++) PD_REQ(e[s] >= 0 && e[s] <= lim);
#undef PD_REQ
  return TSD_OK;
}
}  // namespace

extern "C" int tsd_debug_ip_attn_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                     int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  TSD_TRY(check_fields("ip_attn_run", n, TSD_PD_COUNT));
  TSD_TRY(pd_extents(desc, ext));
  const int64_t* d = desc;
  if (info) for (int i = 0; i < TSD_PI_COUNT; i++) info[i] = 0;
  if (!host_in) return TSD_OK;  // sizing only: no context or device needed
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("ip_attn_run", ext, TSD_PO_COUNT, TSD_PO_O, host_in, host_out));
  HIP_TRY(hipSetDevice(ctx->device));
  GuardedOperands ops(ctx, TSD_PO_COUNT);
  for (int s = 0; s < TSD_PO_OIN; s++)
    if (ext[s]) TSD_TRY(ops.add(s, ext[s], pd_elem_bytes(s), host_in[s]));
  // O is updated in place: it starts as the OIN payload, which is no device operand of its own
  const replay::Box logical{d[TSD_PD_B], d[TSD_PD_SOB], d[TSD_PD_S], d[TSD_PD_LDO], d[TSD_PD_H] * d[TSD_PD_D]};
  TSD_TRY(ops.add(TSD_PO_O, ext[TSD_PO_O], 2, host_in[TSD_PO_OIN], host_out[0], logical));
  IpAttnArgs a;
  a.Q = (const half_t*)ops.at(TSD_PO_Q); a.ldq = (int)d[TSD_PD_LDQ]; a.sQ = d[TSD_PD_SQB];
  a.K = (const half_t*)ops.at(TSD_PO_K); a.ldk = (int)d[TSD_PD_LDK]; a.sK = d[TSD_PD_SKB];
  a.Vt = (const half_t*)ops.at(TSD_PO_VT); a.ldvt = (int)d[TSD_PD_LDVT]; a.sVt = d[TSD_PD_SVTB];
  a.O = (half_t*)ops.at(TSD_PO_O); a.ldo = (int)d[TSD_PD_LDO]; a.sO = d[TSD_PD_SOB];
  a.s = (const float*)ops.at(TSD_PO_S);
  a.B = (int)d[TSD_PD_B]; a.H = (int)d[TSD_PD_H]; a.d = (int)d[TSD_PD_D]; a.S = (int)d[TSD_PD_S]; a.N = (int)d[TSD_PD_N];
  a.scale = f32_of(d[TSD_PD_SCALE]);
  const int r = run_planned(ctx, [&]() -> int { return launch_ip_attn_add(ctx, a); });
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  TSD_TRY(ops.read_back(&info[TSD_PI_CHANGED]));
  return r;
}

// ---- the CLIP vision encoder's image front end on caller operands (tests/clipvision_ref.py holds k_clip_image_patches to an fp64 reference) ----
extern "C" int tsd_debug_image_patches_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                           int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  TSD_TRY(check_fields("image_patches_run", n, TSD_VD_COUNT));
  const int64_t* d = desc;
  for (int i = 0; i < TSD_VO_COUNT; i++) ext[i] = 0;
#define VD_REQ(cond) \
  if (!(cond)) TSD_FAIL(TSD_E_ARG, "image_patches_run: descriptor cannot be sized (%s)", #cond)
  VD_REQ(d[TSD_VD_VERSION] == TSD_VD_VERSION_1);
  VD_REQ(d[TSD_VD_B] > 0 && d[TSD_VD_B] <= 64 && d[TSD_VD_H] > 0 && d[TSD_VD_H] <= 4096 && d[TSD_VD_W] > 0 && d[TSD_VD_W] <= 4096);
  VD_REQ(d[TSD_VD_LD] >= CV_PATCH_K && d[TSD_VD_LD] <= 4096);
#undef VD_REQ
  ext[TSD_VO_IMG] = d[TSD_VD_B] * 3 * d[TSD_VD_H] * d[TSD_VD_W];
  ext[TSD_VO_OUT] = d[TSD_VD_B] * CV_PATCHES * d[TSD_VD_LD];
  if (info) for (int i = 0; i < TSD_VI_COUNT; i++) info[i] = 0;
  if (!host_in) return TSD_OK;  // sizing only: no context or device needed
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  TSD_TRY(check_slots("image_patches_run", ext, TSD_VO_COUNT, TSD_VO_OUT, host_in, host_out));
  HIP_TRY(hipSetDevice(ctx->device));
  const int B = (int)d[TSD_VD_B], H = (int)d[TSD_VD_H], W = (int)d[TSD_VD_W], ld = (int)d[TSD_VD_LD];
  VisionTab t;
  TSD_TRY(vision_tab(ctx, H, W, &t));  // the sides the launcher refuses are refused here, before anything is allocated
  info[TSD_VI_TAPS_H] = t.tx; info[TSD_VI_TAPS_V] = t.ty; info[TSD_VI_ROWS] = t.rows; info[TSD_VI_LDS] = (int64_t)3 * t.rows * CV_PATCH * 4;
  GuardedOperands ops(ctx, TSD_VO_COUNT);
  TSD_TRY(ops.add(TSD_VO_IMG, ext[TSD_VO_IMG], 4, host_in[TSD_VO_IMG]));
  // every element of the extent is written (the pad columns as zeros): the whole extent is logical
  TSD_TRY(ops.add(TSD_VO_OUT, ext[TSD_VO_OUT], 2, nullptr, host_out[0], replay::Box::dense(ext[TSD_VO_OUT])));
  const int r = run_planned(ctx, [&]() -> int { return launch_clip_image_patches(ctx, (const float*)ops.at(TSD_VO_IMG), B, H, W, (half_t*)ops.at(TSD_VO_OUT), ld); });
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  TSD_TRY(ops.read_back(&info[TSD_VI_CHANGED]));
  return r;
}
