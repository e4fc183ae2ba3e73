// common.h - internal types shared by the host graph code and the HIP kernels of libtsd.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/tsd.h"
#include "counter_rng.h"

typedef _Float16 half_t;

// ---- error plumbing -------------------------------------------------------------------
void tsd_set_error(const char* fmt, ...);
#define TSD_FAIL(code, ...)      \
  do {                           \
    tsd_set_error(__VA_ARGS__);  \
    return (code);               \
  } while (0)
#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess) TSD_FAIL(TSD_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
  } while (0)
#define TSD_TRY(expr)            \
  do {                           \
    int r__ = (expr);            \
    if (r__ != TSD_OK) return r__; \
  } while (0)

// ---- device resources --------------------------------------------------------------------
// Every device allocation, event and stream of the library is made and released through these (runtime.cpp): each calls HIP and then
// records the outcome in the process-wide ledger (device_ledger.h) that tsd_debug_device_ledger reports.  They change nothing about the
// call: arguments, result and error are HIP's.  No file of the library calls the runtime's own functions for these.
hipError_t dev_malloc(void** p, size_t bytes);
hipError_t dev_free(void* p);
hipError_t dev_event_create(hipEvent_t* e);
hipError_t dev_event_destroy(hipEvent_t e);
hipError_t dev_stream_create(hipStream_t* s, unsigned flags);
hipError_t dev_stream_destroy(hipStream_t s);
// the create / destroy entry of a handle type: one more, one fewer
enum DevHandle : int { DEV_CTX = 0, DEV_MODEL = 1, DEV_SESSION = 2 };
void dev_handle_count(DevHandle kind, int delta);

// ---- workspace arena: stack allocator over one big device allocation ------------------
// All kernels of a context run on one stream, so releasing to a mark and re-using the bytes is
// ordered by the stream.  `planning` mode only tracks the high-water mark (no launches).
struct Arena {
  char* base = nullptr;
  size_t cap = 0, top = 0, peak = 0;
  bool planning = false;
  size_t mark() const { return top; }
  void release(size_t m) { top = m; }
  void* alloc(size_t bytes) {
    size_t a = (top + 255) & ~size_t(255);
    size_t n = a + bytes;
    if (n > peak) peak = n;
    if (!planning && n > cap) return nullptr;
    top = n;
    return planning ? (void*)(uintptr_t)(0x1000 + a) : (void*)(base + a);
  }
};

// Every tuning / A-B switch of the library.  Read from the environment ONCE, by tsd_ctx_create, into the context that the launches
// run on: no dispatch code calls getenv and no switch is process-global, so two contexts (one per GPU, one host thread each - SURVEY.md
// section 8b "Threading") can run different settings side by side.  The tsd_debug_set_* entry points change ONE context and bump its
// `gen`; a denoise session remembers the generation it sized its workspace for (session.cpp).  Defaults = the measured optimum.
struct TsdOptions {
  // graph shape (graph.cpp)
  int qkv_fuse = 1;        // TSD_QKV_FUSE: q | k | V^T (and the context K | V^T of all blocks) from ONE GEMM with a transposed tail
  int res_fuse_skip = 1;   // TSD_RES_FUSE_SKIP: residual block's 1x1 skip convolution as extra K of its second 3x3 convolution
  int gn_composite = 1;    // TSD_GN_COMPOSITE: GroupNorm over a channel concat from the two producers' partial statistics
  int conv_in_im2col = 1;  // TSD_CONV_IN_IM2COL: the 4-channel input convolution as one im2col K tile
  int chain = 1;           // TSD_CHAIN: fused head / tail kernels of the 64x64-level attention blocks
  int fold_out = 1;        // TSD_FOLD_OUT: op-by-op attention blocks (C = 640 / 1280): GEGLU's second linear + the output 1x1 conv as one GEMM over [h | r]
  int ups_fold = 1;        // TSD_UPS_FOLD: conv1 of the residual blocks behind a nearest-2x upsample as four 2x2 parity convolutions on folded weights (ConvW::w_uf): K = 4 Cin instead of 9 Cin
  int fold_dup = 1;        // TSD_FOLD_DUP: layer 10's concat(x, x) folded into its conv1 / skip weights (UNetW::res_dup): a 1280 -> 1280 block instead of 2560 -> 1280
  int control_stats = 1;   // TSD_CONTROL_STATS: the ControlNet injection re-emits the GroupNorm statistics of the tensors it rewrites (0: it discards them and every consumer runs its own statistics pass)
  int session_hoist = 1;   // TSD_SESSION_HOIST: a denoise session computes the time path of every schedule entry and the context K / V^T once per upload(), not once per step
  // derived weight copies (model.cpp; read when a model's derived buffers are built)
  int conv_w_tm_mib = 2, lin_w_tm = 1, lin_w_tm_kib = 1024;  // TSD_CONV_W_TM, TSD_LIN_W_TM, TSD_LIN_W_TM_KIB
  // flash attention (kernels_attn.hip)
  int attn_qb = 2;         // TSD_ATTN_QB: d = 40, 32-query blocks per wave where the key loop is long
  int attn_qb_force = 0;   // tsd_debug_set_attn_qb: 0 = by shape, 1 / 2 = always (4-wave workgroups), 3 = always the 8-wave kernel
  int attn_wg8 = 1;        // TSD_ATTN_WG8: d = 40 long key loops on the 8-wave two-group kernel (kernels_attn8.hip)
  int attn8_var = 0;       // TSD_ATTN8_VAR: timing / A-B variant of that kernel (builds with -DTSD_ATTN8_VARIANTS only)
  int attn_diag = 1;       // tsd_debug_set_attn_diag: second optimistic reference (the query's own key block)
  int attn_xcd = 0;        // TSD_ATTN_XCD: XCD-aware (head, query tile) map
  // GEMM / conv dispatch (gemm_plan.cpp)
  int xcdn = 0, conv_halo = 0, splitk = 1, splitk_mink = 4096, splitk_tiles = 256, splitk_small = 8, splitk_wide = 1, splitk_ring4 = 0,
      splitk_big = 0, sk_cfg = 5, thin_cfg = 0, tune = 15, sk256 = 0, skip128 = 1;  // sk256: TSD_GEMM_SK256 (256-row tiles for split-K launches)
  int force_cfg = -1;      // tsd_debug_gemm_bench / _check: tile configuration forced for the launches of this context
  int sk_big_graph = 0;    // slices of the long-K split launches asked for by the graph being enqueued (gemm_set_splitk_big)
  char cfg_override[512] = "";  // TSD_GEMM_CFG_OVERRIDE
  int gn_apply_mult = 2;   // TSD_GN_APPLY_MULT
  int gn_finalize_min = 2048;  // TSD_GN_FINALIZE_MIN: slab x group partial pairs per sample from which a separate k_gn_finalize launch finishes the statistics
  int debug_occ = 0;       // TSD_DEBUG_OCC
  int debug_poison_what = 31;  // TSD_DEBUG_POISON_WHAT: 1 arena, 2 derived weights, 4 session state, 8 the buffers a session grows (session_grow), 16 staging
  int debug_poison = -1;   // TSD_DEBUG_POISON=<byte>: fresh device allocations (arena, session state and buffers, derived weights, staging) are filled with it - a result that changes with the byte reads memory nobody wrote
  int bench_wrot = 1, bench_epi = 0, bench_altcfg = -1, gemm_ts = 0;  // microbenchmark only (tsd_debug_gemm_bench)
  unsigned gen = 0;        // bumped by every tsd_debug_set_* call on this context
};
void options_from_env(TsdOptions& o);

// Host-side plan of one GroupNorm launch (kernels_norm.hip gn_plan): where the statistics come from and how the passes are cut.
// launch_groupnorm / launch_gn_stats act on it and leave it in tsd_ctx::gn_last; tsd_debug_norm_run reports it.
struct GnComposite;
struct GnPlan {
  int PL = 0;             // pixel lanes per 256-thread block
  int slab_pixels = 0;    // pixels per slab of the own statistics pass
  int apply_pixels = 0;   // pixels per apply block
  int nslab = 0;          // slabs per sample the statistics are finished from (own slabs, the producer's, or 64 prereduced chunks)
  bool composite = false;   // the GnComposite was accepted
  bool have_stats = false;  // producer partials are used: no own pass over the tensor
  bool prereduce = false;   // k_gn_prereduce runs first
  int stats_ready = 0;      // a separate k_gn_finalize launch finishes the statistics
  const float* part = nullptr; int part_nslab = 0;  // the producer table (composite: its first table)
};
GnPlan gn_plan(const TsdOptions& opt, int HW, int C, int groups, const float* pre_part, int pre_nslab, const GnComposite* comp);

// Host-side plan of one attention-core launch (kernels_attn.hip attn_plan): the kernel launch_flash_attention picks and the switches it
// passes to it.  launch_flash_attention acts on it and leaves it in tsd_ctx::attn_last; tsd_debug_attn_run reports it.  `softmax` is
// set by the launch_softmax_rows_* launchers instead (1 k_softmax_rows<float>, 2 k_softmax_rows<half_t>, 3 / 4 k_softmax_rows_h8<1> / <2>).
struct AttnPlan {
  int kernel = 0;   // tsd_attn_kernel: 1 flash_attn_kernel<40,1>, 2 <40,2>, 3 flash_attn8_kernel<40>, 4 <80,1>, 5 <160,1>; 0 = none ran
  int diag = 0, xcd_map = 0;
  int softmax = 0;
};
AttnPlan attn_plan(const TsdOptions& opt, int B, int H, int d, int Sq, int Sk);
// What launch_small_linear launched (kernels_elementwise.hip), left in tsd_ctx::sl_last; tsd_debug_elem_run reports it.
struct SmallLinearPlan {
  int nb = 0;      // the k_small_linear<NB> instance: 1, 2, 4, 8 or 16; 0 = none ran
  int passes = 0;  // K passes of 128 * SL_KIT columns
};

// Host-side plan of one GEMM / conv3x3 launch (gemm_plan.cpp): the tile configuration (a row of gemm_tiles.h) that runs, in how many
// split-K slices, as which conv variant - what fixes the fp32 summation tree of the launch.  launch_gemm acts on it and leaves it in
// tsd_ctx::gemm_last; the graph asks it for the statistics geometry; tsd_debug_gemm_run / _plan report it.  It does not depend on the epilogue.
struct GemmArgs;
struct GemmPlan {
  const char* refused = nullptr;  // why this launch cannot run (TSD_E_ARG; cfg holds the offending id) - nothing else is filled in then
  int cfg = -1;          // the tile configuration that runs: the dispatcher's choice after its halo-x / skip128 adjustments, or opt.force_cfg
  int ways = 1;          // split-K slices (1: none)
  int variant = 0;       // gemm_kernel's CV: 0 plain, 1 halo-x, 2 fused 1x1 skip source, 3 upsample fold
  int BM = 0, BN = 0;    // tile
  int BMw = 0, BNw = 0;  // one wave's sub-tile
  int K = 0;             // the K the launch executes (4 * Cin under the upsample fold)
  int lds_bytes = 0;
  int64_t ws_floats = 0; // split-K workspace
  bool gn_stats = false; // the tile's epilogue can emit GroupNorm statistics
  int M = 0, N = 0, batch = 0;
  // EPI_GNSTATS geometry: slabs per sample this launch emits for `groups` groups over its N channels, or 0 when its tile cannot
  int gn_slabs(int rows_per_sample, int groups) const;
};
GemmPlan gemm_plan(const TsdOptions& opt, const GemmArgs& a);

// Coefficient tables of the CLIP image front end for one input size (kernels_vision.hip vision_tab builds and caches them): per axis the
// 224 cropped outputs' first source index, tap count and fp32 weights (pitch tx / ty).  One device allocation: int xs[224], xn[224], ys[224],
// yn[224], float wx[224][tx], wy[224][ty].
struct VisionTab {
  int H = 0, W = 0;
  int tx = 0, ty = 0;   // longest coefficient row of the horizontal / vertical table
  int rows = 0;         // most source rows the 14 output rows of one patch read
  void* dev = nullptr;
};

// cos / sin tables of FreeU's four-bin filter for one plane size (kernels_freeu.hip freeu_tab builds and caches them): one device
// allocation, float cy[H], sy[H], cx[W], sx[W].
struct FreeuTab {
  int H = 0, W = 0;
  float* dev = nullptr;
};

struct tsd_ctx {
  int device = 0;
  TsdOptions opt;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  Arena arena;
  int* sk_flags = nullptr;  // 4096 zeroed ints, allocated on first use: one split-K arrival flag per (slice, tile) holding the
                            // epoch of the launch that published it and, at [4095], a sticky count of hand-offs that timed out
  unsigned sk_epoch = 0;    // split-K launches so far on this context (the flag value of the next launch; never 0)
  int* status = nullptr;    // 16 zeroed ints: [0] non-finite values written to caller-visible tensors since the last report (kernels_elementwise.hip), [2] flash-attention workgroups that repeated exactly
  half_t* zeros = nullptr;  // 4 KiB: [0,2048) zeros (padded im2col taps / head dims); [2048,2176) fp16 ones
  void* staging = nullptr;  // device staging for host<->device copies
  size_t staging_cap = 0;
  void* rccl_comm = nullptr;
  void* rccl_lib = nullptr;
  int nranks = 1, rank = 0;
  bool launch() const { return !arena.planning; }
  // built-in per-kernel-class timer (hipEvents on THIS stream; bench.py's roofline leg)
  bool profile = false;
  std::vector<hipEvent_t> prof_ev;  // pairs (start, stop): created by ProfScope as a pass needs them, kept for the next pass, destroyed with the context
  std::vector<int> prof_cls;
  std::vector<int> prof_kern;   // kernel dispatches per record
  std::vector<int> prof_shape;  // 4 ints per record (M, N, K, batch) - 0 when not a GEMM
  size_t prof_n = 0;
  // tsd_debug_gemm_record: TSD_GD_COUNT descriptor fields per GEMM launch enqueued while on
  bool gemm_rec_on = false;
  std::vector<int64_t> gemm_rec;
  GemmPlan gemm_last;         // plan of the last GEMM / conv3x3 launch enqueued (tsd_debug_gemm_run)
  GnPlan gn_last;             // plan of the last GroupNorm launch enqueued (tsd_debug_norm_run)
  int64_t gn_paths[8] = {};   // tsd_debug_gn_path_counts
  AttnPlan attn_last;         // plan of the last attention-core / row-softmax launch enqueued (tsd_debug_attn_run)
  SmallLinearPlan sl_last;    // the last tiny-M linear launch enqueued (tsd_debug_elem_run)
  std::vector<VisionTab> vision_tabs;  // resize coefficient tables of the CLIP image front end, one per input size (kernels_vision.hip)
  std::vector<FreeuTab> freeu_tabs;    // cos / sin tables of FreeU's skip filter, one per plane size (kernels_freeu.hip)
};

enum KernelClass : int {
  KC_GEMM = 0, KC_CONV = 1, KC_ATTN = 2, KC_GROUPNORM = 3, KC_LAYERNORM = 4, KC_SMALL_LINEAR = 5,
  KC_ELEMENTWISE = 6, KC_SOFTMAX = 7, KC_CHAIN = 8, KC_COUNT = 9
};
// RAII: records a start/stop event pair around the launches in its scope when profiling is on
struct ProfScope {
  tsd_ctx* c; bool on;
  int kernels = 1;  // kernel dispatches inside the scope (a GroupNorm scope brackets up to three): what profile_end counts as launches
  ProfScope(tsd_ctx* ctx, int cls, int M = 0, int N = 0, int K = 0, int batch = 0)
      : c(ctx), on(ctx->profile && ctx->launch()) {
    if (!on) return;
    if (c->prof_n * 2 + 2 > c->prof_ev.size()) {
      hipEvent_t a, b;
      if (dev_event_create(&a) != hipSuccess) { on = false; return; }
      if (dev_event_create(&b) != hipSuccess) { (void)dev_event_destroy(a); on = false; return; }
      c->prof_ev.push_back(a); c->prof_ev.push_back(b);
    }
    if (c->prof_cls.size() <= c->prof_n) { c->prof_cls.push_back(cls); c->prof_shape.resize(4 * c->prof_cls.size()); }
    else c->prof_cls[c->prof_n] = cls;
    int* sh = &c->prof_shape[4 * c->prof_n];
    sh[0] = M; sh[1] = N; sh[2] = K; sh[3] = batch;
    (void)hipEventRecord(c->prof_ev[c->prof_n * 2], c->stream);
  }
  ~ProfScope() {
    if (!on) return;
    (void)hipEventRecord(c->prof_ev[c->prof_n * 2 + 1], c->stream);
    if (c->prof_kern.size() <= c->prof_n) c->prof_kern.resize(c->prof_n + 1);
    c->prof_kern[c->prof_n] = kernels;
    c->prof_n++;
  }
};

int ctx_reserve_arena(tsd_ctx* ctx, size_t bytes);
// call after a stream synchronize: TSD_E_STATE if any split-K hand-off of this context ever timed out (results since then
// cannot be trusted)
int ctx_check_splitk(tsd_ctx* ctx);
// ... and TSD_E_NONFINITE if inf / NaN reached a caller-visible tensor since the last report (count cleared once reported).  Every
// synchronisation point of the ABI calls this one; it includes ctx_check_splitk.
int ctx_check_status(tsd_ctx* ctx);
// Body of the tsd_debug_set_* switches: the option takes `v` if lo <= v <= hi; the option generation (which invalidates the workspace
// plan of uploaded sessions) moves only when the stored value really CHANGES - restoring the value that is already there in a
// try / finally does not cost every session of the context an upload().  Returns the previous value (>= 0); TSD_E_ARG (< 0) for a
// NULL context is the only negative return.
inline int ctx_set_option(tsd_ctx* ctx, int TsdOptions::*field, int v, int lo, int hi) {
  if (!ctx) return TSD_E_ARG;
  const int prev = ctx->opt.*field;
  if (v >= lo && v <= hi && v != prev) { ctx->opt.*field = v; ctx->opt.gen++; }
  return prev;
}

int ctx_reserve_staging(tsd_ctx* ctx, size_t bytes);
// destroys the communicator of the context, if it holds one (api_model.cpp: tsd_dist_finalize and tsd_ctx_destroy)
void dist_release(tsd_ctx* ctx);

// ---- device tensor views (NHWC fp16 activations) ---------------------------------------
struct Act {  // [B][H][W][C] with row pitch ld (elements) between pixels
  half_t* p = nullptr;
  int B = 0, H = 0, W = 0, C = 0, ld = 0;
  // GroupNorm statistics emitted by the producing GEMM/conv epilogue (EPI_GNSTATS): gn_buf/gn_groups are set by whoever
  // allocates the tensor (capacity B * (H*W/32) * gn_groups * 2 floats); gn_part/gn_nslab by the producer if it could.
  float* gn_buf = nullptr; int gn_groups = 0;
  const float* gn_part = nullptr; int gn_nslab = 0;
  int64_t pixels() const { return (int64_t)B * H * W; }
};

template <class T>
static inline T* arena_alloc(tsd_ctx* ctx, int64_t n) {
  return (T*)ctx->arena.alloc((size_t)n * sizeof(T));
}
static inline Act act_alloc(tsd_ctx* ctx, int B, int H, int W, int C) {
  Act a;
  a.B = B; a.H = H; a.W = W; a.C = C; a.ld = C;
  a.p = arena_alloc<half_t>(ctx, (int64_t)B * H * W * C);
  return a;
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline int round_up(int a, int b) { return ceil_div(a, b) * b; }

// ---- packed weights ------------------------------------------------------------------
struct ConvW {  // fp16 [Opad][k*k][Ipad] (K-major for the implicit GEMM), fp32 bias [Opad]
  const half_t* w = nullptr;
  const float* b = nullptr;
  int I = 0, O = 0, k = 0, Ipad = 0, Opad = 0;
  // derived (model_check_ready, weight-heavy 3x3 convs only): the same weights K-tile-major, [k*k*Ipad / 64][Opad][64] - the 160 x 64
  // tile a workgroup stages per K step is 20 KB of consecutive bytes instead of 160 rows a whole weight row (up to 46 KB) apart
  const half_t* w_tm = nullptr;
  // derived (model_check_ready, conv1 of the residual blocks the graph runs behind a nearest-2x upsample): the upsample folded into the
  // weights - four parity copies [q = 2 py + px][4 * Ipad / 64][Opad][64] of the 2x2 kernels, K-tile-major, contiguous (GemmArgs::Wuf)
  const half_t* w_uf = nullptr;
};
struct LinW {  // fp16 [N][Kpad], fp32 bias [N] (nullptr when the reference passes use_bias=False)
  const half_t* w = nullptr;
  const float* b = nullptr;
  int N = 0, K = 0, Kpad = 0;
  const half_t* w_tm = nullptr;  // derived K-tile-major copy [Kpad / 64][N][64] (see ConvW::w_tm)
};

// ---- GEMM / implicit-GEMM conv launcher (kernels_gemm.hip) ------------------------------
enum : int {
  EPI_BIAS_N = 1,    // + bias[n]
  EPI_BIAS_M = 2,    // + bias[m]            (swapped-operand GEMMs, e.g. V^T projection)
  EPI_ROWVEC = 4,    // + rowvec[(m / rows_per_batch) * rowvec_ld + n]   (time-embedding add)
  EPI_RESIDUAL = 8,  // + R[m][n]
  EPI_RES_UPS = 16,  // residual is read through a nearest-2x upsample of a (Ho/2, Wo/2) tensor
  EPI_GEGLU = 32,    // out[m][n/2] = a * gelu_tanh(g) for interleaved (a,g) column pairs
  EPI_OUT_F32 = 64,  // store fp32 instead of fp16
  EPI_GNSTATS = 128, // also emit per-(sample, row slab, group) sum / sum of squares of the rounded output: the statistics
                     // pass of the GroupNorm that consumes this tensor (gn_* fields)
};

struct GemmArgs {
  // "A" operand: rows m.  Dense mode: A0[m][k] for k < K0, A1[m][k-K0] for k >= K0 (concat).
  const half_t* A0 = nullptr; int lda0 = 0; int K0 = 0;
  const half_t* A1 = nullptr; int lda1 = 0;
  // conv3x3 mode (conv != 0): A0 is NHWC [B][Hs][Ws][lda0]; output pixel m = (b*Ho+oy)*Wo+ox reads
  // tap (kh,kw) at (oy*stride-pad+kh, ox*stride-pad+kw) of the (optionally 2x-upsampled) source.
  int conv = 0, Hs = 0, Ws = 0, Ho = 0, Wo = 0, Cin = 0, stride = 1, pad = 1, ups = 0;
  // conv3x3 + fused 1x1 convolution of a second tensor at the same resolution (residual block skip path): K = 9*Cin + Cin1 + Cin2,
  // A1 [.][lda1] gives channels 0..Cin1, A2 [.][lda2] channels Cin1..Cin1+Cin2 (channel concat), weights Wt1[N][ldw1]
  const half_t* A2 = nullptr; int lda2 = 0; int Cin1 = 0, Cin2 = 0;
  const half_t* Wt1 = nullptr; int ldw1 = 0;
  const half_t* Wt = nullptr; int ldw = 0;  // "W" operand [N][K]
  // conv3x3, ups == 2 (upsample fold): the launch is DESCRIBED by Wt / ldw / w_kts / K = 9 * Cin of the original 3x3 weights, like ups == 1,
  // and EXECUTES K = 4 * Cin on Wuf - the four parity copies of the folded 2x2 weights, each K-tile-major [4 * Cin / 64][N][64], contiguous
  // (model.cpp ups_fold_host; gemm_ups_fold_ok is the eligibility rule, launch_gemm refuses everything else and writes nothing)
  const half_t* Wuf = nullptr;
  int w_kts = 0;  // bytes from one 64-deep K tile of W to the next; 0 = 128 (row-major [N][K]).  K-tile-major [K/64][N][64]: ldw = 64, w_kts = N * 128
  int M = 0, N = 0, K = 0;
  int batch = 1; int64_t sA = 0, sW = 0, sC = 0, sR = 0;  // element strides per batch
  int epi = 0;
  const float* bias = nullptr;
  const float* rowvec = nullptr; int rowvec_ld = 0; int rows_per_batch = 1;
  const half_t* R = nullptr; int ldr = 0;
  void* C = nullptr; int ldc = 0;
  float out_scale = 1.f;  // applied to the accumulator before bias/residual
  // Transposed tail (dense GEMMs): output columns n >= vt_n0 are stored channel-major instead - Vt[(m / vt_S) * vt_sB + (n - vt_n0) * vt_ld
  // + m % vt_S] (fp16) - so a fused q/k/v projection leaves q | k token-major in C and V^T [B][C][S] for the attention kernel in
  // ONE launch (helpers/attention.mojo:29-31).  vt_n0 must be a multiple of the tile width, vt_S (rows per sample) of 8.
  half_t* Vt = nullptr; int vt_n0 = 0, vt_ld = 0, vt_S = 0; int64_t vt_sB = 0;
  // EPI_GNSTATS: partial[(b * gn_nslab + slab) * gn_groups + g][2], slab = wave-tile row block within the sample
  float* gn_part = nullptr; int gn_groups = 0, gn_rows_per_sample = 0, gn_nslab = 0;
  // rows of one sample (H*W) when the caller knows it: lets few-row, long-K layers run split-K independently of the batch
  int rows_per_sample_hint = 0;
};
int launch_gemm(tsd_ctx* ctx, const GemmArgs& a);
bool gemm_ups_fold_ok(const TsdOptions& opt, const GemmArgs& a);  // may this conv3x3 over a 2x-upsampled source run with ups = 2? (gemm_plan.cpp)
// host fold of 3x3 weights [O][3][3][Ipad] (row pitch ldw >= 9 * Ipad, fp16 bits) into [4][O][2][2][Ipad]; returns the non-finite sums (model.cpp)
int64_t ups_fold_host(const uint16_t* w, int O, int Ipad, int ldw, uint16_t* out);
// ... and the same in the device layout GemmArgs::Wuf reads: per parity K-tile-major [4 * Ipad / 64][O][64], contiguous (Ipad % 64 == 0)
int64_t ups_fold_pack_host(const uint16_t* w, int O, int Ipad, int ldw, uint16_t* out_tm);
// the launch as a tsd_debug_gemm_* descriptor (TSD_GD_COUNT fields; api_replay.cpp)
void gemm_describe(const tsd_ctx* ctx, const GemmArgs& a, int64_t* desc);
// slices of the long-K split launches (K >= 8192, 16x16 level) for the graph being enqueued on this context; returns the previous value
int gemm_set_splitk_big(tsd_ctx* ctx, int ways);

// ---- other kernel launchers -----------------------------------------------------------
// layout / elementwise (kernels_elementwise.hip)
int launch_chw_f32_to_nhwc_f16(tsd_ctx* ctx, const float* src, int B, int C, int H, int W, int Cuse, float scale,
                               half_t* dst, int Cdst);
// [B][C][H][W] fp32 (C <= 7) -> im2col rows [B*H*W][64] fp16 of a 3x3 / stride 1 / pad 1 convolution: column t*C + c = tap t, channel c
// (zero outside the image and beyond 9*C); launch_pack_im2col_w builds the matching [O][64] weight matrix from packed conv weights
int launch_chw_f32_to_im2col3x3_f16(tsd_ctx* ctx, const float* src, int B, int C, int H, int W, half_t* dst, float scale = 1.f);
int launch_pack_im2col_w(tsd_ctx* ctx, const half_t* w, int O, int Ipad, int C, half_t* dst);
int launch_pack_tile_major(tsd_ctx* ctx, const half_t* w, int N, int K, half_t* dst);  // [N][K] -> [K/64][N][64]
// fold of a linear layer into the 1x1 convolution that follows it: wf[n][0..K2) = sum_j wo[n][j] * w2[j][k], wf[n][K2..K2+C) = wo[n][..],
// bf[n] = sum_j wo[n][j] * b2[j] + bo[n]  (fp32 sums in index order, one rounding to fp16 per folded weight)
int launch_fold_linear_conv1x1(tsd_ctx* ctx, const half_t* wo, int ldo, const float* bo, const half_t* w2, int ld2, const float* b2, int C, int K2,
                               half_t* wf, int ldf, float* bf);
int launch_nhwc_f16_to_chw_f32(tsd_ctx* ctx, const half_t* src, int B, int C, int H, int W, int ld, float* dst);
int launch_nhwc_f32_to_chw_f32(tsd_ctx* ctx, const float* src, int B, int C, int H, int W, int ld, float* dst);
int launch_f32_to_f16_rows(tsd_ctx* ctx, const float* src, int64_t rows, int cols, half_t* dst, int ld_dst,
                           int64_t rows_dst);  // zero-pads cols..ld_dst and rows..rows_dst
int launch_f16_to_f32_rows(tsd_ctx* ctx, const half_t* src, int64_t rows, int cols, int ld_src, float* dst);
int launch_unary_f32(tsd_ctx* ctx, int op, const float* x, int64_t n, float* y);  // 0 silu 1 gelu 2 rescale
int launch_pad_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int t, int b, int l, int r, float* y);
int launch_upsample_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, float* y);
int launch_softmax_rows_f32(tsd_ctx* ctx, const float* x, int64_t rows, int cols, float* y);
int launch_softmax_rows_f16(tsd_ctx* ctx, half_t* x, int64_t rows, int cols, int ld);  // in place
int launch_softmax_rows_f16_causal(tsd_ctx* ctx, half_t* x, int64_t rows, int cols, int ld, int period, int zero_to);
int launch_clip_embed(tsd_ctx* ctx, const int* tokens, const half_t* table, int n_vocab, int D, const float* pos, int B,
                      int T, half_t* y);
int launch_quick_gelu_f16(tsd_ctx* ctx, half_t* x, int64_t n);
int launch_gelu_erf_f16(tsd_ctx* ctx, half_t* x, int64_t n);  // torch's exact GELU in place (the SD-2.x text encoder's MLP)
int launch_time_embedding(tsd_ctx* ctx, const float* t_dev, float t_scalar, int B, float* out);  // out [B][320]; t_dev NULL -> scalar
int launch_small_linear(tsd_ctx* ctx, const float* x, int B, int K, int ldx, const half_t* w, int ldw, const float* bias,
                        int N, int silu_in, float* y, int ldy);
int launch_add_const_f32(tsd_ctx* ctx, float* dst, int64_t n, float c);
// -DTSD_JITTER builds: n launches of the two-wave hazard kernel, launch i stores the word it saw to out[i]; TSD_E_ARG in any other build
int launch_jitter_selftest(tsd_ctx* ctx, unsigned* out, int n);
// out[m][j] = x[m][2j] * gelu_erf(x[m][2j+1]) : GEGLU with torch's exact GELU on the interleaved (a, gate) pairs of an
// un-fused geglu1 output (extension for real checkpoints; the reference's tanh form is fused into the GEMM epilogue)
int launch_geglu_erf_f16(tsd_ctx* ctx, const half_t* x, int64_t rows, int n_out, half_t* out);
int launch_fill_uniform(tsd_ctx* ctx, float* dst, int64_t n, uint64_t seed, uint64_t tensor_id, float bound);
// weight packing: src fp32 reference layout -> packed fp16
int launch_pack_conv(tsd_ctx* ctx, const float* src, int O, int I, int k, half_t* dst, int Opad, int Ipad);
int launch_pack_linear(tsd_ctx* ctx, const float* src, int N, int K, half_t* dst, int Kpad, int geglu_interleave);
int launch_pack_bias(tsd_ctx* ctx, const float* src, int N, float* dst, int Npad, int geglu_interleave);
int launch_transpose_f32_to_f16(tsd_ctx* ctx, const float* src, int batch, int K, int N, half_t* dst, int Kpad,
                                int Npad);
// low-rank merge into ONE packed weight, in place (kernels_lora.hip): W[o][c] = rn16(W[o][c] + scale * sum_j up[o - row0][j] down[j][c]) for the
// reference rows [row0, row0 + rows) of a packed linear [N][ld] (k = 0; `interleave`: GEGLU rows) or convolution [Opad][k*k][ld] (k = 1, 3);
// up [rows][rank] / down [rank][I * max(k*k, 1)] device fp32, columns in the reference order; pad rows / channels are never written
int launch_lora_merge(tsd_ctx* ctx, half_t* W, int N, int I, int k, int ld, int interleave, int row0, int rows, const float* up,
                      const float* down, int rank, float scale);
// host inverse of launch_pack_linear / launch_pack_conv on fp16 bit patterns (model.cpp): packed -> fp32 in the reference layout
void unpack_weight_host(const uint16_t* packed, int N, int I, int k, int ld, int interleave, float* out);
int launch_ddpm_step(tsd_ctx* ctx, float* latents, const float* eps, const float* eps_uncond, float cfg_scale,
                     const float* noise, int64_t n, float inv_sqrt_a, float sqrt_b, float c_x0, float c_xt,
                     float sigma, int eps_hw = 0);  // eps_hw > 0: eps in the output convolution's layout [B][eps_hw][4]
// the same update with the noise drawn in the kernel: element j of sample b (chw elements each, n <= 16 chw) takes
// normal_counter(bases.base[b], j) where launch_ddpm_step reads noise[b * chw + j]; the noise is always added
int launch_ddpm_step_seeded(tsd_ctx* ctx, float* latents, const float* eps, const float* eps_uncond, float cfg_scale,
                            const NormalBases& bases, int64_t chw, int64_t n, float inv_sqrt_a, float sqrt_b, float c_x0, float c_xt,
                            float sigma, int eps_hw = 0);
int launch_add_noise(tsd_ctx* ctx, float* latents, const float* noise, int64_t n, float sa, float sb);

// ---- linear-multistep sampler update (kernels_sampler.hip) and its host schedule (sampler.cpp) ------------------------------
// e = (eps - eps_u) * cfg_scale + eps_u ; x0 = (x - sigma_t e) / alpha_t ; x_out = c_x x + c_e e + c_h hist_in + c_n noise ; hist_out = x0
struct SamplerCoeffs {
  float alpha_t, sigma_t, c_x, c_e, c_h, c_n;
};
// eps_uncond / hist_in / noise / hist_out may be nullptr (the term or the store is skipped); x_out may be x and hist_out may be
// hist_in (every element is read and written by one thread); eps_hw as in launch_ddpm_step
int launch_sampler_step(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                        const float* hist_in, const float* noise, int64_t n, const SamplerCoeffs& c, int eps_hw, float* x_out,
                        float* hist_out);
// the same update with c_n z drawn in the kernel (launch_ddpm_step_seeded's rule); no noise pointer
int launch_sampler_step_seeded(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                               const float* hist_in, const NormalBases& bases, int64_t chw, int64_t n, const SamplerCoeffs& c,
                               int eps_hw, float* x_out, float* hist_out);
// The two updates for a model output that means v = alpha e - sigma x0 (kernels_vpred.hip): the same x_out arithmetic with v in place of e
// (c.c_e multiplies v) and hist_out = alpha_t x - sigma_t v, which divides by nothing.  Arguments as above.
int launch_sampler_step_v(tsd_ctx* ctx, const float* x, const float* v, const float* v_uncond, float cfg_scale, const float* hist_in,
                          const float* noise, int64_t n, const SamplerCoeffs& c, int eps_hw, float* x_out, float* hist_out);
int launch_sampler_step_v_seeded(tsd_ctx* ctx, const float* x, const float* v, const float* v_uncond, float cfg_scale,
                                 const float* hist_in, const NormalBases& bases, int64_t chw, int64_t n, const SamplerCoeffs& c,
                                 int eps_hw, float* x_out, float* hist_out);
// dst[b * per_sample + j] = normal_counter(bases.base[b], first + j) for the n = (samples) * per_sample elements of dst, n <= 16 per_sample
// (kernels_sampler.hip k_fill_normal): N(0,1) of the counter RNG, the values the seeded updates draw inline
int launch_fill_normal(tsd_ctx* ctx, float* dst, int64_t n, int64_t per_sample, const NormalBases& bases, uint64_t first);
// masked denoising (kernels_sampler.hip): x_out = m x + (1 - m)(a_prev known + s_prev noise); x / known / noise / x_out CHW [B][4][hw],
// mask [B][hw]; noise may be nullptr (that term is skipped); x_out may be x
int launch_inpaint_blend(tsd_ctx* ctx, const float* x, const float* mask, const float* known, const float* noise, int B, int64_t hw,
                         float a_prev, float s_prev, float* x_out);
// pixel mask [B][8L][8L] -> latent mask [B][L][L] by 8x8 blocks; mode is a tsd_mask_mode
int launch_latent_mask(tsd_ctx* ctx, const float* mask_px, int B, int LH, int LW, int mode, float* mask_lat);
// ---- slot sessions (kernels_slots.hip): every sample of the batch at its own schedule index ------------------------------------
// One by-value table serves the whole batch: entry b holds what launch_ddpm_step_seeded / launch_sampler_step(_seeded) would be given for
// sample b alone.  c[]: SLOT_DDPM { sqrt(abar), sqrt(1 - abar), c_x0, c_xt, sigma } (ddpm_coeffs), SLOT_LMS the SamplerCoeffs in field order.
// The noise bases sit beside the entries as the NormalBases the element functions index by sample.  40 * 16 + 128 = 768 bytes of kernel
// arguments, read-only, entry b through scalar loads (b is the block's y index).
enum { SLOT_SKIP = 0, SLOT_DDPM = 1, SLOT_LMS = 2 };               // SlotEntry::mode; SKIP: the sample is not read, written or counted
enum { SLOT_HIST_IN = 1, SLOT_HIST_OUT = 2, SLOT_NOISE = 4 };      // SlotEntry::flags
struct SlotEntry {
  int mode, flags;
  float cfg_scale;
  float c[6];
  int pad_;
};
struct SlotTable {
  SlotEntry e[16];
  NormalBases bases;  // stream 16 + i_b of the slot's seed (read under SLOT_NOISE only)
};
// x [B][4][hw] CHW in place, hist [B][4][hw] in place (read under SLOT_HIST_IN, written under SLOT_HIST_OUT), eps / eps_uncond as in
// launch_ddpm_step (eps_hw > 0: [B][eps_hw][4]); chw = 4 * hw elements per sample
int launch_slot_update(tsd_ctx* ctx, float* x, const float* eps, const float* eps_uncond, float* hist, const SlotTable& tab, int B,
                       int64_t chw, int eps_hw);
// The same update with the masked-denoising blend of launch_inpaint_blend applied before the store, per slot: entry b of a second by-value
// table holds the blend's scalars for sample b (a_prev, s_prev of the timestep ITS update reaches) and whether it blends at all.
// 16 * 16 = 256 bytes beside the 768 of SlotTable: 1104 bytes of explicit arguments with the pointers and scalars, a kernel argument
// segment of 1360 bytes with the hidden ones (limit 4 KiB).
// mask [B][hw], known / noise [B][4][hw] are read for `on` entries only; an entry that is off stores what launch_slot_update stores.
struct SlotBlend {
  int on;
  float a_prev, s_prev;
  int pad_;
};
struct SlotBlendTable {
  SlotBlend e[16];
};
int launch_slot_update_blend(tsd_ctx* ctx, float* x, const float* eps, const float* eps_uncond, float* hist, const SlotTable& tab,
                             const SlotBlendTable& blend, const float* mask, const float* known, const float* noise, int B, int64_t chw,
                             int eps_hw);
// The two slot updates of a v-prediction session (kernels_vpred.hip): every entry is SLOT_SKIP or SLOT_LMS (TSD_E_ARG for SLOT_DDPM: a v
// session never plans it), applied by the v element function.  The prediction type belongs to the launch: all slots share the model.
int launch_slot_update_v(tsd_ctx* ctx, float* x, const float* v, const float* v_uncond, float* hist, const SlotTable& tab, int B,
                         int64_t chw, int eps_hw);
int launch_slot_update_blend_v(tsd_ctx* ctx, float* x, const float* v, const float* v_uncond, float* hist, const SlotTable& tab,
                               const SlotBlendTable& blend, const float* mask, const float* known, const float* noise, int B,
                               int64_t chw, int eps_hw);
// rows of the hoisted time table for samples at different schedule indices: out[b][0..N) = ttab[row[b]][0..N), b < Bu <= 16
struct SlotRows {
  int row[16];
};
int launch_slot_time_rows(tsd_ctx* ctx, const float* ttab, int N, const SlotRows& rows, int Bu, float* out);
// the same without the table: tdev[b] = t[b], the per-sample timesteps launch_time_embedding reads
struct SlotTimes {
  float t[16];
};
int launch_slot_timesteps(tsd_ctx* ctx, const SlotTimes& t, int Bu, float* tdev);

// ---- guidance rescale (kernels_guidance.hip states the formula): a pre-pass over eps / eps_uncond between the forward and the update ----
// Entry b of the by-value table: on = 0 leaves sample b unread and unwritten (phi = 0, an idle or finished slot).  256 bytes of arguments.
struct CfgRescaleEntry {
  int on;
  float cfg_scale, phi;
  int pad_;
};
struct CfgRescaleTable {
  CfgRescaleEntry e[16];
};
enum { CFG_RESCALE_GMAX = 64, CFG_RESCALE_PARTIAL_DOUBLES = 16 * CFG_RESCALE_GMAX * 4 };  // partial [B <= 16][G <= 64][4] fp64: 32 KiB
int cfg_rescale_blocks(int64_t chw);  // G: partials (and blocks) per sample, a function of chw alone
// eps / eps_uncond [B][chw] in place (either eps layout: a sample's chw floats are contiguous in both); partial: CFG_RESCALE_PARTIAL_DOUBLES
// doubles of scratch; g_out [B] or nullptr, written for `on` entries only.  Two launches, no copy, no synchronisation.
int launch_cfg_rescale(tsd_ctx* ctx, float* eps, float* eps_uncond, const CfgRescaleTable& tab, int B, int64_t chw, double* partial,
                       float* g_out);

// ---- ControlNet injection (kernels_control.hip states the formula): x <- rn16(x + s_b r) in place on up to 16 NHWC fp16 tensors in ONE
// launch, and the GroupNorm partials of the rounded result into each tensor's own table.  56 bytes per entry: 904 bytes of arguments.
enum { CONTROL_MAX_ENTRIES = 16, CONTROL_RESIDUALS = 13 };  // a ControlNet gives 12 skip residuals and one for the bottleneck output
struct ControlEntry {
  half_t* x;        // [B][HW][ldx], written in place
  const half_t* r;  // [B][HW][ldr]
  float* part;      // [B][nslab][groups][2] (sum, sum of squares) per slab, or nullptr: no statistics for this tensor
  int ldx, ldr, HW, C;
  int groups, nslab;  // what the tensor's producer used; without statistics nslab only cuts the work (groups is ignored)
  int blk0;           // first block of the entry: the prefix sum of nslab (launch_control_inject fills it)
  int pad_;
};
struct ControlTable {
  ControlEntry e[CONTROL_MAX_ENTRIES];
  int n;
  int skip_zero;  // 1: a sample whose scale is exactly 0 is neither read nor written - its tensor and its producer's statistics stand
};
// scale: device fp32 [B]
int launch_control_inject(tsd_ctx* ctx, ControlTable tab, int B, const float* scale);

// ---- FreeU (kernels_freeu.hip states the formulas): in place on the two inputs of a decoder concat, h [B][H*W][ldh] (channels < Ch / 2
// scaled by b, or by (b - 1) n[p] + 1 in the modulated mode) and r [B][H*W][ldr] (its four lowest spatial frequencies scaled by s).  b == 1
// leaves h unread and unwritten, s == 1 leaves r so (either pointer may then be nullptr).  mean: [B][H*W] floats of scratch, read and
// written under TSD_FREEU_MODULATED with b != 1 only.  ONE launch, one more in front of it in the modulated mode; Ch a multiple of 16, Cr
// of 8, pitches multiples of 8, both tensors 16-byte aligned, H, W >= 2.
struct FreeuOp {
  half_t* h = nullptr; half_t* r = nullptr;
  float* mean = nullptr;
  int B = 0, H = 0, W = 0, Ch = 0, Cr = 0, ldh = 0, ldr = 0;
  float b = 1.f, s = 1.f;
  int mode = 0;  // TSD_FREEU_CONSTANT / TSD_FREEU_MODULATED
};
int launch_freeu(tsd_ctx* ctx, const FreeuOp& op);
int freeu_tab(tsd_ctx* ctx, int H, int W, const float** dev_out);

// alphas_cumprod of the scaled-linear beta schedule (sampler.mojo:28-32), fp32 like the reference's Tensor
void sampler_alphas_cumprod(int n_train, std::vector<float>& out);
// the same table (zero_terminal_snr = 0, bitwise) or its zero-terminal-SNR rescale (1; Lin et al. 2023, algorithm 1 on sqrt(abar), in
// double, one rounding to float per entry; the last entry is exactly 0).  TSD_E_ARG for another flag value, and for n_train < 2 under 1.
int sampler_alphas_cumprod(int n_train, int zero_terminal_snr, std::vector<float>& out);
// timestep list of `spacing` (tsd_timestep_spacing) with the first `start_step` entries dropped; TSD_E_ARG on a bad argument
int sampler_timesteps(int spacing, int n_train, int n_infer, int start_step, std::vector<int>& out);
// scalars of step i of `timesteps` as double: out[8] = { t, t_prev (-1: the clean sample), alpha_t, sigma_t, c_x, c_e, c_h, c_n }
int sampler_coeffs(int kind, double eta, const std::vector<float>& alphas_cumprod, const std::vector<int>& timesteps, int i,
                   int have_history, double out[8]);
// The plan of step i: what its update launch is given, whoever launches it (session.cpp: the lockstep step and every slot of an advance).
// Fills e->mode (SLOT_DDPM / SLOT_LMS), e->c[] in the order documented at SlotEntry and e->flags: SLOT_NOISE the update adds noise,
// SLOT_HIST_IN it reads the previous step's x0 (hist_valid: the caller holds it for step i), SLOT_HIST_OUT it keeps its own.
// cfg_scale is the caller's.  DDPM's previous timestep is t - n_train / n_infer under LEADING spacing, the next list entry under TRAILING.
// prediction (tsd_prediction_type) says what the model output means.  Under TSD_PRED_V every sampler, DDPM included, is a SLOT_LMS entry
// whose c[3] multiplies v, for the v kernels (launch_sampler_step_v ..): never SLOT_DDPM, and SLOT_NOISE wherever c_n != 0.
int sampler_step_plan(int kind, double eta, int spacing, int n_train, int n_infer, const std::vector<float>& alphas_cumprod,
                      const std::vector<int>& timesteps, int i, bool hist_valid, int prediction, SlotEntry* e);
// TSD_E_ARG for an unknown prediction type, and for epsilon-prediction on a list with a timestep of alpha_bar = 0 (x0 does not exist)
int sampler_prediction_ok(int prediction, const std::vector<float>& alphas_cumprod, const std::vector<int>& timesteps);
// sampler_coeffs for either prediction type (checked by sampler_prediction_ok); under TSD_PRED_V out[5] multiplies v and no row
// divides by alpha_t: finite at alpha_bar_t = 0
int sampler_coeffs_ex(int kind, double eta, const std::vector<float>& alphas_cumprod, const std::vector<int>& timesteps, int i,
                      int have_history, int prediction, double out[8]);

// ---- non-finite accounting (kernels_elementwise.hip explains where it is reported) -------------------------------------------
__device__ __forceinline__ bool nonfinite_f(float v) { return !(fabsf(v) <= 3.4028234e38f); }  // inf or NaN
__device__ __forceinline__ void nonfinite_report(int* counter, int nbad) {
  if (nbad) atomicAdd(counter, nbad);  // rare path
}
int launch_encoder_sample(tsd_ctx* ctx, const float* moments_nhwc, int B, int HW, int ld, const float* noise_chw,
                          float* latents_chw);

// norms (kernels_norm.hip).  Dual source: channels [0,C0) from x0, [C0,C) from x1 (concat).
struct NormSrc {
  const half_t* x0 = nullptr; int ld0 = 0; int C0 = 0;
  const half_t* x1 = nullptr; int ld1 = 0;
};
// Extension for real (PyTorch-trained) checkpoints, not reference behaviour: per-channel weight / bias and
// 1/sqrt(var + eps) instead of the reference's 1/(sigma + eps).  nullptr = reference semantics.
struct NormAffine {
  const float* w = nullptr;  // [C] (nullptr: ones)
  const float* b = nullptr;  // [C] (nullptr: zeros)
  int torch_rstd = 1;        // 1: rsqrt(var + eps) ; 0: 1 / (sqrt(var) + eps)
};
// Statistics of a GroupNorm as sums of producer-emitted partials of a FINER grouping: norm group g = fine groups
// [g*comb, (g+1)*comb) of the concatenation (part0: G0 fine groups, part1: G1) - both [B][nslab][G*][2], one slab per 32 rows.
struct GnComposite {
  const float* part0 = nullptr; int G0 = 0;
  const float* part1 = nullptr; int G1 = 0;
  int nslab = 0, comb = 1;
};
int launch_groupnorm(tsd_ctx* ctx, const NormSrc& src, int B, int HW, int C, int groups, float eps, float gamma,
                     int silu, half_t* y, int ldy, const float* pre_part = nullptr, int pre_nslab = 0,
                     const NormAffine* aff = nullptr, const GnComposite* comp = nullptr);
int launch_layernorm(tsd_ctx* ctx, const half_t* x, int64_t rows, int C, int ldx, float eps, half_t* y, int ldy,
                     const NormAffine* aff = nullptr);

// attention (kernels_attn.hip): fused flash attention for d_head in {40, 64, 80, 160}.
struct AttnArgs {
  const half_t* Q = nullptr; int ldq = 0; int64_t sQ = 0;    // Q[b][s][h*d + j]
  const half_t* K = nullptr; int ldk = 0; int64_t sK = 0;    // K[b][t][h*d + j]
  const half_t* Vt = nullptr; int ldvt = 0; int64_t sVt = 0; // Vt[b][h*d + j][t]  (t contiguous)
  half_t* O = nullptr; int ldo = 0; int64_t sO = 0;          // O[b][s][h*d + j]
  int B = 0, H = 0, d = 0, Sq = 0, Sk = 0;
  float scale = 1.f;
};
bool attn_fused_supported(int d);

// IP-Adapter's decoupled cross attention (kernels_ipattn.hip states the formula): O <- rn16(O + s_b * Attn(Q, K_ip, V_ip)) in place over
// N <= 16 image tokens, one launch.  K: [b][j][h*d + c] token-major, at least N rows; Vt: [b][h*d + c][j], ldvt >= 16 (keys j >= N of
// either operand never reach the result); s: device fp32 [B], a sample whose scale is exactly 0 is neither read nor written.
enum { IP_MAX_TOKENS = 16 };
struct IpAttnArgs {
  const half_t* Q = nullptr; int ldq = 0; int64_t sQ = 0;
  const half_t* K = nullptr; int ldk = 0; int64_t sK = 0;
  const half_t* Vt = nullptr; int ldvt = 0; int64_t sVt = 0;
  half_t* O = nullptr; int ldo = 0; int64_t sO = 0;
  const float* s = nullptr;
  int B = 0, H = 0, d = 0, S = 0, N = 0;
  float scale = 1.f;
};
int launch_ip_attn_add(tsd_ctx* ctx, const IpAttnArgs& a);

// fused row-local tail of `Unet_Attention_Block.forward` (kernels_chain.hip): self-attention out_proj + residual, LayerNorm,
// cross-attention over the projected context, LayerNorm, GEGLU feed-forward, 1x1 conv_out + long residual in ONE kernel.
struct AttnTailArgs {
  const half_t* ao = nullptr; int ld_ao = 0;    // self-attention output [M][C]
  const half_t* tok = nullptr; int ld_tok = 0;  // first residual (conv_in output)
  const half_t* x = nullptr; int ld_x = 0;      // block input (long residual)
  half_t* out = nullptr; int ld_out = 0;
  const half_t* wstream = nullptr;  // launch_attn_tail_pack() image of sa_out, ca_q, ca_out, geglu1, geglu2, conv_out
  const float *bso = nullptr, *bco = nullptr, *b1 = nullptr, *b2 = nullptr, *bout = nullptr;
  const half_t* Kc = nullptr; int ldk = 0; int64_t sK = 0;
  const half_t* Vt = nullptr; int ldvt = 0; int64_t sVt = 0;
  int C = 0, d = 0, heads = 0, T = 0, S = 0; int64_t M = 0;
  float scale = 1.f, eps = 1e-5f;
  float* gn_part = nullptr; int gn_nslab = 0;  // GroupNorm(32) statistics of the output, one slab per 32 rows
};
bool attn_tail_supported(const tsd_ctx* ctx, int C, int d, int heads, int T, int64_t M, int S);
int launch_attn_tail(tsd_ctx* ctx, const AttnTailArgs& a);
size_t attn_tail_stream_bytes();
// fused head of the same block (kernels_chain.hip): GroupNorm-apply, 1x1 conv_in (-> tok), LayerNorm, q / k projections and
// the V^T projection in ONE kernel.  gn_stats = finished (mean, 1/(sigma+eps)) pairs of the block input, [B][32][2].
struct AttnHeadArgs {
  const half_t* x = nullptr; int ld_x = 0;
  const float* gn_stats = nullptr;
  const half_t* wstream = nullptr;  // launch_attn_head_pack() image of conv_in and in_proj
  const float* b_in = nullptr;      // conv_in bias
  half_t* tok = nullptr; int ld_tok = 0;
  half_t* qk = nullptr; int ld_qk = 0;              // [M][2C]: q | k
  half_t* vt = nullptr; int ld_vt = 0; int64_t s_vt = 0;  // [B][C][ld_vt]
  int64_t M = 0; int S = 0; float eps = 1e-5f;
};
size_t attn_head_stream_bytes();
int launch_attn_head_pack(tsd_ctx* ctx, const half_t* Wc, int ld_c, const half_t* Win, int ld_in, half_t* dst);
int launch_attn_head(tsd_ctx* ctx, const AttnHeadArgs& a);
// finish GroupNorm statistics from producer-emitted partials [B][nslab][groups][2] -> stats [B][groups][2] (mean, gamma/(sigma+eps))
int launch_gn_stats(tsd_ctx* ctx, const half_t* x, int ld, int B, int HW, int C, int groups, float eps, float gamma, float* stats);
int launch_gn_finalize(tsd_ctx* ctx, const float* partial, int nslab, int B, int HW, int C, int groups, float eps, float gamma,
                       float* stats);
int launch_attn_tail_pack(tsd_ctx* ctx, const half_t* Wso, int ld_so, const half_t* Wq, int ld_q, const half_t* Wco, int ld_co,
                          const half_t* W1, int ld_1, const half_t* W2, int ld_2, const half_t* Wout, int ld_out, half_t* dst);
int launch_flash_attention(tsd_ctx* ctx, const AttnArgs& a);

// ---- CLIP vision front end (kernels_vision.hip states the formula): images fp32 [B][3][H][W] on 0 .. 255 -> resized (PIL's antialiased
// bicubic, shortest edge 224), centre-cropped, normalised patch rows fp16 [B * 256][ld], column c * 196 + kh * 14 + kw, columns 588 .. ld - 1
// zero.  8 <= H, W <= 2048 (TSD_E_SHAPE), ld >= 592 and a multiple of 8.  The coefficient tables are built on the host and kept on the context.
enum { CV_SIDE = 224, CV_PATCH = 14, CV_GRID = 16, CV_PATCHES = 256, CV_PATCH_K = 588, CV_PATCH_LD = 592 };
int vision_tab(tsd_ctx* ctx, int H, int W, VisionTab* out);
int launch_clip_image_patches(tsd_ctx* ctx, const float* img, int B, int H, int W, half_t* out, int ld);
// x[b * sx + n] = rn16(cls[n] + f32(pos[n])), n < C, b < B: the class rows of the token tensor (the patch rows come from the patch GEMM's
// residual epilogue)
int launch_vision_class_rows(tsd_ctx* ctx, const float* cls, const half_t* pos, int B, int C, half_t* x, int64_t sx);
