// runtime.cpp - context, error string, workspace arena, staging.  No CPU fallback anywhere: if HIP
// reports no device every compute entry point fails with TSD_E_HIP.
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "device_ledger.h"

static thread_local char g_err[512] = "";

// ---- the ledger of device resources and the only calls of the runtime that make or release one ---------------------------------------
static ledger::DeviceLedger& the_ledger() {
  static ledger::DeviceLedger l;
  return l;
}
hipError_t dev_malloc(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) the_ledger().alloc(*p, bytes);
  return e;
}
hipError_t dev_free(void* p) {
  const hipError_t e = hipFree(p);
  the_ledger().free(p, e == hipSuccess);
  return e;
}
hipError_t dev_event_create(hipEvent_t* ev) {
  const hipError_t e = hipEventCreate(ev);
  if (e == hipSuccess) the_ledger().event_create(*ev);
  return e;
}
hipError_t dev_event_destroy(hipEvent_t ev) {
  const hipError_t e = hipEventDestroy(ev);
  the_ledger().event_destroy(ev, e == hipSuccess);
  return e;
}
hipError_t dev_stream_create(hipStream_t* s, unsigned flags) {
  const hipError_t e = hipStreamCreateWithFlags(s, flags);
  if (e == hipSuccess) the_ledger().stream_create(*s);
  return e;
}
hipError_t dev_stream_destroy(hipStream_t s) {
  const hipError_t e = hipStreamDestroy(s);
  the_ledger().stream_destroy(s, e == hipSuccess);
  return e;
}
void dev_handle_count(DevHandle kind, int delta) { the_ledger().handle((ledger::Handle)kind, delta); }

static_assert((int)ledger::ALLOCS_LIVE == TSD_DL_ALLOCS_LIVE && (int)ledger::BYTES_LIVE == TSD_DL_BYTES_LIVE &&
              (int)ledger::EVENTS_LIVE == TSD_DL_EVENTS_LIVE && (int)ledger::STREAMS_LIVE == TSD_DL_STREAMS_LIVE &&
              (int)ledger::CTX_LIVE == TSD_DL_CTX_LIVE && (int)ledger::MODELS_LIVE == TSD_DL_MODELS_LIVE &&
              (int)ledger::SESSIONS_LIVE == TSD_DL_SESSIONS_LIVE && (int)ledger::ALLOCS_TOTAL == TSD_DL_ALLOCS_TOTAL &&
              (int)ledger::FREES_TOTAL == TSD_DL_FREES_TOTAL && (int)ledger::FREES_UNKNOWN == TSD_DL_FREES_UNKNOWN &&
              (int)ledger::RELEASE_ERRORS == TSD_DL_RELEASE_ERRORS && (int)ledger::COUNT == TSD_DL_COUNT,
              "tsd_device_ledger_field (include/tsd.h) and ledger::Field (device_ledger.h) name the same fields in the same order");
static_assert((int)ledger::CTX == DEV_CTX && (int)ledger::MODEL == DEV_MODEL && (int)ledger::SESSION == DEV_SESSION, "DevHandle == ledger::Handle");
// The first min(n, TSD_DL_COUNT) fields of the ledger; returns TSD_DL_COUNT.  Needs no device and no context.
extern "C" int tsd_debug_device_ledger(int64_t* out, int n) {
  if (!out || n < 0) TSD_FAIL(TSD_E_ARG, "tsd_debug_device_ledger: out is NULL or n < 0");
  return the_ledger().snapshot(out, n);
}

void tsd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// the ONLY place the library reads its tuning switches from the environment (one pass per context, at tsd_ctx_create)
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e && *e ? atoi(e) : dflt; }
void options_from_env(TsdOptions& o) {
  o.qkv_fuse = env_int("TSD_QKV_FUSE", o.qkv_fuse);
  o.res_fuse_skip = env_int("TSD_RES_FUSE_SKIP", o.res_fuse_skip);
  o.gn_composite = env_int("TSD_GN_COMPOSITE", o.gn_composite);
  o.conv_in_im2col = env_int("TSD_CONV_IN_IM2COL", o.conv_in_im2col);
  o.chain = env_int("TSD_CHAIN", o.chain) ? 1 : 0;
  o.fold_out = env_int("TSD_FOLD_OUT", o.fold_out) ? 1 : 0;
  o.ups_fold = env_int("TSD_UPS_FOLD", o.ups_fold) ? 1 : 0;
  o.fold_dup = env_int("TSD_FOLD_DUP", o.fold_dup) ? 1 : 0;
  o.session_hoist = env_int("TSD_SESSION_HOIST", o.session_hoist) ? 1 : 0;
  o.control_stats = env_int("TSD_CONTROL_STATS", o.control_stats) ? 1 : 0;
  o.conv_w_tm_mib = env_int("TSD_CONV_W_TM", o.conv_w_tm_mib);
  o.lin_w_tm = env_int("TSD_LIN_W_TM", o.lin_w_tm);
  o.lin_w_tm_kib = env_int("TSD_LIN_W_TM_KIB", o.lin_w_tm_kib);
  { const int q = env_int("TSD_ATTN_QB", o.attn_qb); if (q == 1 || q == 2) o.attn_qb = q; }
  o.attn_xcd = env_int("TSD_ATTN_XCD", o.attn_xcd);
  o.attn_wg8 = env_int("TSD_ATTN_WG8", o.attn_wg8) ? 1 : 0;
  o.attn8_var = env_int("TSD_ATTN8_VAR", o.attn8_var);
  o.xcdn = env_int("TSD_GEMM_XCDN", o.xcdn);
  o.conv_halo = env_int("TSD_CONV_HALO", o.conv_halo);
  o.splitk = env_int("TSD_GEMM_SPLITK", o.splitk);
  o.splitk_mink = env_int("TSD_GEMM_SPLITK_MINK", o.splitk_mink);
  o.splitk_tiles = env_int("TSD_GEMM_SPLITK_TILES", o.splitk_tiles);
  o.splitk_small = env_int("TSD_GEMM_SPLITK_SMALL", o.splitk_small);
  o.splitk_wide = env_int("TSD_GEMM_SPLITK_WIDE", o.splitk_wide);
  o.splitk_ring4 = env_int("TSD_GEMM_SPLITK_RING4", o.splitk_ring4);
  o.splitk_big = env_int("TSD_GEMM_SPLITK_BIG", o.splitk_big);
  o.sk_cfg = env_int("TSD_GEMM_SK_CFG", o.sk_cfg);
  o.sk256 = env_int("TSD_GEMM_SK256", o.sk256);
  o.thin_cfg = env_int("TSD_GEMM_THIN_CFG", o.thin_cfg);
  o.skip128 = env_int("TSD_GEMM_SKIP128", o.skip128);
  o.tune = env_int("TSD_GEMM_TUNE", o.tune);
  if (const char* ov = getenv("TSD_GEMM_CFG_OVERRIDE")) { strncpy(o.cfg_override, ov, sizeof(o.cfg_override) - 1); o.cfg_override[sizeof(o.cfg_override) - 1] = 0; }
  o.gn_apply_mult = env_int("TSD_GN_APPLY_MULT", o.gn_apply_mult);
  o.gn_finalize_min = env_int("TSD_GN_FINALIZE_MIN", o.gn_finalize_min);
  o.debug_occ = getenv("TSD_DEBUG_OCC") ? 1 : 0;
  o.debug_poison = env_int("TSD_DEBUG_POISON", o.debug_poison);
  o.debug_poison_what = env_int("TSD_DEBUG_POISON_WHAT", o.debug_poison_what);
  o.bench_wrot = env_int("TSD_BENCH_WROT", o.bench_wrot); if (o.bench_wrot < 1) o.bench_wrot = 1;
  o.bench_epi = env_int("TSD_BENCH_EPI", o.bench_epi);
  o.bench_altcfg = env_int("TSD_BENCH_ALTCFG", o.bench_altcfg);
  o.gemm_ts = getenv("TSD_GEMM_TS") ? 1 : 0;
}

extern "C" int tsd_version(void) { return TSD_VERSION; }
extern "C" const char* tsd_last_error(void) { return g_err; }

extern "C" int tsd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// what tsd_ctx_create makes on the device, each into its field as soon as it exists ...
static int ctx_init(tsd_ctx* c) {
  HIP_TRY(dev_stream_create(&c->stream, hipStreamNonBlocking));
  HIP_TRY(dev_event_create(&c->ev0));
  HIP_TRY(dev_event_create(&c->ev1));
  HIP_TRY(dev_malloc((void**)&c->status, 16 * sizeof(int)));
  HIP_TRY(hipMemsetAsync(c->status, 0, 16 * sizeof(int), c->stream));
  HIP_TRY(dev_malloc((void**)&c->zeros, 4096));
  HIP_TRY(hipMemsetAsync(c->zeros, 0, 4096, c->stream));
  HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)(c->zeros + 1024), 0x3C00, 64, c->stream));  // 64 halves of 1.0 (attention row sums)
  HIP_TRY(hipStreamSynchronize(c->stream));
  return TSD_OK;
}
// ... and everything a context owns on the device, released: whatever exists of a context that failed half-way, or all of a live one
// whose stream is idle.  The object itself goes too.
static void ctx_release(tsd_ctx* c) {
  if (c->arena.base) (void)dev_free(c->arena.base);
  if (c->staging) (void)dev_free(c->staging);
  if (c->zeros) (void)dev_free(c->zeros);
  if (c->status) (void)dev_free(c->status);
  if (c->sk_flags) (void)dev_free(c->sk_flags);
  for (VisionTab& t : c->vision_tabs) if (t.dev) (void)dev_free(t.dev);
  for (FreeuTab& t : c->freeu_tabs) if (t.dev) (void)dev_free(t.dev);
  for (hipEvent_t e : c->prof_ev) (void)dev_event_destroy(e);
  if (c->ev0) (void)dev_event_destroy(c->ev0);
  if (c->ev1) (void)dev_event_destroy(c->ev1);
  if (c->stream) (void)dev_stream_destroy(c->stream);
  delete c;
}

extern "C" int tsd_ctx_create(int device, tsd_ctx** out) {
  if (!out) TSD_FAIL(TSD_E_ARG, "tsd_ctx_create: out is NULL");
  *out = nullptr;
  // kernel arguments in device memory (see tsd/_lib.py): effective when this is the process's first HIP call; hosts that
  // initialise HIP earlier export HIP_FORCE_DEV_KERNARG=1 themselves
  setenv("HIP_FORCE_DEV_KERNARG", "1", 0);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
    TSD_FAIL(TSD_E_HIP, "tsd_ctx_create: no HIP device visible (libtsd has no CPU fallback)");
  if (device < 0 || device >= n) TSD_FAIL(TSD_E_ARG, "tsd_ctx_create: device %d out of range [0,%d)", device, n);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    TSD_FAIL(TSD_E_HIP, "tsd_ctx_create: device %d is %s; libtsd is built for gfx950 only", device, prop.gcnArchName);
  tsd_ctx* c = new tsd_ctx();
  c->device = device;
  options_from_env(c->opt);
  const int r = ctx_init(c);
  if (r != TSD_OK) { ctx_release(c); return r; }  // the one way out of a context that did not come to be: nothing of it stays
  dev_handle_count(DEV_CTX, +1);
  *out = c;
  return TSD_OK;
}

extern "C" int tsd_ctx_destroy(tsd_ctx* c) {
  if (!c) return TSD_OK;
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  dist_release(c);  // a communicator the caller did not finalize
  ctx_release(c);
  dev_handle_count(DEV_CTX, -1);
  return TSD_OK;
}

int ctx_check_splitk(tsd_ctx* c) {
  if (!c->sk_flags) return TSD_OK;
  int n = 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(&n, c->sk_flags + 4095, sizeof(int), hipMemcpyDeviceToHost));
  if (n != 0) {
    // reported once, then cleared: the caller re-runs what it computed since the last clean synchronisation point
    const int zero = 0;
    (void)hipMemcpy(c->sk_flags + 4095, &zero, sizeof(int), hipMemcpyHostToDevice);
    TSD_FAIL(TSD_E_STATE, "%d split-K hand-off(s) timed out on this context (GPU shared or preempted?): results computed "
             "since the last clean synchronisation are invalid; re-run them", n);
  }
  return TSD_OK;
}

// call after a stream synchronize
int ctx_check_status(tsd_ctx* c) {
  TSD_TRY(ctx_check_splitk(c));
  if (!c->status) return TSD_OK;
  int n = 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(&n, c->status, sizeof(int), hipMemcpyDeviceToHost));
  if (n != 0) {
    const int zero = 0;  // reported once, then cleared
    (void)hipMemcpy(c->status, &zero, sizeof(int), hipMemcpyHostToDevice);
    TSD_FAIL(TSD_E_NONFINITE, "%d non-finite value(s) (inf / NaN) reached a tensor that leaves the device since the last clean "
             "synchronisation: an fp16 activation overflowed (|x| > 65504) or an input was not finite; the outputs are not "
             "the reference's (BASELINE.md section 4: supported dynamic range)", n);
  }
  return TSD_OK;
}
// Non-finite values written to caller-visible tensors on this context since the last report / reset (synchronises the stream).
extern "C" int tsd_debug_nonfinite_count(tsd_ctx* c, int reset) {
  if (!c || !c->status) return -1;
  if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return -1;
  int n = 0;
  if (hipMemcpy(&n, c->status, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (reset) { const int zero = 0; if (hipMemcpy(c->status, &zero, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) return -1; }
  return n;
}

// Overwrite the per-call scratch of the context with `byte`: the whole arena and the whole staging buffer, as they are now, on the
// context's stream.  Nothing else - not sk_flags (a hand-off in flight keeps its flags), not status, not zeros, no table, model or session.
extern "C" int tsd_debug_scribble(tsd_ctx* c, int byte) {
  if (!c) TSD_FAIL(TSD_E_ARG, "tsd_debug_scribble: ctx is NULL");
  if (byte < 0 || byte > 255) TSD_FAIL(TSD_E_ARG, "tsd_debug_scribble: byte %d is outside 0..255", byte);
  HIP_TRY(hipSetDevice(c->device));
  if (c->arena.base && c->arena.cap) HIP_TRY(hipMemsetAsync(c->arena.base, byte, c->arena.cap, c->stream));
  if (c->staging && c->staging_cap) HIP_TRY(hipMemsetAsync(c->staging, byte, c->staging_cap, c->stream));
  return TSD_OK;
}

extern "C" int tsd_ctx_synchronize(tsd_ctx* c) {
  if (!c) TSD_FAIL(TSD_E_ARG, "tsd_ctx_synchronize: ctx is NULL");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return ctx_check_status(c);
}

extern "C" int tsd_ctx_timer_start(tsd_ctx* c) {
  if (!c) TSD_FAIL(TSD_E_ARG, "ctx is NULL");
  HIP_TRY(hipEventRecord(c->ev0, c->stream));
  return TSD_OK;
}
extern "C" int tsd_ctx_timer_stop(tsd_ctx* c, float* ms) {
  if (!c || !ms) TSD_FAIL(TSD_E_ARG, "ctx/ms is NULL");
  HIP_TRY(hipEventRecord(c->ev1, c->stream));
  HIP_TRY(hipEventSynchronize(c->ev1));
  HIP_TRY(hipEventElapsedTime(ms, c->ev0, c->ev1));
  return TSD_OK;
}

extern "C" int tsd_ctx_profile_begin(tsd_ctx* c) {
  if (!c) TSD_FAIL(TSD_E_ARG, "ctx is NULL");
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->profile = true;
  c->prof_n = 0;
  return TSD_OK;
}
extern "C" int tsd_ctx_profile_end(tsd_ctx* c, float* ms_per_class, int* launches_per_class, int nclass) {
  if (!c || !ms_per_class || !launches_per_class) TSD_FAIL(TSD_E_ARG, "profile_end: NULL argument");
  c->profile = false;
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < nclass; i++) { ms_per_class[i] = 0.f; launches_per_class[i] = 0; }
  for (size_t i = 0; i < c->prof_n; i++) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
    const int k = c->prof_cls[i];
    if (k >= 0 && k < nclass) { ms_per_class[k] += ms; launches_per_class[k] += i < c->prof_kern.size() ? c->prof_kern[i] : 1; }
  }
  c->prof_n = 0;
  return TSD_OK;
}
// per-launch records of the last profiling pass: rec[i] = {class, M, N, K, batch}, ms[i]; returns the count
extern "C" int tsd_ctx_profile_records(tsd_ctx* c, int* rec, float* ms, int cap) {
  if (!c || !rec || !ms) TSD_FAIL(TSD_E_ARG, "profile_records: NULL argument");
  c->profile = false;
  HIP_TRY(hipStreamSynchronize(c->stream));
  int n = 0;
  for (size_t i = 0; i < c->prof_n && n < cap; i++, n++) {
    HIP_TRY(hipEventElapsedTime(&ms[n], c->prof_ev[2 * i], c->prof_ev[2 * i + 1]));
    rec[5 * n] = c->prof_cls[i];
    for (int j = 0; j < 4; j++) rec[5 * n + 1 + j] = c->prof_shape[4 * i + j];
  }
  return n;
}

int ctx_reserve_arena(tsd_ctx* c, size_t bytes) {
  if (c->arena.cap >= bytes) return TSD_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->arena.base) HIP_TRY(dev_free(c->arena.base));
  c->arena.base = nullptr;
  c->arena.cap = 0;
  const size_t want = bytes + (bytes >> 4) + (1 << 20);
  hipError_t e = dev_malloc((void**)&c->arena.base, want);
  if (e != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "workspace arena: allocating %zu bytes failed: %s", want, hipGetErrorString(e));
  c->arena.cap = want;
  if (c->opt.debug_poison >= 0 && (c->opt.debug_poison_what & 1)) HIP_TRY(hipMemsetAsync(c->arena.base, c->opt.debug_poison & 255, want, c->stream));  // on the context's stream: ordered before everything that uses the arena
  return TSD_OK;
}

int ctx_reserve_staging(tsd_ctx* c, size_t bytes) {
  if (c->staging_cap >= bytes) return TSD_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->staging) HIP_TRY(dev_free(c->staging));
  c->staging = nullptr;
  c->staging_cap = 0;
  hipError_t e = dev_malloc(&c->staging, bytes);
  if (e != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "staging: allocating %zu bytes failed: %s", bytes, hipGetErrorString(e));
  c->staging_cap = bytes;
  if (c->opt.debug_poison >= 0 && (c->opt.debug_poison_what & 16)) HIP_TRY(hipMemsetAsync(c->staging, c->opt.debug_poison & 255, bytes, c->stream));
  return TSD_OK;
}
