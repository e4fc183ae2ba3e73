// model.cpp - device-resident packed weights: one blob per model (what RCCL broadcasts),
// per-parameter upload/pack, synthetic counter-RNG init, and the resolved weight trees.
#include <math.h>
#include <string.h>

#include <vector>

#include "model.h"

bool attn_tail_weights_ok(const AttnW& w) {
  const int C = w.C;
  const bool plain = !w.ln[1].w && !w.ln[1].b && !w.ln[2].w && !w.ln[2].b && !w.gelu_erf;
  return plain && C == 320 && w.n_head == 8 && w.n_embed == 40 && w.sa_out.b && w.ca_out.b && w.geglu1.b && w.geglu2.b &&
         w.conv_out.b && !w.ca_q.b && w.sa_out.Kpad == C && w.ca_q.Kpad == C && w.ca_out.Kpad == C && w.geglu1.Kpad == C &&
         w.geglu2.Kpad == 4 * C && w.conv_out.Ipad == C && w.conv_out.k == 1;
}

bool attn_head_weights_ok(const AttnW& w) {
  const int C = w.C;
  return C == 320 && w.n_head == 8 && w.n_embed == 40 && !w.gn.w && !w.gn.b && !w.ln[0].w && !w.ln[0].b && w.conv_in.b &&
         w.conv_in.k == 1 && w.conv_in.Ipad == C && w.conv_in.Opad == C && !w.sa_in.b && w.sa_in.Kpad == C && w.sa_in.N == 3 * C;
}

// ---- duplicate-concat fold (UNetW::res_dup): host arithmetic on fp16 bit patterns, no HIP -------------------------------------------
// fp16 -> double is exact; the sum of two fp16 values spans at most 40 binades + 11 bits < 53, so the double sum is exact and the
// conversion back is the ONE rounding (nearest, ties to even; overflow -> inf; NaN keeps its top payload bits).
static double f16_bits_to_f64(uint16_t h) {
  const uint64_t sign = (uint64_t)(h & 0x8000) << 48;
  const int e = (h >> 10) & 31;
  const uint64_t m = h & 0x3FF;
  uint64_t u;
  if (e == 31) u = sign | (0x7FFull << 52) | (m << 42);
  else if (e == 0) {
    const double v = ldexp((double)m, -24);
    return sign ? -v : v;
  } else u = sign | ((uint64_t)(e - 15 + 1023) << 52) | (m << 42);
  double d;
  memcpy(&d, &u, 8);
  return d;
}

static uint16_t f64_to_f16_bits_rne(double v) {
  uint64_t u;
  memcpy(&u, &v, 8);
  const uint16_t sign = (uint16_t)((u >> 48) & 0x8000);
  const int e = (int)((u >> 52) & 0x7FF);
  uint64_t m = u & ((1ull << 52) - 1);
  if (e == 0x7FF) {
    uint16_t r = (uint16_t)(0x7C00 + (m >> 42));
    if (m && r == 0x7C00) r++;  // a NaN stays a NaN
    return sign | r;
  }
  if (e == 0) return sign;  // zero (a double subnormal is no sum of fp16 values)
  const int E = e - 1023;
  m |= 1ull << 52;  // v = m * 2^(E - 52); one fp16 ulp is 2^(E - 10) for a normal result, 2^-24 below 2^-14
  const int shift = 42 + (E < -14 ? -14 - E : 0);
  if (shift > 63) return sign;
  uint64_t q = m >> shift;
  const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) q++;
  // normal: q in [2^10, 2^11] and the exponent field is E + 15 - a carry out of the mantissa moves it up by itself; subnormal: q is the pattern
  uint64_t bits = E >= -14 ? ((uint64_t)(E + 14) << 10) + q : q;
  if (bits >= 0x7C00) bits = 0x7C00;
  return sign | (uint16_t)bits;
}

// out[o][t][c] = w[o][t][c] + w[o][t][half + c] for c < half, 0 for half <= c < ldo; w is [rows][taps][ldw] with ldw >= 2 * half.
// Returns how many sums are not finite.
static int64_t dup_fold_host(const uint16_t* w, int64_t rows, int taps, int ldw, int half, uint16_t* out, int ldo) {
  int64_t bad = 0;
  for (int64_t rt = 0; rt < rows * taps; rt++) {
    const uint16_t* s = w + rt * ldw;
    uint16_t* d = out + rt * ldo;
    for (int c = 0; c < half; c++) {
      const uint16_t a = s[c], b = s[half + c];
      d[c] = f64_to_f16_bits_rne(f16_bits_to_f64(a) + f16_bits_to_f64(b));
      bad += (d[c] & 0x7C00) == 0x7C00;
    }
    for (int c = half; c < ldo; c++) d[c] = 0;
  }
  return bad;
}

extern "C" int64_t tsd_debug_dup_fold_host(const void* w, int rows, int taps, int ldw, int half, void* out, int ldo) {
  if (!w || !out || rows <= 0 || taps <= 0 || half <= 0 || ldw < 2 * half || ldo < half) TSD_FAIL(TSD_E_ARG, "dup_fold_host: bad argument");
  return dup_fold_host((const uint16_t*)w, rows, taps, ldw, half, (uint16_t*)out, ldo);
}

// ---- upsample fold (ConvW::w_uf): a 3x3 convolution of a nearest-2x upsampled image as four 2x2 convolutions of the image itself ----------
// Output pixel (2 yi + py, 2 xi + px) reads source rows {yi - 1, yi} through kernel rows {0}, {1, 2} when py = 0 and rows {yi, yi + 1} through
// {0, 1}, {2} when py = 1; columns alike.  A group never straddles the border of the upsampled image, so its zero padding is the source's.
// out[q = 2 py + px][o][kh2][kw2][c] = the sum of w[o][kh][kw][c] over the two groups.  Up to four fp16 values: an integer multiple of 2^-24
// below 2^18, exact in double whatever the order; ONE rounding to fp16, nearest-even.  Returns how many sums are not finite.
static inline int uf_lo(int parity, int k2) { return parity == 0 ? (k2 == 0 ? 0 : 1) : (k2 == 0 ? 0 : 2); }
static inline int uf_hi(int parity, int k2) { return parity == 0 ? (k2 == 0 ? 0 : 2) : (k2 == 0 ? 1 : 2); }
int64_t ups_fold_host(const uint16_t* w, int O, int Ipad, int ldw, uint16_t* out) {
  // fp16 -> double through a table of all 65536 patterns (built once): the fold of the two production layers converts 50 M weights
  static const std::vector<double> f64_of = [] {
    std::vector<double> t(65536);
    for (int i = 0; i < 65536; i++) t[i] = f16_bits_to_f64((uint16_t)i);
    return t;
  }();
  int64_t bad = 0;
  for (int q = 0; q < 4; q++)
    for (int o = 0; o < O; o++)
      for (int t = 0; t < 4; t++) {
        const int py = q >> 1, px = q & 1, kh2 = t >> 1, kw2 = t & 1;
        uint16_t* d = out + (((size_t)q * O + o) * 4 + t) * Ipad;
        const uint16_t* s = w + (size_t)o * ldw;
        for (int c = 0; c < Ipad; c++) {
          double sum = 0.0;
          bool first = true;  // (the first term is taken as it is: a lone -0 stays -0)
          for (int kh = uf_lo(py, kh2); kh <= uf_hi(py, kh2); kh++)
            for (int kw = uf_lo(px, kw2); kw <= uf_hi(px, kw2); kw++) {
              const double v = f64_of[s[(size_t)(kh * 3 + kw) * Ipad + c]];
              sum = first ? v : sum + v;
              first = false;
            }
          d[c] = f64_to_f16_bits_rne(sum);
          bad += (d[c] & 0x7C00) == 0x7C00;
        }
      }
  return bad;
}
// the device layout of the fold: per parity the [O][4 * Ipad] matrix K-tile-major, [4 * Ipad / 64][O][64] (what launch_pack_tile_major makes
// of it), the four copies contiguous.  Ipad % 64 == 0.
int64_t ups_fold_pack_host(const uint16_t* w, int O, int Ipad, int ldw, uint16_t* out_tm) {
  const int K = 4 * Ipad;
  std::vector<uint16_t> f((size_t)4 * O * K);
  const int64_t bad = ups_fold_host(w, O, Ipad, ldw, f.data());
  for (int q = 0; q < 4; q++)
    for (int kt = 0; kt < K / 64; kt++)
      for (int o = 0; o < O; o++)
        memcpy(out_tm + (((size_t)q * (K / 64) + kt) * O + o) * 64, f.data() + ((size_t)q * O + o) * K + (size_t)kt * 64, 128);
  return bad;
}

extern "C" int64_t tsd_debug_ups_fold_host(const void* w, int O, int Ipad, int ldw, void* out) {
  if (!w || !out || O <= 0 || Ipad <= 0 || ldw < 9 * Ipad) TSD_FAIL(TSD_E_ARG, "ups_fold_host: bad argument");
  return ups_fold_host((const uint16_t*)w, O, Ipad, ldw, (uint16_t*)out);
}

// residual blocks of the 23-layer graph that read their input through the nearest-2x upsample (g_unet_forward: res(15, .., 1), res(20, .., 1))
static const int UPS_RES_BLOCKS[2] = {14, 19};
// structure only: a 3x3 conv1 over the block's own channels, whole K tiles per tap, the 160-column tile family
static bool ups_fold_weights_ok(const ResW& r) {
  return r.conv1.w && r.conv1.k == 3 && r.conv1.Ipad > 0 && r.conv1.Ipad % 64 == 0 && r.conv1.Ipad == r.cin && r.conv1.Opad % 160 == 0;
}

// parameters changed: derived buffers are stale until the next model_check_ready()
static void model_invalidate_derived(tsd_model* m) {
  m->ready = false;
  m->gen++;
  m->unet.res_dup_on = false; m->unet.res_dup = ResW();
  for (auto& a : m->unet.attn) { a.tail_stream = nullptr; a.head_stream = nullptr; a.fold_w = nullptr; a.fold_w_tm = nullptr; a.fold_b = nullptr; }
  m->unet.conv_in_im2col = nullptr;
  m->vae.conv_in_im2col = nullptr;
  for (auto& r : m->unet.res) { r.conv1.w_tm = nullptr; r.conv2.w_tm = nullptr; r.conv1.w_uf = nullptr; }
  m->unet.conv4.w_tm = nullptr; m->unet.conv7.w_tm = nullptr; m->unet.kproj_all.w_tm = nullptr;
  for (auto& cv : m->unet.conv) cv.w_tm = nullptr;
  for (auto& a : m->unet.attn) {
    for (LinW* l : {&a.sa_in, &a.sa_out, &a.ca_q, &a.ca_out, &a.geglu1, &a.geglu2}) l->w_tm = nullptr;
    a.conv_in.w_tm = nullptr; a.conv_out.w_tm = nullptr;
  }
}

static size_t packed_bytes(const ParamSpec& p) {
  if (!p.used) return 0;
  switch (p.kind) {
    case P_CONV_W: return (size_t)p.Opad * p.shape[2] * p.shape[3] * p.Kpad * sizeof(half_t);
    case P_CONV_B: return (size_t)p.Opad * sizeof(float);
    case P_LIN_W: return (size_t)p.rows() * p.Kpad * sizeof(half_t);
    default: return (size_t)p.shape[0] * sizeof(float);
  }
}

// the zeroed blob of a laid-out model and the views into it ...
static int model_init_blob(tsd_model* m) {
  tsd_ctx* ctx = m->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  hipError_t e = dev_malloc((void**)&m->blob, m->blob_bytes);
  if (e != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "weights: allocating %zu bytes failed: %s", m->blob_bytes, hipGetErrorString(e));
  HIP_TRY(hipMemsetAsync(m->blob, 0, m->blob_bytes, ctx->stream));
  return model_resolve(m);
}
// ... and everything a model owns on the device, released once the context's stream is idle: whatever exists of a model that failed
// half-way, or all of a live one (adapter snapshots included: a model may be destroyed merged).  The object itself goes too.
static void model_release(tsd_model* m) {
  (void)hipSetDevice(m->ctx->device);
  (void)hipStreamSynchronize(m->ctx->stream);
  if (m->blob) (void)dev_free(m->blob);
  if (m->derived) (void)dev_free(m->derived);
  for (auto& kv : m->lora_base) (void)dev_free(kv.second);
  delete m;
}

extern "C" int tsd_model_create(tsd_ctx* ctx, int kind, tsd_model** out) {
  if (!ctx || !out) TSD_FAIL(TSD_E_ARG, "tsd_model_create: NULL argument");
  if (!is_model_kind(kind)) TSD_FAIL(TSD_E_ARG, "bad model kind %d", kind);
  tsd_model* m = new tsd_model();
  m->ctx = ctx;
  m->kind = kind;
  m->params = build_param_specs(kind);
  // blob layout: time-projection weights (region 1) and biases (region 2) are laid out contiguously in
  // layer order so the nine Linear(1280,C) become ONE [6720][1280] GEMV (SURVEY.md App.D K8).
  size_t off = 0;
  for (auto& p : m->params) p.bytes = packed_bytes(p);
  {  // regions 1/2 densely packed (no gaps between the nine tensors), everything else 256-B aligned
    size_t o = 0;
    for (auto& p : m->params) if (p.region == 1) { p.off = o; o += p.bytes; }
    o = (o + 255) & ~size_t(255);
    for (auto& p : m->params) if (p.region == 2) { p.off = o; o += p.bytes; }
    o = (o + 255) & ~size_t(255);
    for (auto& p : m->params) if (p.region == 3) { p.off = o; o += p.bytes; }
    o = (o + 255) & ~size_t(255);
    for (auto& p : m->params) if (p.region == 4) { p.off = o; o += p.bytes; }
    o = (o + 255) & ~size_t(255);
    for (auto& p : m->params) if (p.region == 0) { p.off = o; o += p.bytes; o = (o + 255) & ~size_t(255); }
    off = o;
  }
  m->blob_bytes = off;
  for (size_t i = 0; i < m->params.size(); i++) m->index[m->params[i].name] = (int)i;
  m->loaded.assign(m->params.size(), 0);
  const int r = model_init_blob(m);
  if (r != TSD_OK) { model_release(m); return r; }  // the one way out of a model that did not come to be: nothing of it stays
  dev_handle_count(DEV_MODEL, +1);
  *out = m;
  return TSD_OK;
}

extern "C" int tsd_model_destroy(tsd_model* m) {
  if (!m) return TSD_OK;
  model_release(m);
  dev_handle_count(DEV_MODEL, -1);
  return TSD_OK;
}

// Forget the adapter snapshots (all of them, or the one of parameter `index`) WITHOUT restoring anything: what the blob holds now is the base.
// Call after the stream is idle.
static void lora_drop(tsd_model* m, int index = -1) {
  for (auto it = m->lora_base.begin(); it != m->lora_base.end();) {
    if (index >= 0 && it->first != index) { ++it; continue; }
    (void)dev_free(it->second);
    it = m->lora_base.erase(it);
  }
}

// pack parameter `i` from a device fp32 tensor in the reference layout
static int pack_param(tsd_model* m, int i, const float* dev_src) {
  tsd_ctx* ctx = m->ctx;
  const ParamSpec& p = m->params[i];
  if (!p.used) return TSD_OK;
  char* dst = m->blob + p.off;
  switch (p.kind) {
    case P_CONV_W:
      return launch_pack_conv(ctx, dev_src, (int)p.shape[0], (int)p.shape[1], (int)p.shape[2], (half_t*)dst, p.Opad,
                              p.Kpad);
    case P_CONV_B: return launch_pack_bias(ctx, dev_src, (int)p.shape[0], (float*)dst, p.Opad, 0);
    case P_LIN_W:
      return launch_pack_linear(ctx, dev_src, p.rows(), p.cols(), (half_t*)dst, p.Kpad, p.interleave);
    default: return launch_pack_bias(ctx, dev_src, (int)p.shape[0], (float*)dst, (int)p.shape[0], p.interleave);
  }
}

extern "C" int tsd_model_set_param(tsd_model* m, int index, const float* data, int64_t numel) {
  if (!m || !data) TSD_FAIL(TSD_E_ARG, "tsd_model_set_param: NULL argument");
  if (index < 0 || index >= (int)m->params.size()) TSD_FAIL(TSD_E_ARG, "param index %d out of range", index);
  const ParamSpec& p = m->params[index];
  if (numel != p.numel())
    TSD_FAIL(TSD_E_SHAPE, "param %s: got %lld elements, expected %lld", p.name.c_str(), (long long)numel,
             (long long)p.numel());
  m->loaded[index] = 1;
  if (!p.used) return TSD_OK;  // allocated by the reference, never read by its forward
  tsd_ctx* ctx = m->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(ctx_reserve_staging(ctx, (size_t)numel * sizeof(float)));
  HIP_TRY(hipMemcpyAsync(ctx->staging, data, (size_t)numel * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
  TSD_TRY(pack_param(m, index, (const float*)ctx->staging));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  lora_drop(m, index);  // the new value is the new base of this parameter
  model_invalidate_derived(m);
  return TSD_OK;
}

extern "C" int tsd_model_init_random(tsd_model* m, uint64_t seed) {
  if (!m) TSD_FAIL(TSD_E_ARG, "tsd_model_init_random: NULL model");
  tsd_ctx* ctx = m->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  int64_t maxn = 0;
  for (auto& p : m->params) if (p.used) maxn = std::max(maxn, p.numel());
  TSD_TRY(ctx_reserve_staging(ctx, (size_t)maxn * sizeof(float)));
  for (size_t i = 0; i < m->params.size(); i++) {
    const ParamSpec& p = m->params[i];
    m->loaded[i] = 1;
    if (!p.used) continue;
    float* tmp = (float*)ctx->staging;
    if (p.bound == 0.f) HIP_TRY(hipMemsetAsync(tmp, 0, (size_t)p.numel() * sizeof(float), ctx->stream));
    else TSD_TRY(launch_fill_uniform(ctx, tmp, p.numel(), seed, (uint64_t)m->kind * 4096 + i, p.bound));
    if (p.offset != 0.f) TSD_TRY(launch_add_const_f32(ctx, tmp, p.numel(), p.offset));
    TSD_TRY(pack_param(m, (int)i, tmp));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  lora_drop(m);
  model_invalidate_derived(m);
  return TSD_OK;
}

extern "C" int tsd_model_packed_blob(tsd_model* m, void** device_ptr, size_t* bytes) {
  if (!m || !device_ptr || !bytes) TSD_FAIL(TSD_E_ARG, "tsd_model_packed_blob: NULL argument");
  *device_ptr = m->blob;
  *bytes = m->blob_bytes;
  return TSD_OK;
}

extern "C" int tsd_model_mark_loaded(tsd_model* m) {
  if (!m) TSD_FAIL(TSD_E_ARG, "NULL model");
  std::fill(m->loaded.begin(), m->loaded.end(), 1);
  if (!m->lora_base.empty()) {  // the blob was written from outside (a weight broadcast): it is the base now
    HIP_TRY(hipSetDevice(m->ctx->device));
    HIP_TRY(hipStreamSynchronize(m->ctx->stream));
    lora_drop(m);
  }
  model_invalidate_derived(m);
  return TSD_OK;
}

// ---- reading a parameter back ---------------------------------------------------------------------------------------------------------
// host inverse of k_pack_linear / k_pack_conv on fp16 bit patterns: out is fp32 in the reference layout ([N][I], or [N][I][k][k])
void unpack_weight_host(const uint16_t* packed, int N, int I, int k, int ld, int interleave, float* out) {
  const int kk = k ? k * k : 1;
  for (int o = 0; o < N; o++) {
    const int prow = interleave ? (o < N / 2 ? 2 * o : 2 * (o - N / 2) + 1) : o;
    for (int t = 0; t < kk; t++) {
      const uint16_t* s = packed + ((size_t)prow * kk + t) * ld;
      float* d = out + (size_t)o * I * kk + t;
      for (int i = 0; i < I; i++) d[(size_t)i * kk] = (float)f16_bits_to_f64(s[i]);
    }
  }
}

static int param_checked(tsd_model* m, int index, const char* who) {
  if (!m) TSD_FAIL(TSD_E_ARG, "%s: NULL model", who);
  if (index < 0 || index >= (int)m->params.size()) TSD_FAIL(TSD_E_ARG, "%s: param index %d out of range", who, index);
  return TSD_OK;
}

// raw packed bytes of one parameter (debug / tests): out == NULL asks for the size; returns the byte count (0: the parameter is not used)
extern "C" int tsd_debug_model_packed_param(tsd_model* m, int index, void* out, size_t cap) {
  TSD_TRY(param_checked(m, index, "tsd_debug_model_packed_param"));
  const ParamSpec& p = m->params[index];
  if (!out || !p.bytes) return (int)p.bytes;
  if (cap < p.bytes) TSD_FAIL(TSD_E_ARG, "packed_param %s: %zu bytes do not fit %zu", p.name.c_str(), p.bytes, cap);
  HIP_TRY(hipSetDevice(m->ctx->device));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  HIP_TRY(hipMemcpy(out, m->blob + p.off, p.bytes, hipMemcpyDeviceToHost));
  return (int)p.bytes;
}

// The parameter as the forward reads it, unpacked to the reference layout in fp32: every weight is exactly an fp16 value (the model keeps
// no fp32 masters), biases and norm parameters are the fp32 that was set.  A parameter the forward never reads reads back as zeros.
extern "C" int tsd_model_get_param(tsd_model* m, int index, float* out, int64_t numel) {
  TSD_TRY(param_checked(m, index, "tsd_model_get_param"));
  if (!out) TSD_FAIL(TSD_E_ARG, "tsd_model_get_param: NULL argument");
  const ParamSpec& p = m->params[index];
  if (numel != p.numel())
    TSD_FAIL(TSD_E_SHAPE, "param %s: room for %lld elements, it has %lld", p.name.c_str(), (long long)numel, (long long)p.numel());
  if (!p.used) { memset(out, 0, (size_t)numel * sizeof(float)); return TSD_OK; }
  if (!m->loaded[index]) TSD_FAIL(TSD_E_STATE, "model parameter %s was never set", p.name.c_str());
  std::vector<char> raw(p.bytes);
  HIP_TRY(hipSetDevice(m->ctx->device));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  HIP_TRY(hipMemcpy(raw.data(), m->blob + p.off, p.bytes, hipMemcpyDeviceToHost));
  const int N = (int)p.shape[0];
  if (p.kind == P_CONV_W) unpack_weight_host((const uint16_t*)raw.data(), N, (int)p.shape[1], (int)p.shape[2], p.Kpad, 0, out);
  else if (p.kind == P_LIN_W) unpack_weight_host((const uint16_t*)raw.data(), p.rows(), p.cols(), 0, p.Kpad, p.interleave, out);
  else {
    const float* s = (const float*)raw.data();
    const bool inter = p.kind == P_LIN_B && p.interleave;
    for (int o = 0; o < N; o++) out[o] = s[inter ? (o < N / 2 ? 2 * o : 2 * (o - N / 2) + 1) : o];
  }
  return TSD_OK;
}

// ---- low-rank adapters (LoRA): W <- rn16(W + scale * up . down) on the packed fp16 weights, the base bits kept for an exact removal ------------
// Rows [row0, row0 + rows) of weight parameter `index`, host fp32 up [rows][rank] and down [rank][cols], cols in the reference column order
// (I for a linear layer, i * k * k + tap for a convolution).  The merge runs on a copy in the context's staging buffer (kernels_lora.hip) and
// replaces the parameter only when every merged value is finite: on any error the weights, the snapshots and lora_count are as before.
// The first merge into a parameter snapshots its packed bytes; later merges stack on the merged value, ONE rounding to fp16 each (so two
// stacked adapters are not bit-equal to one merge of their sum).  Synchronous.
extern "C" int tsd_model_lora_add(tsd_model* m, int index, int row0, int rows, const float* up, const float* down, int rank, float scale) {
  if (!m || !up || !down) TSD_FAIL(TSD_E_ARG, "tsd_model_lora_add: NULL argument");
  TSD_TRY(param_checked(m, index, "tsd_model_lora_add"));
  if (is_controlnet_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "lora_add: adapters on a ControlNet are not supported");
  if (is_ip_adapter_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "lora_add: adapters on an IP-Adapter are not supported");
  if (is_clip_vision_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "lora_add: adapters on the CLIP vision encoder are not supported");
  const ParamSpec& p = m->params[index];
  if (p.kind != P_CONV_W && p.kind != P_LIN_W) TSD_FAIL(TSD_E_ARG, "lora_add: %s is a bias / norm parameter, not a weight matrix", p.name.c_str());
  if (!p.used) TSD_FAIL(TSD_E_ARG, "lora_add: %s is never read by the forward", p.name.c_str());
  if (rank < 1 || rank > 1024) TSD_FAIL(TSD_E_ARG, "lora_add: rank %d outside 1..1024", rank);
  if (!(fabsf(scale) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "lora_add: scale is not finite");
  const int N = (int)p.shape[0], I = (int)p.shape[1], k = p.kind == P_CONV_W ? (int)p.shape[2] : 0;
  if (row0 < 0 || rows <= 0 || row0 > N - rows) TSD_FAIL(TSD_E_SHAPE, "lora_add: rows [%d, %d) outside %s (%d rows)", row0, row0 + rows, p.name.c_str(), N);
  if (!m->loaded[index]) TSD_FAIL(TSD_E_STATE, "model parameter %s was never set", p.name.c_str());
  tsd_ctx* ctx = m->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t cols = (size_t)I * (k ? k * k : 1);
  const size_t wb = (p.bytes + 255) & ~size_t(255), ub = ((size_t)rows * rank * 4 + 255) & ~size_t(255), db = (size_t)rank * cols * 4;
  TSD_TRY(ctx_reserve_staging(ctx, wb + ub + db));
  char* st = (char*)ctx->staging;
  HIP_TRY(hipMemcpyAsync(st, m->blob + p.off, p.bytes, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(st + wb, up, (size_t)rows * rank * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(st + wb + ub, down, db, hipMemcpyHostToDevice, ctx->stream));
  const bool was_planning = ctx->arena.planning;
  ctx->arena.planning = false;
  const int r = launch_lora_merge(ctx, (half_t*)st, N, I, k, p.Kpad, p.interleave, row0, rows, (const float*)(st + wb), (const float*)(st + wb + ub), rank, scale);
  ctx->arena.planning = was_planning;
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  TSD_TRY(r);
  TSD_TRY(ctx_check_status(ctx));  // TSD_E_NONFINITE (reported once, then cleared): a merged weight left fp16, or up / down held inf / NaN
  if (!m->lora_base.count(index)) {
    char* snap = nullptr;
    hipError_t e = dev_malloc((void**)&snap, p.bytes);
    if (e != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "lora_add: allocating %zu bytes for the base of %s failed: %s", p.bytes, p.name.c_str(), hipGetErrorString(e));
    // on the context's stream, like the copy over the parameter below: a device-to-device hipMemcpy on the null stream may still be reading
    // the base when that copy starts
    e = hipMemcpyAsync(snap, m->blob + p.off, p.bytes, hipMemcpyDeviceToDevice, ctx->stream);
    if (e != hipSuccess) { (void)dev_free(snap); TSD_FAIL(TSD_E_HIP, "lora_add: snapshot of %s: %s", p.name.c_str(), hipGetErrorString(e)); }
    m->lora_base[index] = snap;
  }
  HIP_TRY(hipMemcpyAsync(m->blob + p.off, st, p.bytes, hipMemcpyDeviceToDevice, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  model_invalidate_derived(m);
  return TSD_OK;
}

// every touched parameter back to its base, bit for bit; the snapshots are freed
extern "C" int tsd_model_lora_clear(tsd_model* m) {
  if (!m) TSD_FAIL(TSD_E_ARG, "tsd_model_lora_clear: NULL model");
  if (m->lora_base.empty()) return TSD_OK;
  tsd_ctx* ctx = m->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  for (auto& kv : m->lora_base) {
    const ParamSpec& p = m->params[kv.first];
    HIP_TRY(hipMemcpyAsync(m->blob + p.off, kv.second, p.bytes, hipMemcpyDeviceToDevice, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  lora_drop(m);
  model_invalidate_derived(m);
  return TSD_OK;
}

// parameters that currently differ from their base
extern "C" int tsd_model_lora_count(tsd_model* m) {
  if (!m) TSD_FAIL(TSD_E_ARG, "tsd_model_lora_count: NULL model");
  return (int)m->lora_base.size();
}

// derived device buffers (not part of the broadcast blob: every rank rebuilds them from the packed weights)
static int model_build_derived(tsd_model* m) {
  tsd_ctx* ctx = m->ctx;
  if (is_decoder_kind(m->kind) || is_encoder_kind(m->kind)) {  // first convolution of the VAE halves: im2col weights
    if (m->vae.conv.empty()) return TSD_OK;
    const ConvW& c0 = m->vae.conv[0];
    if (!(c0.w && c0.k == 3 && c0.I > 0 && 9 * c0.I <= 64 && c0.Ipad == 64)) return TSD_OK;
    const size_t need = (size_t)c0.Opad * 64 * sizeof(half_t);
    HIP_TRY(hipSetDevice(ctx->device));
    if (m->derived_bytes < need) {
      if (m->derived) HIP_TRY(dev_free(m->derived));
      m->derived = nullptr; m->derived_bytes = 0;
      hipError_t e = dev_malloc((void**)&m->derived, need);
      if (e != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "derived weights: allocating %zu bytes failed: %s", need, hipGetErrorString(e));
      m->derived_bytes = need;
      if (ctx->opt.debug_poison >= 0 && (ctx->opt.debug_poison_what & 2)) HIP_TRY(hipMemsetAsync(m->derived, ctx->opt.debug_poison & 255, need, ctx->stream));
    }
    const bool wp = ctx->arena.planning;
    ctx->arena.planning = false;
    const int r = launch_pack_im2col_w(ctx, c0.w, c0.Opad, c0.Ipad, c0.I, (half_t*)m->derived);
    ctx->arena.planning = wp;
    if (r == TSD_OK) m->vae.conv_in_im2col = (const half_t*)m->derived;
    return r;
  }
  if (!is_diffusion_kind(m->kind) && !is_controlnet_kind(m->kind)) return TSD_OK;
  const bool full_graph = is_full_unet_kind(m->kind) || is_controlnet_kind(m->kind);  // a ControlNet is the full-size graph's encoder half
  std::vector<AttnW*> el;
  for (auto& a : m->unet.attn) if (a.C && (attn_tail_weights_ok(a) || attn_head_weights_ok(a))) el.push_back(&a);
  // input convolution (4 latent channels): [Opad][64] im2col weights
  const ConvW& cin = full_graph ? (m->unet.conv.empty() ? m->unet.conv1 : m->unet.conv[0]) : m->unet.conv1;
  const bool cin_ok = cin.w && cin.k == 3 && cin.I > 0 && 9 * cin.I <= 64 && cin.Ipad == 64;
  const size_t cin_b = cin_ok ? ((size_t)cin.Opad * 64 * sizeof(half_t) + 255) & ~size_t(255) : 0;
  // weight-heavy 3x3 convs (>= TSD_CONV_W_TM MiB of weights; 0 = off): K-tile-major copies
  const int tm_mib = ctx->opt.conv_w_tm_mib;  // measured: +0.3 % headline, +0.6 % full-size UNet (profiles/r03_conv_w_tile_major_ab.txt)
  // linear layers / 1x1 convs: TSD_LIN_W_TM = 0 turns them off, TSD_LIN_W_TM_KIB sets the size threshold (default 1 MiB; with 512 KiB the
  // 800-KB 640 x 640 projections of the 32x32 level join in: measured equal, 205.65 vs 205.60 steps/s)
  const int tml_kib = ctx->opt.lin_w_tm_kib;
  const size_t tml_bytes = (size_t)(tml_kib > 0 ? tml_kib : 1024) << 10;
  // Layer 10 of the Tiny-SD graph reads concat(a[9], a[9]) (g_unet_forward; diffusion.mojo:253-256): its conv1 / skip weights with the two
  // input-channel halves added (UNetW::res_dup).  Structure only: an even split into multiples of 64 channels, an even group count whose
  // groups do not straddle the halves, and no per-channel affine (that would differ between the halves).
  bool dup = false;
  if (ctx->opt.fold_dup && !full_graph && m->unet.res.size() > 9 && m->unet.attn.size() > 8) {
    const ResW& r = m->unet.res[9];
    const int half = r.cin / 2;
    dup = r.cin > 0 && r.cin % 2 == 0 && half % 64 == 0 && m->unet.attn[8].C == half && r.groups % 2 == 0 && half % (r.groups / 2) == 0 &&
          r.conv1.w && r.conv1.k == 3 && r.conv1.Ipad == r.cin && r.has_skip && r.skip.w && r.skip.k == 1 && r.skip.Ipad == r.cin &&
          r.skip.Opad == r.conv1.Opad && !r.gn1.w && !r.gn1.b;  // (NormAffine::torch_rstd only counts when the affine is passed: g_resblock)
  }
  size_t dup_w1_b = 0, dup_sk_b = 0, dup_tm_b = 0;
  if (dup) {
    const ResW& r = m->unet.res[9];
    dup_w1_b = (((size_t)r.conv1.Opad * 9 * (r.cin / 2) * 2) + 255) & ~size_t(255);
    dup_sk_b = (((size_t)r.skip.Opad * (r.cin / 2) * 2) + 255) & ~size_t(255);
    if (tm_mib > 0 && (size_t)r.conv1.Opad * 9 * (r.cin / 2) * 2 >= (size_t)tm_mib << 20) dup_tm_b = dup_w1_b;
  }
  std::vector<ConvW*> tm;
  size_t tm_b = 0;
  if (tm_mib > 0)
    for (auto& r : m->unet.res)
      for (ConvW* c : {&r.conv1, &r.conv2})
        // (the graph runs the folded conv1 of layer 10: no tile-major copy of the unfolded one)
        if (!(dup && c == &m->unet.res[9].conv1) && c->w && c->k == 3 && (size_t)c->Opad * 9 * c->Ipad * 2 >= (size_t)tm_mib << 20) { tm.push_back(c); tm_b += (((size_t)c->Opad * 9 * c->Ipad * 2) + 255) & ~size_t(255); }
  if (tm_mib > 0) {  // downsampling / upsampling convs outside the residual blocks
    for (ConvW* c : {&m->unet.conv4, &m->unet.conv7})
      if (c->w && c->k == 3 && (size_t)c->Opad * 9 * c->Ipad * 2 >= (size_t)tm_mib << 20) { tm.push_back(c); tm_b += (((size_t)c->Opad * 9 * c->Ipad * 2) + 255) & ~size_t(255); }
    for (auto& cv : m->unet.conv)
      if (cv.w && cv.k == 3 && (size_t)cv.Opad * 9 * cv.Ipad * 2 >= (size_t)tm_mib << 20) { tm.push_back(&cv); tm_b += (((size_t)cv.Opad * 9 * cv.Ipad * 2) + 255) & ~size_t(255); }
  }
  if (tm_mib > 0 && ctx->opt.lin_w_tm != 0)
    for (auto& a : m->unet.attn)
      if (a.C && !(attn_tail_weights_ok(a) && attn_head_weights_ok(a)))
        for (ConvW* c : {&a.conv_in, &a.conv_out})
          if (c->w && c->k == 1 && c->Ipad % 64 == 0 && (size_t)c->Opad * c->Ipad * 2 >= tml_bytes) { tm.push_back(c); tm_b += (((size_t)c->Opad * c->Ipad * 2) + 255) & ~size_t(255); }
  // ... and of the attention blocks' linear layers (TSD_LIN_W_TM MiB; the 64x64-level blocks read theirs through the fused kernels' streams)
  const int tml_mib = ctx->opt.lin_w_tm;  // measured: +0.4 % headline, +0.6 % full-size UNet (profiles/r03_lin_w_tile_major_ab.txt)
  std::vector<LinW*> tml;
  if (tml_mib > 0)
    for (auto& a : m->unet.attn)
      if (a.C && !(attn_tail_weights_ok(a) && attn_head_weights_ok(a)))
        for (LinW* l : {&a.sa_in, &a.sa_out, &a.ca_q, &a.ca_out, &a.geglu1, &a.geglu2})
          if (l->w && l->Kpad % 64 == 0 && l->Kpad == l->K && (size_t)l->N * l->Kpad * 2 >= tml_bytes) { tml.push_back(l); tm_b += (((size_t)l->N * l->Kpad * 2) + 255) & ~size_t(255); }
  LinW* kv = nullptr;  // k_proj | v_proj rows of all blocks (adjacent in the blob: the fused context projection of g_unet_forward)
  if (tml_mib > 0 && m->unet.kproj_all.w && m->unet.vproj_all.w == m->unet.kproj_all.w + (int64_t)m->unet.kproj_all.N * m->unet.kproj_all.Kpad &&
      m->unet.kproj_all.Kpad % 64 == 0 && m->unet.vproj_all.N == m->unet.kproj_all.N) {
    kv = &m->unet.kproj_all;
    tm_b += (((size_t)2 * kv->N * kv->Kpad * 2) + 255) & ~size_t(255);
  }
  // GEGLU's second linear folded into the output 1x1 convolution (AttnW::fold_w): blocks that do not run the fused tail kernel
  std::vector<AttnW*> fold;
  size_t fold_b = 0;
  if (ctx->opt.fold_out)
    for (auto& a : m->unet.attn)
      if (a.C && !attn_tail_weights_ok(a) && a.geglu2.w && a.conv_out.w && a.conv_out.k == 1 && a.conv_out.Ipad == a.C && a.conv_out.Opad == a.C &&
          a.geglu2.N == a.C && a.geglu2.Kpad == 4 * a.C && a.geglu2.K == 4 * a.C && a.C % 64 == 0) {
        fold.push_back(&a);
        fold_b += 2 * ((((size_t)a.C * 5 * a.C * 2) + 255) & ~size_t(255)) + ((((size_t)a.C * 4) + 255) & ~size_t(255));
      }
  // conv1 of the blocks behind a nearest-2x upsample: the upsample folded into four 2x2 parity kernels (ConvW::w_uf).  Built whatever
  // TSD_UPS_FOLD says - the option is read per forward, by the graph - and keyed on structure only, never on a batch or a latent size.
  std::vector<ConvW*> uf;
  size_t uf_b = 0;
  if (!full_graph)
    for (int bi : UPS_RES_BLOCKS)
      if (bi < (int)m->unet.res.size() && ups_fold_weights_ok(m->unet.res[bi])) {
        ConvW* c = &m->unet.res[bi].conv1;
        uf.push_back(c);
        uf_b += (((size_t)16 * c->Opad * c->Ipad * 2) + 255) & ~size_t(255);
      }
  if (el.empty() && !cin_ok && tm.empty() && tml.empty() && !kv && fold.empty() && !dup && uf.empty()) return TSD_OK;
  const size_t tail_b = (attn_tail_stream_bytes() + 255) & ~size_t(255), head_b = (attn_head_stream_bytes() + 255) & ~size_t(255);
  const size_t each = tail_b + head_b, need = each * el.size() + cin_b + tm_b + fold_b + dup_w1_b + dup_sk_b + dup_tm_b + uf_b;
  HIP_TRY(hipSetDevice(ctx->device));
  if (m->derived_bytes < need) {
    if (m->derived) HIP_TRY(dev_free(m->derived));
    m->derived = nullptr; m->derived_bytes = 0;
    hipError_t e = dev_malloc((void**)&m->derived, need);
    if (e != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "derived weights: allocating %zu bytes failed: %s", need, hipGetErrorString(e));
    m->derived_bytes = need;
    if (ctx->opt.debug_poison >= 0 && (ctx->opt.debug_poison_what & 2)) HIP_TRY(hipMemsetAsync(m->derived, ctx->opt.debug_poison & 255, need, ctx->stream));
  }
  const bool was_planning = ctx->arena.planning;
  ctx->arena.planning = false;
  int r = TSD_OK;
  for (size_t i = 0; i < el.size() && r == TSD_OK; i++) {
    AttnW& a = *el[i];
    half_t* dst = (half_t*)(m->derived + i * each);
    if (attn_tail_weights_ok(a)) {
      r = launch_attn_tail_pack(ctx, a.sa_out.w, a.sa_out.Kpad, a.ca_q.w, a.ca_q.Kpad, a.ca_out.w, a.ca_out.Kpad, a.geglu1.w,
                                a.geglu1.Kpad, a.geglu2.w, a.geglu2.Kpad, a.conv_out.w, a.conv_out.Ipad, dst);
      if (r == TSD_OK) a.tail_stream = dst;
    }
    if (r == TSD_OK && attn_head_weights_ok(a)) {
      half_t* hd = (half_t*)(m->derived + i * each + tail_b);
      r = launch_attn_head_pack(ctx, a.conv_in.w, a.conv_in.Ipad, a.sa_in.w, a.sa_in.Kpad, hd);
      if (r == TSD_OK) a.head_stream = hd;
    }
  }
  if (r == TSD_OK && cin_ok) {
    half_t* dst = (half_t*)(m->derived + each * el.size());
    r = launch_pack_im2col_w(ctx, cin.w, cin.Opad, cin.Ipad, cin.I, dst);
    if (r == TSD_OK) m->unet.conv_in_im2col = dst;
  }
  {
    size_t off = each * el.size() + cin_b;
    for (size_t i = 0; i < tm.size() && r == TSD_OK; i++) {
      ConvW* c = tm[i];
      half_t* dst = (half_t*)(m->derived + off);
      r = launch_pack_tile_major(ctx, c->w, c->Opad, c->k * c->k * c->Ipad, dst);
      if (r == TSD_OK) c->w_tm = dst;
      off += (((size_t)c->Opad * c->k * c->k * c->Ipad * 2) + 255) & ~size_t(255);
    }
    if (kv && r == TSD_OK) {
      half_t* dst = (half_t*)(m->derived + off);
      r = launch_pack_tile_major(ctx, kv->w, 2 * kv->N, kv->Kpad, dst);
      if (r == TSD_OK) kv->w_tm = dst;
      off += (((size_t)2 * kv->N * kv->Kpad * 2) + 255) & ~size_t(255);
    }
    for (size_t i = 0; i < tml.size() && r == TSD_OK; i++) {
      LinW* l = tml[i];
      half_t* dst = (half_t*)(m->derived + off);
      r = launch_pack_tile_major(ctx, l->w, l->N, l->Kpad, dst);
      if (r == TSD_OK) l->w_tm = dst;
      off += (((size_t)l->N * l->Kpad * 2) + 255) & ~size_t(255);
    }
    for (size_t i = 0; i < fold.size() && r == TSD_OK; i++) {
      AttnW* a = fold[i];
      const int C = a->C;
      const size_t wb = (((size_t)C * 5 * C * 2) + 255) & ~size_t(255);
      half_t* wf = (half_t*)(m->derived + off);
      half_t* wf_tm = (half_t*)(m->derived + off + wb);
      float* bf = (float*)(m->derived + off + 2 * wb);
      r = launch_fold_linear_conv1x1(ctx, a->conv_out.w, a->conv_out.Ipad, a->conv_out.b, a->geglu2.w, a->geglu2.Kpad, a->geglu2.b, C, 4 * C, wf, 5 * C, bf);
      if (r == TSD_OK) r = launch_pack_tile_major(ctx, wf, C, 5 * C, wf_tm);
      if (r == TSD_OK) { a->fold_w = wf; a->fold_w_tm = wf_tm; a->fold_b = bf; }
      off += 2 * wb + ((((size_t)C * 4) + 255) & ~size_t(255));
    }
    if (dup && r == TSD_OK) {
      // Host-side and exact: both halves to the host, summed in double (two fp16 values can be 40 binades apart), rounded to fp16 once.
      // Once per build of the derived buffers; a sum that leaves fp16 must not be silent (as for the attention blocks' fold below).
      const ResW& r10 = m->unet.res[9];
      const int half = r10.cin / 2;
      const size_t n1 = (size_t)r10.conv1.Opad * 9 * r10.cin, ns = (size_t)r10.skip.Opad * r10.cin;
      std::vector<uint16_t> src(std::max(n1, ns)), dst(std::max(n1, ns) / 2);
      half_t* w1 = (half_t*)(m->derived + off);
      half_t* wsk = (half_t*)(m->derived + off + dup_w1_b);
      half_t* w1_tm = dup_tm_b ? (half_t*)(m->derived + off + dup_w1_b + dup_sk_b) : nullptr;
      off += dup_w1_b + dup_sk_b + dup_tm_b;
      int64_t bad = 0;
      hipError_t e = hipStreamSynchronize(ctx->stream);
      for (int k = 0; k < 2 && e == hipSuccess; k++) {
        const ConvW& c = k ? r10.skip : r10.conv1;
        const size_t n = k ? ns : n1;
        e = hipMemcpy(src.data(), c.w, n * 2, hipMemcpyDeviceToHost);
        if (e != hipSuccess) break;
        bad += dup_fold_host(src.data(), c.Opad, c.k * c.k, c.Ipad, half, dst.data(), half);
        e = hipMemcpyAsync(k ? wsk : w1, dst.data(), n, hipMemcpyHostToDevice, ctx->stream);  // n / 2 folded weights of 2 bytes
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      }
      if (e != hipSuccess) {
        tsd_set_error("duplicate-concat fold: %s", hipGetErrorString(e));
        r = TSD_E_HIP;
      } else if (bad) {
        tsd_set_error("unet.layer10: %lld folded conv1 / skip weights are not finite (the sum of the two input-channel halves leaves fp16)",
                      (long long)bad);
        r = TSD_E_NONFINITE;
      } else {
        ResW d = r10;  // conv2 (with the tile-major copy made above), biases, time projection, second norm: shared
        d.cin = half; d.groups_in = r10.groups / 2;
        d.conv1.w = w1; d.conv1.I = half; d.conv1.Ipad = half; d.conv1.w_tm = nullptr;
        d.skip.w = wsk; d.skip.I = half; d.skip.Ipad = half; d.skip.w_tm = nullptr;
        if (w1_tm) {
          r = launch_pack_tile_major(ctx, w1, d.conv1.Opad, 9 * half, w1_tm);
          if (r == TSD_OK) d.conv1.w_tm = w1_tm;
        }
        if (r == TSD_OK) { m->unet.res_dup = d; m->unet.res_dup_on = true; }
      }
    }
    for (size_t i = 0; i < uf.size() && r == TSD_OK; i++) {
      // host-side and exact like the duplicate-concat fold above; a sum that leaves fp16 must not be silent
      ConvW* c = uf[i];
      const size_t nsrc = (size_t)c->Opad * 9 * c->Ipad, ndst = (size_t)16 * c->Opad * c->Ipad;
      std::vector<uint16_t> src(nsrc), dst(ndst);
      half_t* dev = (half_t*)(m->derived + off);
      off += ((ndst * 2) + 255) & ~size_t(255);
      hipError_t e = hipStreamSynchronize(ctx->stream);
      if (e == hipSuccess) e = hipMemcpy(src.data(), c->w, nsrc * 2, hipMemcpyDeviceToHost);
      int64_t bad = 0;
      if (e == hipSuccess) {
        bad = ups_fold_pack_host(src.data(), c->Opad, c->Ipad, 9 * c->Ipad, dst.data());
        e = hipMemcpyAsync(dev, dst.data(), ndst * 2, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
      }
      if (e != hipSuccess) {
        tsd_set_error("upsample fold: %s", hipGetErrorString(e));
        r = TSD_E_HIP;
      } else if (bad) {
        tsd_set_error("residual block behind an upsample (%d -> %d): %lld folded conv1 weights are not finite (a sum of up to four taps leaves fp16)",
                      c->Ipad, c->Opad, (long long)bad);
        r = TSD_E_NONFINITE;
      } else {
        c->w_uf = dev;
      }
    }
  }
  // A folded weight is a product of two weight matrices rounded to fp16 once: one that leaves fp16 (or a non-finite bias) must not be
  // silent.  Host-side scan, once per build of the derived buffers.
  if (r == TSD_OK && !fold.empty()) {
    hipError_t e = hipStreamSynchronize(ctx->stream);
    for (size_t i = 0; i < fold.size() && r == TSD_OK && e == hipSuccess; i++) {
      const AttnW* a = fold[i];
      const int C = a->C;
      std::vector<uint16_t> hw((size_t)C * 5 * C);
      std::vector<float> hb(C);
      e = hipMemcpy(hw.data(), a->fold_w, hw.size() * 2, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(hb.data(), a->fold_b, hb.size() * 4, hipMemcpyDeviceToHost);
      if (e != hipSuccess) break;
      int64_t bad = 0;
      for (uint16_t v : hw) bad += (v & 0x7C00) == 0x7C00;
      for (float v : hb) bad += !(fabsf(v) <= 3.4028235e38f);
      if (bad) {
        fold[i]->fold_w = nullptr; fold[i]->fold_w_tm = nullptr; fold[i]->fold_b = nullptr;
        tsd_set_error("attention block with C = %d: %lld folded weights / biases are not finite (W_out . W_2 leaves fp16)", C, (long long)bad);
        r = TSD_E_NONFINITE;
      }
    }
    if (e != hipSuccess && r == TSD_OK) {
      tsd_set_error("fold check: %s", hipGetErrorString(e));
      r = TSD_E_HIP;
    }
  }
  ctx->arena.planning = was_planning;
  return r;
}

int model_check_ready(tsd_model* m) {
  if (m->ready) return TSD_OK;
  for (size_t i = 0; i < m->params.size(); i++)
    if (m->params[i].used && !m->loaded[i])
      TSD_FAIL(TSD_E_STATE, "model parameter %s was never set", m->params[i].name.c_str());
  TSD_TRY(model_build_derived(m));
  m->ready = true;
  return TSD_OK;
}

extern "C" int tsd_model_prepare(tsd_model* m) {
  if (!m) TSD_FAIL(TSD_E_ARG, "NULL model");
  HIP_TRY(hipSetDevice(m->ctx->device));
  TSD_TRY(model_check_ready(m));
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  return TSD_OK;
}

// Debug entry: the folded [C][5C] fp16 weight and fp32 bias of attention block `block` (index into the UNet's layers); returns C,
// 0 when that block does not fold
extern "C" int tsd_debug_model_fold(tsd_model* m, int block, void* wf, float* bf) {
  if (!m) TSD_FAIL(TSD_E_ARG, "NULL model");
  if (!is_diffusion_kind(m->kind) || block < 0 || block >= (int)m->unet.attn.size())
    TSD_FAIL(TSD_E_ARG, "model_fold: no attention block %d in this model", block);
  HIP_TRY(hipSetDevice(m->ctx->device));
  TSD_TRY(model_check_ready(m));
  const AttnW& a = m->unet.attn[block];
  if (!a.fold_w) return 0;
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  if (wf) HIP_TRY(hipMemcpy(wf, a.fold_w, (size_t)a.C * 5 * a.C * 2, hipMemcpyDeviceToHost));
  if (bf) HIP_TRY(hipMemcpy(bf, a.fold_b, (size_t)a.C * 4, hipMemcpyDeviceToHost));
  return a.C;
}

// Debug entry: the folded conv1 [Opad][9][cin/2] and skip [Opad][cin/2] fp16 weights of the duplicate-concat block (UNet layer 10);
// returns cin/2, 0 when this model / context does not fold
extern "C" int tsd_debug_model_dup_fold(tsd_model* m, void* conv1_w, void* skip_w) {
  if (!m) TSD_FAIL(TSD_E_ARG, "NULL model");
  if (!is_diffusion_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "model_dup_fold: not a diffusion model");
  HIP_TRY(hipSetDevice(m->ctx->device));
  TSD_TRY(model_check_ready(m));
  if (!m->unet.res_dup_on) return 0;
  const ResW& d = m->unet.res_dup;
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  if (conv1_w) HIP_TRY(hipMemcpy(conv1_w, d.conv1.w, (size_t)d.conv1.Opad * 9 * d.conv1.Ipad * 2, hipMemcpyDeviceToHost));
  if (skip_w) HIP_TRY(hipMemcpy(skip_w, d.skip.w, (size_t)d.skip.Opad * d.skip.Ipad * 2, hipMemcpyDeviceToHost));
  return d.cin;
}

// Debug entry: the device copy of residual block `block`'s folded conv1 (index into the UNet's layers) - four parity copies, each
// [4 * Ipad / 64][Opad][64] fp16; returns Ipad, 0 when the block does not fold
extern "C" int tsd_debug_model_ups_fold(tsd_model* m, int block, void* out) {
  if (!m) TSD_FAIL(TSD_E_ARG, "NULL model");
  if (!is_diffusion_kind(m->kind) || block < 0 || block >= (int)m->unet.res.size())
    TSD_FAIL(TSD_E_ARG, "model_ups_fold: no residual block %d in this model", block);
  HIP_TRY(hipSetDevice(m->ctx->device));
  TSD_TRY(model_check_ready(m));
  const ConvW& c = m->unet.res[block].conv1;
  if (!c.w_uf) return 0;
  HIP_TRY(hipStreamSynchronize(m->ctx->stream));
  if (out) HIP_TRY(hipMemcpy(out, c.w_uf, (size_t)16 * c.Opad * c.Ipad * 2, hipMemcpyDeviceToHost));
  return c.Ipad;
}

ConvW model_conv(const tsd_model* m, const std::string& prefix) {
  ConvW w;
  auto it = m->index.find(prefix + ".kernel");
  if (it == m->index.end()) return w;
  const ParamSpec& pw = m->params[it->second];
  const ParamSpec& pb = m->params[it->second + 1];
  if (!pw.used) return w;
  w.w = (const half_t*)(m->blob + pw.off);
  w.b = (const float*)(m->blob + pb.off);
  w.O = (int)pw.shape[0]; w.I = (int)pw.shape[1]; w.k = (int)pw.shape[2]; w.Ipad = pw.Kpad; w.Opad = pw.Opad;
  return w;
}

LinW model_lin(const tsd_model* m, const std::string& prefix, bool use_bias) {
  LinW w;
  auto it = m->index.find(prefix + ".weight");
  if (it == m->index.end()) return w;
  const ParamSpec& pw = m->params[it->second];
  const ParamSpec& pb = m->params[it->second + 1];
  w.w = (const half_t*)(m->blob + pw.off);
  w.b = (use_bias && pb.used) ? (const float*)(m->blob + pb.off) : nullptr;
  w.N = (int)pw.shape[0]; w.K = (int)pw.shape[1]; w.Kpad = pw.Kpad;
  return w;
}

int model_resolve(tsd_model* m) {
  if (is_ip_adapter_kind(m->kind)) {
    IpAdapterW& ip = m->ip;
    auto aff = [&](const std::string& name) {
      NormAffine a;
      a.w = (const float*)(m->blob + m->params[m->index.at(name + ".weight")].off);
      a.b = (const float*)(m->blob + m->params[m->index.at(name + ".bias")].off);
      a.torch_rstd = 1;
      return a;
    };
    if (is_ip_plus_kind(m->kind)) {  // the resampler in place of image_proj.proj / .norm
      auto linw = [&](const std::string& name) {  // a weight with no bias entry behind it
        const ParamSpec& pw = m->params[m->index.at(name + ".weight")];
        LinW w;
        w.w = (const half_t*)(m->blob + pw.off); w.N = pw.rows(); w.K = pw.cols(); w.Kpad = pw.Kpad;
        return w;
      };
      ip.n_tokens = IPP_TOKENS;
      ip.latents = (const half_t*)(m->blob + m->params[m->index.at("image_proj.latents")].off);
      ip.proj_in = model_lin(m, "image_proj.proj_in", true);
      ip.proj_out = model_lin(m, "image_proj.proj_out", true);
      ip.norm_out = aff("image_proj.norm_out");
      for (int l = 0; l < IPP_DEPTH; l++) {
        const std::string n = "image_proj.layers." + std::to_string(l);
        IpResampleLayerW& w = ip.layer[l];
        w.norm1 = aff(n + ".0.norm1"); w.norm2 = aff(n + ".0.norm2"); w.ff_norm = aff(n + ".1.0");
        w.to_q = linw(n + ".0.to_q"); w.to_kv = linw(n + ".0.to_kv"); w.to_out = linw(n + ".0.to_out");
        w.ff1 = linw(n + ".1.1"); w.ff2 = linw(n + ".1.3");
      }
    } else {
      ip.n_tokens = IP_SD15_TOKENS;
      ip.proj = model_lin(m, "image_proj.proj", true);
      ip.norm = aff("image_proj.norm");
    }
    int kvoff = 0, t = 0;
    for (int i = 0; i < SD15_N; i++) {
      const LayerDef& l = SD15_STEPS[i].l;
      ip.kv_off[i] = 0; ip.C[i] = 0;
      if (l.kind != L_ATTN) continue;
      const std::string n = "ip_adapter." + std::to_string(ip_adapter_published_index(t++));
      const ParamSpec& pk = m->params[m->index.at(n + ".to_k_ip.weight")];
      const ParamSpec& pv = m->params[m->index.at(n + ".to_v_ip.weight")];
      if (kvoff == 0) {  // the two tables are contiguous in the blob (regions 3 / 4), in the order of the list
        LinW& k = m->unet.kproj_all; LinW& v = m->unet.vproj_all;
        k.w = (const half_t*)(m->blob + pk.off); k.b = nullptr; k.K = (int)pk.shape[1]; k.Kpad = pk.Kpad;
        v.w = (const half_t*)(m->blob + pv.off); v.b = nullptr; v.K = (int)pv.shape[1]; v.Kpad = pv.Kpad;
      }
      ip.kv_off[i] = kvoff; ip.C[i] = l.a * l.b;
      kvoff += l.a * l.b;
    }
    ip.n_blocks = t;
    m->unet.kproj_all.N = kvoff; m->unet.vproj_all.N = kvoff;  // 12480 rows each
    return TSD_OK;
  }
  if (is_clip_vision_kind(m->kind)) {
    ClipVisionW& v = m->vision;
    auto aff = [&](const std::string& name) {
      NormAffine a;
      a.w = (const float*)(m->blob + m->params[m->index.at(name + ".weight")].off);
      a.b = (const float*)(m->blob + m->params[m->index.at(name + ".bias")].off);
      a.torch_rstd = 1;
      return a;
    };
    auto linw = [&](const std::string& name) {  // a weight with no bias entry behind it
      const ParamSpec& pw = m->params[m->index.at(name + ".weight")];
      LinW w;
      w.w = (const half_t*)(m->blob + pw.off); w.N = (int)pw.shape[0]; w.K = (int)pw.shape[1]; w.Kpad = pw.Kpad;
      return w;
    };
    v.cls = (const float*)(m->blob + m->params[m->index.at("embeddings.class_embedding")].off);
    v.patch = linw("embeddings.patch_embedding");
    v.pos = linw("embeddings.position_embedding").w;
    v.pre_ln = aff("pre_layrnorm");
    for (int i = 0; i < CV_LAYERS; i++) {
      const std::string n = "layers." + std::to_string(i);
      ClipVisionLayerW& l = v.layer[i];
      l.ln1 = aff(n + ".ln1"); l.ln2 = aff(n + ".ln2");
      l.in_proj = model_lin(m, n + ".in_proj", true);
      l.out_proj = model_lin(m, n + ".out_proj", true);
      l.fc1 = model_lin(m, n + ".fc1", true);
      l.fc2 = model_lin(m, n + ".fc2", true);
    }
    v.post_ln = aff("post_layernorm");
    v.proj = linw("visual_projection");
    return TSD_OK;
  }
  if (is_diffusion_kind(m->kind) || is_controlnet_kind(m->kind)) {
    UNetW& u = m->unet;
    const bool cn = is_controlnet_kind(m->kind);
    const bool full = is_full_unet_kind(m->kind) || cn;
    const bool torch_norms = is_torch_unet_kind(m->kind);
    auto aff = [&](const std::string& name) {
      NormAffine a;
      if (torch_norms) {
        a.w = (const float*)(m->blob + m->params[m->index.at(name + ".weight")].off);
        a.b = (const float*)(m->blob + m->params[m->index.at(name + ".bias")].off);
        a.torch_rstd = 1;
      }
      return a;
    };
    const int n_layers = cn ? SD15_ENC_N : (full ? SD15_N : 23);
    u.res.assign(n_layers, ResW());
    u.attn.assign(n_layers, AttnW());
    u.conv.assign(n_layers, ConvW());
    u.t1 = model_lin(m, "time_embed.layer1", true);
    u.t2 = model_lin(m, "time_embed.layer2", true);
    int toff = 0, kvoff = 0;
    bool first = true;
    for (int i = 0; i < n_layers; i++) {
      const LayerDef& l = full ? full_unet_steps(m->kind)[i].l : UNET_LAYERS[i];
      const std::string n = "unet.layer" + std::to_string(i + 1);
      if (l.kind == L_RES) {
        ResW& r = u.res[i];
        r.cin = l.a; r.cout = l.b; r.groups = 32; r.has_skip = l.a != l.b;
        r.conv1 = model_conv(m, n + ".layer2");
        r.conv2 = model_conv(m, n + ".layer5");
        if (r.has_skip) r.skip = model_conv(m, n + ".layer6");
        r.time = model_lin(m, n + ".layer3", true);
        r.time_off = toff;
        if (first) { u.tproj = r.time; first = false; }
        toff += l.b;
        r.gn1 = aff(n + ".layer1"); r.gn2 = aff(n + ".layer4");
      } else if (l.kind == L_ATTN) {
        AttnW& a = u.attn[i];
        a.n_head = l.a; a.n_embed = l.b; a.C = l.a * l.b;
        a.conv_in = model_conv(m, n + ".layer2");
        a.sa_in = model_lin(m, n + ".layer4.in_proj", false);
        a.sa_out = model_lin(m, n + ".layer4.out_proj", true);
        a.ca_q = model_lin(m, n + ".layer6.q_proj", false);
        a.ca_k = model_lin(m, n + ".layer6.k_proj", false);
        a.ca_v = model_lin(m, n + ".layer6.v_proj", false);
        a.d_ctx = a.ca_k.K;
        a.ca_out = model_lin(m, n + ".layer6.out_proj", true);
        a.geglu1 = model_lin(m, n + ".layer8", true);
        a.geglu2 = model_lin(m, n + ".layer9", true);
        a.conv_out = model_conv(m, n + ".layer10");
        a.kv_off = kvoff;
        if (kvoff == 0) { u.kproj_all = a.ca_k; u.vproj_all = a.ca_v; }
        kvoff += a.C;
        a.gelu_erf = torch_norms;
        a.gn = aff(n + ".layer1"); a.ln[0] = aff(n + ".layer3"); a.ln[1] = aff(n + ".layer5"); a.ln[2] = aff(n + ".layer7");
      } else if (full && (l.kind == L_CONV || l.kind == L_UPCONV)) {
        u.conv[i] = model_conv(m, n);
      }
    }
    u.tproj.N = toff;  // the layer3 weights of all residual blocks are contiguous in the blob (6720 rows; 20160 full-size)
    u.kproj_all.N = kvoff; u.vproj_all.N = kvoff;  // 6720 rows each (12480 full-size)
    if (!full) {
      u.conv1 = model_conv(m, "unet.layer1");
      u.conv4 = model_conv(m, "unet.layer4");
      u.conv7 = model_conv(m, "unet.layer7");
    }
    if (cn) {  // no output layer; the hint encoder and the zero convolutions instead
      for (int i = 0; i < CN_HINT_N; i++) u.hint[i] = model_conv(m, "hint.conv" + std::to_string(i + 1));
      u.zero.clear();
      for (int i = 0, k = 0; i < SD15_ENC_N; i++)
        if (SD15_STEPS[i].flags & U_PUSH) u.zero.push_back(model_conv(m, "zero.skip" + std::to_string(++k)));
      u.zero_mid = model_conv(m, "zero.mid");
      return TSD_OK;
    }
    u.final_conv = model_conv(m, "final.layer2");
    u.final_gn = aff("final.layer1");
    u.final_groups = torch_norms ? 32 : 320;
  } else if (is_clip_kind(m->kind)) {
    ClipW& c = m->clip;
    auto aff = [&](const std::string& name) {
      NormAffine a;
      if (is_torch_clip_kind(m->kind)) {
        a.w = (const float*)(m->blob + m->params[m->index.at(name + ".weight")].off);
        a.b = (const float*)(m->blob + m->params[m->index.at(name + ".bias")].off);
        a.torch_rstd = 1;
      }
      return a;
    };
    c.final_ln = aff("layernorm");
    c.tok = (const half_t*)(m->blob + m->params[m->index.at("embedding.token.weight")].off);
    c.pos = (const float*)(m->blob + m->params[m->index.at("embedding.position")].off);
    c.D = clip_kind_width(m->kind); c.H = c.D / 64; c.n_layer = clip_kind_layers(m->kind);
    c.gelu_erf = m->kind == TSD_MODEL_CLIP_SD2;
    for (int i = 0; i < c.n_layer; i++) {
      const std::string n = "player" + std::to_string(i + 1);
      c.layer[i].in_proj = model_lin(m, n + ".layer2.in_proj", true);
      c.layer[i].out_proj = model_lin(m, n + ".layer2.out_proj", true);
      c.layer[i].l4 = model_lin(m, n + ".layer4", true);
      c.layer[i].l5 = model_lin(m, n + ".layer5", true);
      c.layer[i].ln1 = aff(n + ".layer1");
      c.layer[i].ln2 = aff(n + ".layer3");
    }
  } else {
    const LayerDef* L = is_decoder_kind(m->kind) ? DECODER_LAYERS : ENCODER_LAYERS;
    const int n_layers = is_decoder_kind(m->kind) ? 26 : 19;
    const bool torch_norms = is_vae_torch_kind(m->kind);
    auto aff = [&](const std::string& name) {
      NormAffine a;
      if (torch_norms) {
        a.w = (const float*)(m->blob + m->params[m->index.at(name + ".weight")].off);
        a.b = (const float*)(m->blob + m->params[m->index.at(name + ".bias")].off);
        a.torch_rstd = 1;
      }
      return a;
    };
    VaeW& v = m->vae;
    v.gn_eps = torch_norms ? 1e-6f : 1e-5f;
    v.gn.assign(n_layers, NormAffine());
    v.conv.assign(n_layers, ConvW());
    v.res.assign(n_layers, ResW());
    v.attn.assign(n_layers, VaeAttnW());
    for (int i = 0; i < n_layers; i++) {
      const LayerDef& l = L[i];
      const std::string n = "l" + std::to_string(i + 1);
      if (l.kind == L_CONV || l.kind == L_CONV_S2) v.conv[i] = model_conv(m, n);
      else if (l.kind == L_RES) {
        ResW& r = v.res[i];
        r.cin = l.a; r.cout = l.b; r.has_skip = l.a != l.b;
        r.groups = torch_norms ? 32 : 16;  // GroupNorm(16), vae.mojo:42-43 ; the trained VAE has 32
        r.eps = torch_norms ? 1e-6f : 1e-5f;
        r.gn1 = aff(n + ".group_norm1"); r.gn2 = aff(n + ".group_norm2");
        r.conv1 = model_conv(m, n + ".conv1");
        r.conv2 = model_conv(m, n + ".conv2");
        if (r.has_skip) r.skip = model_conv(m, n + ".res_conv_layer");
      } else if (l.kind == L_ATTN) {
        v.attn[i].C = l.a;
        v.attn[i].in_proj = model_lin(m, n + ".attention.in_proj", true);
        v.attn[i].out_proj = model_lin(m, n + ".attention.out_proj", true);
        v.attn[i].gn = aff(n + ".group_norm");
        v.attn[i].eps = torch_norms ? 1e-6f : 1e-5f;
      } else if (l.kind == L_GN) {
        v.gn[i] = aff(n);
      }
    }
  }
  return TSD_OK;
}
