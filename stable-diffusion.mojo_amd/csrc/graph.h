// graph.h - host-side graph of the hot path: block and module forwards enqueue kernels on the
// context stream; activations live in the workspace arena as NHWC fp16.
#pragma once
#include "model.h"

// how the C-ABI entry points (api_ops.cpp, api_model.cpp, session.cpp, api_replay.cpp) refuse a NULL pointer argument
#define NOTNULL(p) \
  if (!(p)) TSD_FAIL(TSD_E_ARG, "%s: argument '%s' is NULL", __func__, #p)
// A context option set for a scope (one replayed launch, one bench entry): the previous value is back when the scope ends, on every
// path out of it - an early HIP_TRY / TSD_TRY return must not leave later launches of the context pinned
template <class T>
struct Override {
  T& ref;
  const T prev;
  Override(T& r, T now) : ref(r), prev(r) { ref = now; }
  ~Override() { ref = prev; }
};

// channel-concat view of up to two NHWC tensors with identical (B,H,W) (diffusion.mojo:253-270)
struct CatSrc {
  const half_t* p0 = nullptr; int ld0 = 0; int C0 = 0;
  const half_t* p1 = nullptr; int ld1 = 0; int C1 = 0;
  const float* gn_part0 = nullptr; int gn_nslab0 = 0, gn_groups0 = 0;  // producer-emitted GroupNorm statistics of p0
  const float* gn_part1 = nullptr; int gn_nslab1 = 0, gn_groups1 = 0;  // ... and of p1
};
static inline CatSrc cat1(const Act& a) {
  CatSrc c; c.p0 = a.p; c.ld0 = a.ld; c.C0 = a.C;
  c.gn_part0 = a.gn_part; c.gn_nslab0 = a.gn_nslab; c.gn_groups0 = a.gn_groups;
  return c;
}
// Groups to emit statistics for on a C0-channel tensor whose consumer is GroupNorm(groups) over concat(it, a C1-channel skip whose
// own statistics come in C1 / groups-channel groups): the skip's granularity when the concat's groups are whole multiples of it
// (1280 + 640 -> 60-channel groups = 3 x 20: emit 64 groups of 20), else `groups`
static inline int concat_stat_groups(int C0, int C1, int groups) {
  if (C1 <= 0 || C1 % groups || (C0 + C1) % groups) return groups;
  const int cf = C1 / groups, cpg = (C0 + C1) / groups;
  return (cpg % cf == 0 && C0 % cf == 0 && C0 / cf <= 256) ? C0 / cf : groups;
}
// activation whose producer may emit the statistics of the GroupNorm(groups) that will consume it
Act act_alloc_gn(tsd_ctx* ctx, int B, int H, int W, int C, int groups);
static inline CatSrc cat2(const Act& a, const Act& b) {
  CatSrc c = cat1(a); c.p1 = b.p; c.ld1 = b.ld; c.C1 = b.C;
  c.gn_part1 = b.gn_part; c.gn_nslab1 = b.gn_nslab; c.gn_groups1 = b.gn_groups;
  return c;
}

// y = conv3x3(x) (+bias) (+rowvec per sample) (+residual); `ups`: x is read through a nearest-2x upsample.
int g_conv3x3(tsd_ctx* ctx, const Act& x, const ConvW& w, int stride, int pad, int pad_br, int ups,
              const float* rowvec, int rowvec_ld, const Act* res, int res_ups, bool out_f32, void* y, int ldy,
              Act* stat = nullptr,  // stat: the output tensor's Act when GroupNorm statistics are wanted
              const CatSrc* skip_x = nullptr, const ConvW* skip_w = nullptr);  // + conv1x1(skip_x) fused as extra K (same resolution)
// y[M][N] = A[M][K] . W^T (+bias) (+residual) ; A may be a concat view
int g_linear(tsd_ctx* ctx, const CatSrc& a, int64_t M, const half_t* w, int ldw, int N, int K, const float* bias,
             const half_t* res, int ldr, int epi_extra, void* y, int ldy, Act* stat = nullptr, int rows_per_sample = 0,
             const half_t* w_tm = nullptr);  // w_tm: K-tile-major copy of w ([K/64][N][64]) - used instead when given

int g_resblock(tsd_ctx* ctx, const CatSrc& x, int B, int Hin, int Win, int ups, const ResW& w, const float* tvec,
               int tld, Act& out);
struct CtxKV {  // projected context keys (token-major) and values (channel-major) of one attention block
  const half_t* K = nullptr; int ldk = 0; int64_t sK = 0;
  const half_t* Vt = nullptr; int ldvt = 0; int64_t sVt = 0;
};
// IP-Adapter: one block's projected image tokens - K_ip token-major [b][16][.], V_ip^T channel-major [b][C][16], N <= 16 of them live - and
// the per-sample scales, a device fp32 [B].  Present, the block runs op by op (also where the fused head / tail kernels would apply) and
// launch_ip_attn_add runs between the cross-attention core and out_proj.
struct IpKV {
  const half_t* K = nullptr; int ldk = 0; int64_t sK = 0;
  const half_t* Vt = nullptr; int ldvt = 0; int64_t sVt = 0;
  int N = 0;
  const float* scale = nullptr;
};
int g_unet_attn(tsd_ctx* ctx, const Act& x, const AttnW& w, const half_t* ctx16, int T, int Tp, Act& out,
                const CtxKV* pre = nullptr, const IpKV* ipkv = nullptr);
int g_vae_attn(tsd_ctx* ctx, const Act& x, const VaeAttnW& w, Act& out);
int g_attn_core(tsd_ctx* ctx, const AttnArgs& fa);
int g_qkv_proj(tsd_ctx* ctx, const half_t* x, int B, int S, int C, const LinW& in_proj, half_t* qk, half_t* vt, int Sp);

// module forwards on device buffers
// latents: fp32 CHW [B,4,LH,LW]; context16: fp16 [B][Tp][W], W = model_context_width(m) (768; 1024 for the SD-2.x UNet); temb: fp32 [B][320]; eps_out: fp32 CHW [B,4,LH,LW]
// eps_nhwc: eps_out receives the output convolution's own layout, fp32 [B][LH*LW][4], instead of CHW (the denoise session's DDPM update
// reads it directly: one conversion launch per step less)
// pre: what the forward computes from the timestep and the context alone, made ahead by the caller (the denoise session keeps both
// across the steps of an upload()).  Absent, the forward launches the two helpers below itself; present, it launches nothing for them
// and reads neither `temb` nor, for the K / V^T projections, `ctx16`.
struct UNetPre {
  const float* tvec = nullptr; int tld = 0;  // time projections of all residual blocks [.][tproj.N]; tld: per-sample stride (0 = one row for all)
  const half_t* kc_all = nullptr;            // context K of all attention blocks [B*Tp][CK], CK = kproj_all.N
  const half_t* vtc_all = nullptr;           // context V^T [B][CK][Tp]
};
// control: the 13 residuals of a ControlNet forward on the SAME context (fp16 NHWC in its arena: the twelve skips in push order, then the
// bottleneck output), added to the full-size UNet's skips and bottleneck output scaled by control_scale, a device fp32 [B] - one launch
// between the bottleneck and the first decoder step.  Absent, the forward enqueues what it always did.  The Tiny-SD graph refuses it.
struct ControlRes { Act r[CONTROL_RESIDUALS]; };
struct IpRun;
int g_unet_forward(tsd_model* m, const float* latents_chw, const half_t* ctx16, int T, int Tp, const float* temb, int B,
                   int LH, int LW, float* eps_out_chw, bool eps_nhwc = false, const UNetPre* pre = nullptr,
                   const ControlRes* control = nullptr, const float* control_scale = nullptr, const IpRun* ip = nullptr);
// IP-Adapter (kind 20) on the full-size SD-1.x UNet (kinds 5 / 6; everything else refuses it): the adapter's projected tokens of all 16
// blocks, k_all [B*16][CK] and vt_all [B][CK][16] (CK = 12480, the adapter's own packing: IpAdapterW::kv_off), N live tokens, scale a
// device fp32 [B].  Absent, the forward enqueues what it always did.
struct IpRun {
  const tsd_model* ip = nullptr;
  const half_t* k_all = nullptr; const half_t* vt_all = nullptr;
  int N = 0;
  const float* scale = nullptr;
};
// tokens fp32 [B][N][768] (device) -> tok16 fp16 [B][16][768], rows N .. 15 zero (the pad keys must be finite)
int g_ip_stage_tokens(tsd_ctx* ctx, const float* tokens, int B, int N, half_t* tok16);
// K_ip / V_ip^T of all blocks from the staged tokens: g_unet_ctx_kv's GEMMs with Tp = 16 on the adapter's tables
int g_ip_kv(tsd_model* ip, const half_t* tok16, int B, half_t* k_all, half_t* vt_all);
// image_proj: embeds fp32 [B][1024] (device) -> tokens fp32 [B][n_tokens][768] (device) = LayerNorm(Linear(e)), every value an fp16
int g_ip_project(tsd_model* ip, const float* embeds, int B, float* tokens_out);
// kind 24's image_proj, the Perceiver resampler: hidden fp32 [B][S][1280] (device; the vision encoder's hidden_out at S = 257) -> tokens
// fp32 [B][16][768] (device), every value an fp16.  1 <= B <= 16, 1 <= S <= 1024.  One arena mark / release, no allocation, no synchronisation.
int g_ip_resample(tsd_model* ip, const float* hidden, int B, int S, float* tokens_out);
// ControlNet (kinds 10 / 11).  hint_chw: device fp32 [B,3,8LH,8LW] -> hint features fp16 NHWC [B,LH,LW,320] in the arena
int g_controlnet_hint(tsd_model* m, const float* hint_chw, int B, int LH, int LW, Act* out);
// pre: a UNetPre made from the ControlNet's OWN weights (g_unet_time_path / g_unet_ctx_kv on `m`), or nullptr
int g_controlnet_forward(tsd_model* m, const float* latents_chw, const half_t* ctx16, int T, int Tp, const float* temb, const Act& hint_feat,
                         int B, int LH, int LW, const UNetPre* pre, ControlRes* out);
int g_unet_time_path(tsd_model* m, const float* temb, int B, const float** tvec_out);  // -> tvec [B][tproj.N] in the arena
int g_unet_ctx_kv(tsd_model* m, const half_t* ctx16, int Tp, int B, half_t* kc_all, half_t* vtc_all);
int g_decoder_forward(tsd_model* m, const float* latents_chw, int B, int LH, int LW, float* images_chw);
int g_encoder_forward(tsd_model* m, const float* images_chw, const float* noise_chw, int B, int SH, int SW, float* latents_chw);

// run `fn` once in planning mode to size the arena, reserve it, then for real
template <class F>
int run_planned(tsd_ctx* ctx, F&& fn) {
  Arena& a = ctx->arena;
  a.planning = true; a.top = 0; a.peak = 0;
  int r = fn();
  a.planning = false;
  const size_t need = a.peak;
  a.top = 0; a.peak = 0;
  if (r != TSD_OK) return r;
  TSD_TRY(ctx_reserve_arena(ctx, need));
  r = fn();
  a.top = 0;
  return r;
}
// tokens: device int32 [B][77]; out: device fp32 [B][77][D], D = the encoder's width (768; 1024 for TSD_MODEL_CLIP_SD2)
int g_clip_forward(tsd_model* m, const int* tokens_dev, int B, float* out_f32);
// CLIP vision encoder (kind 22).  images: device fp32 [B][3][H][W] on 0 .. 255; embeds_out: device fp32 [B][1024]; hidden_out: device fp32
// [B][257][1280], the input of the last layer, or nullptr (one conversion launch less; embeds_out holds the same bits either way)
int g_clip_vision_forward(tsd_model* m, const float* images, int B, int H, int W, float* embeds_out, float* hidden_out);
