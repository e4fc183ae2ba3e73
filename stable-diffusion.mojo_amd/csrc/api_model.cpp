// api_model.cpp - module-level forwards (device-resident weights) and the RCCL weight broadcast.  The device-resident denoise
// session that runs the forwards step after step is session.cpp.
#include <dlfcn.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "graph.h"

// Every entry point opens with NOTNULL(p) on its pointer arguments (graph.h): TSD_E_ARG and the argument's name in
// tsd_last_error.

namespace {
int h2d(tsd_ctx* c, void* dst, const void* src, size_t bytes) {
  if (c->launch()) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  return TSD_OK;
}
int d2h(tsd_ctx* c, void* dst, const void* src, size_t bytes) {
  if (c->launch()) HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  return TSD_OK;
}
template <class F>
int run_model(tsd_model* m, F&& fn) {
  tsd_ctx* ctx = m->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(model_check_ready(m));
  int r = run_planned(ctx, fn);
  hipError_t e = hipStreamSynchronize(ctx->stream);
  if (r != TSD_OK) return r;
  if (e != hipSuccess) TSD_FAIL(TSD_E_HIP, "stream synchronize failed: %s", hipGetErrorString(e));
  return ctx_check_status(ctx);
}
}  // namespace

// The square entries are the LH == LW == L case of the *_hw entries below them: one body each.
extern "C" int tsd_diffusion_forward_hw(tsd_model* m, const float* latents, const float* context, const float* time_emb,
                                        int B, int LH, int LW, int T, float* out) {
  NOTNULL(m); NOTNULL(latents); NOTNULL(context); NOTNULL(time_emb); NOTNULL(out);
  if (!is_diffusion_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "tsd_diffusion_forward: model is not a Diffusion");
  if (B <= 0 || B > 16 || LH <= 0 || LW <= 0 || T <= 0) TSD_FAIL(TSD_E_SHAPE, "diffusion: B=%d (1..16) L=%dx%d T=%d", B, LH, LW, T);
  const int mult = is_full_unet_kind(m->kind) ? 16 : 8;  // the graph's own rule (graph.cpp), refused here before anything is planned
  if (LH % mult || LW % mult) TSD_FAIL(TSD_E_SHAPE, "diffusion: latent sides %d x %d must be multiples of %d", LH, LW, mult);
  tsd_ctx* ctx = m->ctx;
  const int W = model_context_width(m);  // 768, or 1024 for the SD-2.x UNet
  return run_model(m, [&]() -> int {
    const int Tp = round_up(T, 8);
    const int64_t nl = (int64_t)B * 4 * LH * LW;
    float* dl = arena_alloc<float>(ctx, nl);
    float* dc = arena_alloc<float>(ctx, (int64_t)B * T * W);
    float* dt = arena_alloc<float>(ctx, (int64_t)B * 320);
    half_t* c16 = arena_alloc<half_t>(ctx, (int64_t)B * Tp * W);
    float* de = arena_alloc<float>(ctx, nl);
    if (!dl || !dc || !dt || !c16 || !de) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, dl, latents, nl * 4));
    TSD_TRY(h2d(ctx, dc, context, (size_t)B * T * W * 4));
    TSD_TRY(h2d(ctx, dt, time_emb, (size_t)B * 320 * 4));
    for (int b = 0; b < B; b++)  // [T][W] -> zero-padded [Tp][W] per sample
      TSD_TRY(launch_f32_to_f16_rows(ctx, dc + (int64_t)b * T * W, T, W, c16 + (int64_t)b * Tp * W, W, Tp));
    TSD_TRY(g_unet_forward(m, dl, c16, T, Tp, dt, B, LH, LW, de));
    return d2h(ctx, out, de, nl * 4);
  });
}
extern "C" int tsd_diffusion_forward(tsd_model* m, const float* latents, const float* context, const float* time_emb,
                                     int B, int L, int T, float* out) {
  return tsd_diffusion_forward_hw(m, latents, context, time_emb, B, L, L, T, out);
}

// ---- ControlNet: the residuals alone, and the controlled UNet forward (both models on one context, one plan) --------------------------
namespace {
struct CnInputs {
  float* dl = nullptr; float* dt = nullptr; half_t* c16 = nullptr; float* dh = nullptr;
  int Tp = 0;
};
int cn_check(const tsd_model* cn, int B, int LH, int LW, int T) {
  if (!is_controlnet_kind(cn->kind)) TSD_FAIL(TSD_E_ARG, "controlnet: model is not a ControlNet");
  if (B <= 0 || B > 16 || LH <= 0 || LW <= 0 || T <= 0) TSD_FAIL(TSD_E_SHAPE, "controlnet: B=%d (1..16) L=%dx%d T=%d", B, LH, LW, T);
  if (LH % 16 || LW % 16) TSD_FAIL(TSD_E_SHAPE, "controlnet: latent sides %d x %d must be multiples of 16", LH, LW);
  return TSD_OK;
}
// latents, context (converted to padded fp16 rows), time embedding and hint onto the device
int cn_upload(tsd_ctx* ctx, const float* latents, const float* context, const float* time_emb, const float* hint, int B, int LH, int LW, int T,
              int W, CnInputs* in) {  // W: the context width of the models that read it
  const int Tp = round_up(T, 8);
  const int64_t nl = (int64_t)B * 4 * LH * LW, nh = (int64_t)B * 3 * 64 * LH * LW;
  in->Tp = Tp;
  in->dl = arena_alloc<float>(ctx, nl);
  float* dc = arena_alloc<float>(ctx, (int64_t)B * T * W);
  in->dt = arena_alloc<float>(ctx, (int64_t)B * 320);
  in->c16 = arena_alloc<half_t>(ctx, (int64_t)B * Tp * W);
  in->dh = hint ? arena_alloc<float>(ctx, nh) : nullptr;  // hint == NULL: a forward without a ControlNet (the adapted entry)
  if (!in->dl || !dc || !in->dt || !in->c16 || (hint && !in->dh)) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
  TSD_TRY(h2d(ctx, in->dl, latents, nl * 4));
  TSD_TRY(h2d(ctx, dc, context, (size_t)B * T * W * 4));
  TSD_TRY(h2d(ctx, in->dt, time_emb, (size_t)B * 320 * 4));
  if (hint) TSD_TRY(h2d(ctx, in->dh, hint, nh * 4));
  for (int b = 0; b < B; b++)  // [T][W] -> zero-padded [Tp][W] per sample
    TSD_TRY(launch_f32_to_f16_rows(ctx, dc + (int64_t)b * T * W, T, W, in->c16 + (int64_t)b * Tp * W, W, Tp));
  return TSD_OK;
}
}  // namespace

extern "C" int tsd_controlnet_forward_hw(tsd_model* cn, const float* latents, const float* context, const float* time_emb, const float* hint,
                                         int B, int LH, int LW, int T, float* const* residuals_out) {
  NOTNULL(cn); NOTNULL(latents); NOTNULL(context); NOTNULL(time_emb); NOTNULL(hint); NOTNULL(residuals_out);
  for (int k = 0; k < CONTROL_RESIDUALS; k++)
    if (!residuals_out[k]) TSD_FAIL(TSD_E_ARG, "tsd_controlnet_forward_hw: residuals_out[%d] is NULL", k);
  TSD_TRY(cn_check(cn, B, LH, LW, T));
  tsd_ctx* ctx = cn->ctx;
  return run_model(cn, [&]() -> int {
    CnInputs in;
    TSD_TRY(cn_upload(ctx, latents, context, time_emb, hint, B, LH, LW, T, model_context_width(cn), &in));
    Act hf;
    TSD_TRY(g_controlnet_hint(cn, in.dh, B, LH, LW, &hf));
    ControlRes res;
    TSD_TRY(g_controlnet_forward(cn, in.dl, in.c16, T, in.Tp, in.dt, hf, B, LH, LW, nullptr, &res));
    for (int k = 0; k < CONTROL_RESIDUALS; k++) {
      const Act& r = res.r[k];
      const int64_t n = r.pixels() * r.C;
      float* d = arena_alloc<float>(ctx, n);
      if (!d) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
      TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, r.p, B, r.C, r.H, r.W, r.ld, d));
      TSD_TRY(d2h(ctx, residuals_out[k], d, n * 4));
    }
    return TSD_OK;
  });
}

// the hint encoder alone: hint [B,3,8LH,8LW] -> features fp32 CHW [B,320,LH,LW] (what a session keeps across its steps)
extern "C" int tsd_controlnet_hint_hw(tsd_model* cn, const float* hint, int B, int LH, int LW, float* features_out) {
  NOTNULL(cn); NOTNULL(hint); NOTNULL(features_out);
  TSD_TRY(cn_check(cn, B, LH, LW, 1));
  tsd_ctx* ctx = cn->ctx;
  return run_model(cn, [&]() -> int {
    const int64_t nh = (int64_t)B * 3 * 64 * LH * LW, nf = (int64_t)B * 320 * LH * LW;
    float* dh = arena_alloc<float>(ctx, nh);
    float* df = arena_alloc<float>(ctx, nf);
    if (!dh || !df) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, dh, hint, nh * 4));
    Act hf;
    TSD_TRY(g_controlnet_hint(cn, dh, B, LH, LW, &hf));
    TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, hf.p, B, 320, LH, LW, hf.ld, df));
    return d2h(ctx, features_out, df, nf * 4);
  });
}

extern "C" int tsd_diffusion_forward_control_hw(tsd_model* unet, tsd_model* cn, const float* latents, const float* context,
                                                const float* time_emb, const float* hint, const float* scale, int B, int LH, int LW, int T,
                                                float* eps_out) {
  NOTNULL(unet); NOTNULL(cn); NOTNULL(latents); NOTNULL(context); NOTNULL(time_emb); NOTNULL(hint); NOTNULL(scale); NOTNULL(eps_out);
  if (!is_full_unet_kind(unet->kind)) TSD_FAIL(TSD_E_ARG, "controlled forward: the UNet must be a full-size kind (the Tiny-SD graph has no ControlNet)");
  TSD_TRY(cn_check(cn, B, LH, LW, T));
  if (model_context_width(unet) != model_context_width(cn))
    TSD_FAIL(TSD_E_ARG, "controlled forward: the ControlNet kinds are SD-1.x networks (context width %d); this UNet reads a %d-wide context",
             model_context_width(cn), model_context_width(unet));
  if (unet->ctx != cn->ctx) TSD_FAIL(TSD_E_ARG, "controlled forward: the UNet and the ControlNet belong to different contexts (the residuals live in one arena)");
  for (int b = 0; b < B; b++)
    if (!(fabsf(scale[b]) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "controlled forward: scale[%d] is not finite", b);
  tsd_ctx* ctx = unet->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(model_check_ready(cn));
  return run_model(unet, [&]() -> int {
    CnInputs in;
    TSD_TRY(cn_upload(ctx, latents, context, time_emb, hint, B, LH, LW, T, model_context_width(cn), &in));
    const int64_t nl = (int64_t)B * 4 * LH * LW;
    float* ds = arena_alloc<float>(ctx, B);
    float* de = arena_alloc<float>(ctx, nl);
    if (!ds || !de) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, ds, scale, (size_t)B * 4));
    Act hf;
    TSD_TRY(g_controlnet_hint(cn, in.dh, B, LH, LW, &hf));
    ControlRes res;
    TSD_TRY(g_controlnet_forward(cn, in.dl, in.c16, T, in.Tp, in.dt, hf, B, LH, LW, nullptr, &res));
    TSD_TRY(g_unet_forward(unet, in.dl, in.c16, T, in.Tp, in.dt, B, LH, LW, de, false, nullptr, &res, ds));
    return d2h(ctx, eps_out, de, nl * 4);
  });
}

// ---- IP-Adapter: the image projection alone, and the adapted UNet forward (with or without a ControlNet, all models on one context) ------
extern "C" int tsd_ip_adapter_project(tsd_model* ip, const float* embeds, int B, float* tokens_out) {
  NOTNULL(ip); NOTNULL(embeds); NOTNULL(tokens_out);
  if (!is_ip_adapter_kind(ip->kind)) TSD_FAIL(TSD_E_ARG, "tsd_ip_adapter_project: model is not an IP-Adapter");
  if (is_ip_plus_kind(ip->kind))
    TSD_FAIL(TSD_E_ARG, "tsd_ip_adapter_project: an IP-Adapter Plus reads the vision encoder's hidden states, not the image embedding: "
                        "call tsd_ip_adapter_resample");
  if (B <= 0 || B > 16) TSD_FAIL(TSD_E_SHAPE, "ip_adapter_project: B=%d (1..16)", B);
  tsd_ctx* ctx = ip->ctx;
  return run_model(ip, [&]() -> int {
    const int64_t ne = (int64_t)B * IP_EMBED_DIM, nt = (int64_t)B * ip->ip.n_tokens * IP_CTX_DIM;
    float* de = arena_alloc<float>(ctx, ne);
    float* dt = arena_alloc<float>(ctx, nt);
    if (!de || !dt) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, de, embeds, ne * 4));
    TSD_TRY(g_ip_project(ip, de, B, dt));
    return d2h(ctx, tokens_out, dt, nt * 4);
  });
}

// the "plus" adapter's image projection: the vision encoder's hidden states -> 16 tokens (graph.cpp g_ip_resample)
extern "C" int tsd_ip_adapter_resample(tsd_model* ip, const float* hidden, int B, int S, float* tokens_out) {
  NOTNULL(ip); NOTNULL(hidden); NOTNULL(tokens_out);
  if (!is_ip_adapter_kind(ip->kind)) TSD_FAIL(TSD_E_ARG, "tsd_ip_adapter_resample: model is not an IP-Adapter");
  if (!is_ip_plus_kind(ip->kind))
    TSD_FAIL(TSD_E_ARG, "tsd_ip_adapter_resample: this IP-Adapter has no resampler, it reads the 1024-wide image embedding: "
                        "call tsd_ip_adapter_project");
  if (B <= 0 || B > 16 || S <= 0 || S > IPP_MAX_S) TSD_FAIL(TSD_E_SHAPE, "ip_adapter_resample: B=%d (1..16) S=%d (1..%d)", B, S, IPP_MAX_S);
  tsd_ctx* ctx = ip->ctx;
  return run_model(ip, [&]() -> int {
    const int64_t nh = (int64_t)B * S * IPP_EMBED, nt = (int64_t)B * IPP_TOKENS * IP_CTX_DIM;
    float* dh = arena_alloc<float>(ctx, nh);
    float* dt = arena_alloc<float>(ctx, nt);
    if (!dh || !dt) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, dh, hidden, (size_t)nh * 4));
    TSD_TRY(g_ip_resample(ip, dh, B, S, dt));
    return d2h(ctx, tokens_out, dt, (size_t)nt * 4);
  });
}

extern "C" int tsd_diffusion_forward_ip_hw(tsd_model* unet, tsd_model* ip, const float* tokens, int N, const float* ip_scale, tsd_model* cn,
                                           const float* hint, const float* control_scale, const float* latents, const float* context,
                                           const float* time_emb, int B, int LH, int LW, int T, float* eps_out) {
  NOTNULL(unet);
  if (!ip)  // no adapter: the plain or the controlled entry, launch for launch
    return cn ? tsd_diffusion_forward_control_hw(unet, cn, latents, context, time_emb, hint, control_scale, B, LH, LW, T, eps_out)
              : tsd_diffusion_forward_hw(unet, latents, context, time_emb, B, LH, LW, T, eps_out);
  NOTNULL(tokens); NOTNULL(ip_scale); NOTNULL(latents); NOTNULL(context); NOTNULL(time_emb); NOTNULL(eps_out);
  if (unet->kind != TSD_MODEL_DIFFUSION_SD15 && unet->kind != TSD_MODEL_DIFFUSION_SD15_TORCH)
    TSD_FAIL(TSD_E_ARG, "adapted forward: the UNet must be a full-size SD-1.x kind (an IP-Adapter of this kind fits no other graph)");
  if (!is_ip_adapter_kind(ip->kind)) TSD_FAIL(TSD_E_ARG, "adapted forward: the model is not an IP-Adapter");
  if (ip->ctx != unet->ctx) TSD_FAIL(TSD_E_ARG, "adapted forward: the UNet and the IP-Adapter belong to different contexts");
  if (N < 1 || N > IP_MAX_TOKENS) TSD_FAIL(TSD_E_ARG, "adapted forward: %d image tokens (1..%d)", N, IP_MAX_TOKENS);
  if (B <= 0 || B > 16 || LH <= 0 || LW <= 0 || T <= 0) TSD_FAIL(TSD_E_SHAPE, "diffusion: B=%d (1..16) L=%dx%d T=%d", B, LH, LW, T);
  if (LH % 16 || LW % 16) TSD_FAIL(TSD_E_SHAPE, "diffusion: latent sides %d x %d must be multiples of 16", LH, LW);
  for (int b = 0; b < B; b++)
    if (!(fabsf(ip_scale[b]) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "adapted forward: ip_scale[%d] is not finite", b);
  if (cn) {
    NOTNULL(hint); NOTNULL(control_scale);
    TSD_TRY(cn_check(cn, B, LH, LW, T));
    if (unet->ctx != cn->ctx) TSD_FAIL(TSD_E_ARG, "adapted forward: the UNet and the ControlNet belong to different contexts");
    for (int b = 0; b < B; b++)
      if (!(fabsf(control_scale[b]) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "adapted forward: control_scale[%d] is not finite", b);
  }
  // every sample at scale 0: the adapter adds nothing to any sample, so the forward is the plain (or the controlled) one, launch for
  // launch - the attention blocks keep their fused kernels and the result is that entry's, bit for bit
  bool any = false;
  for (int b = 0; b < B; b++) any = any || ip_scale[b] != 0.f;
  if (!any)
    return cn ? tsd_diffusion_forward_control_hw(unet, cn, latents, context, time_emb, hint, control_scale, B, LH, LW, T, eps_out)
              : tsd_diffusion_forward_hw(unet, latents, context, time_emb, B, LH, LW, T, eps_out);
  tsd_ctx* ctx = unet->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(model_check_ready(ip));
  if (cn) TSD_TRY(model_check_ready(cn));
  return run_model(unet, [&]() -> int {
    CnInputs in;
    TSD_TRY(cn_upload(ctx, latents, context, time_emb, cn ? hint : nullptr, B, LH, LW, T, model_context_width(unet), &in));
    const int64_t nl = (int64_t)B * 4 * LH * LW, ntok = (int64_t)B * N * IP_CTX_DIM, IK = ip->unet.kproj_all.N;
    float* ds = arena_alloc<float>(ctx, 2 * B);  // ip_scale | control_scale
    float* de = arena_alloc<float>(ctx, nl);
    float* dtok = arena_alloc<float>(ctx, ntok);
    half_t* tok16 = arena_alloc<half_t>(ctx, (int64_t)B * IP_MAX_TOKENS * IP_CTX_DIM);
    half_t* kip = arena_alloc<half_t>(ctx, (int64_t)B * IP_MAX_TOKENS * IK);
    half_t* vip = arena_alloc<half_t>(ctx, (int64_t)B * IK * IP_MAX_TOKENS);
    if (!ds || !de || !dtok || !tok16 || !kip || !vip) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, ds, ip_scale, (size_t)B * 4));
    if (cn) TSD_TRY(h2d(ctx, ds + B, control_scale, (size_t)B * 4));
    TSD_TRY(h2d(ctx, dtok, tokens, (size_t)ntok * 4));
    TSD_TRY(g_ip_stage_tokens(ctx, dtok, B, N, tok16));
    TSD_TRY(g_ip_kv(ip, tok16, B, kip, vip));
    IpRun run;
    run.ip = ip; run.k_all = kip; run.vt_all = vip; run.N = N; run.scale = ds;
    ControlRes res;
    if (cn) {
      Act hf;
      TSD_TRY(g_controlnet_hint(cn, in.dh, B, LH, LW, &hf));
      TSD_TRY(g_controlnet_forward(cn, in.dl, in.c16, T, in.Tp, in.dt, hf, B, LH, LW, nullptr, &res));
    }
    TSD_TRY(g_unet_forward(unet, in.dl, in.c16, T, in.Tp, in.dt, B, LH, LW, de, false, nullptr, cn ? &res : nullptr, cn ? ds + B : nullptr, &run));
    return d2h(ctx, eps_out, de, nl * 4);
  });
}

// FreeU: the model's table.  Nothing on the device changes here: unet_full_steps reads the table when a forward is enqueued, and the
// workspace a forward needs is the same with and without it (graph.cpp), so an open session's next step just runs the new graph.
extern "C" int tsd_model_set_freeu(tsd_model* unet, const float* b, const float* s, int mode) {
  NOTNULL(unet);
  if (!is_full_unet_kind(unet->kind)) TSD_FAIL(TSD_E_ARG, "tsd_model_set_freeu: FreeU belongs to the full-size UNets (kinds 5, 6, 16), this model is kind %d", unet->kind);
  if (!b != !s) TSD_FAIL(TSD_E_ARG, "tsd_model_set_freeu: b and s are given together (both NULL turns FreeU off)");
  if (mode != TSD_FREEU_CONSTANT && mode != TSD_FREEU_MODULATED) TSD_FAIL(TSD_E_ARG, "tsd_model_set_freeu: mode %d (0 constant, 1 modulated)", mode);
  bool on = false;
  for (int j = 0; b && j < TSD_FREEU_BLOCKS; j++) {
    if (!isfinite(b[j]) || !isfinite(s[j])) TSD_FAIL(TSD_E_ARG, "tsd_model_set_freeu: block %d: b = %g, s = %g must be finite", j, (double)b[j], (double)s[j]);
    on |= b[j] != 1.f || s[j] != 1.f;
  }
  for (int j = 0; j < TSD_FREEU_BLOCKS; j++) {
    unet->freeu_b[j] = on ? b[j] : 1.f;
    unet->freeu_s[j] = on ? s[j] : 1.f;
  }
  unet->freeu_on = on;
  unet->freeu_mode = on ? mode : TSD_FREEU_CONSTANT;
  return TSD_OK;
}
extern "C" int tsd_model_freeu(tsd_model* unet, float* b, float* s, int* mode) {
  NOTNULL(unet);
  if (!is_full_unet_kind(unet->kind)) TSD_FAIL(TSD_E_ARG, "tsd_model_freeu: FreeU belongs to the full-size UNets (kinds 5, 6, 16), this model is kind %d", unet->kind);
  for (int j = 0; j < TSD_FREEU_BLOCKS; j++) {
    if (b) b[j] = unet->freeu_b[j];
    if (s) s[j] = unet->freeu_s[j];
  }
  if (mode) *mode = unet->freeu_mode;
  return unet->freeu_on ? 1 : 0;
}

extern "C" int tsd_decoder_forward_hw(tsd_model* m, const float* latents, int B, int LH, int LW, float* images) {
  NOTNULL(m); NOTNULL(latents); NOTNULL(images);
  if (!is_decoder_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "tsd_decoder_forward: model is not a Decoder");
  if (B <= 0 || LH <= 0 || LW <= 0 || LH % 8 || LW % 8) TSD_FAIL(TSD_E_SHAPE, "decoder: B=%d L=%dx%d (multiples of 8)", B, LH, LW);
  tsd_ctx* ctx = m->ctx;
  return run_model(m, [&]() -> int {
    const int64_t nl = (int64_t)B * 4 * LH * LW, ni = (int64_t)B * 3 * 64 * LH * LW;
    float* dl = arena_alloc<float>(ctx, nl);
    float* di = arena_alloc<float>(ctx, ni);
    if (!dl || !di) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, dl, latents, nl * 4));
    TSD_TRY(g_decoder_forward(m, dl, B, LH, LW, di));
    return d2h(ctx, images, di, ni * 4);
  });
}
extern "C" int tsd_decoder_forward(tsd_model* m, const float* latents, int B, int L, float* images) {
  return tsd_decoder_forward_hw(m, latents, B, L, L, images);
}

extern "C" int tsd_encoder_forward_hw(tsd_model* m, const float* images, const float* noise, int B, int SH, int SW,
                                      float* latents) {
  NOTNULL(m); NOTNULL(images); NOTNULL(noise); NOTNULL(latents);
  if (!is_encoder_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "tsd_encoder_forward: model is not an Encoder");
  if (B <= 0 || SH <= 0 || SW <= 0 || SH % 64 || SW % 64) TSD_FAIL(TSD_E_SHAPE, "encoder: B=%d S=%dx%d (multiples of 64)", B, SH, SW);
  tsd_ctx* ctx = m->ctx;
  return run_model(m, [&]() -> int {
    const int64_t ni = (int64_t)B * 3 * SH * SW, nl = (int64_t)B * 4 * (SH / 8) * (SW / 8);
    float* di = arena_alloc<float>(ctx, ni);
    float* dn = arena_alloc<float>(ctx, nl);
    float* dl = arena_alloc<float>(ctx, nl);
    if (!di || !dn || !dl) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, di, images, ni * 4));
    TSD_TRY(h2d(ctx, dn, noise, nl * 4));
    TSD_TRY(g_encoder_forward(m, di, dn, B, SH, SW, dl));
    return d2h(ctx, latents, dl, nl * 4);
  });
}
extern "C" int tsd_encoder_forward(tsd_model* m, const float* images, const float* noise, int B, int S,
                                   float* latents) {
  return tsd_encoder_forward_hw(m, images, noise, B, S, S, latents);
}

extern "C" int tsd_clip_forward(tsd_model* m, const int32_t* tokens, int B, int T, float* context) {
  NOTNULL(m); NOTNULL(tokens); NOTNULL(context);
  if (!is_clip_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "tsd_clip_forward: model is not a CLIP");
  if (B <= 0 || T <= 0 || T > 77) TSD_FAIL(TSD_E_SHAPE, "clip: B=%d T=%d (1..77 tokens)", B, T);
  tsd_ctx* ctx = m->ctx;
  std::vector<int32_t> padded((size_t)B * 77, 0);  // clip.mojo:91-93: a zero row of 77 ids, the prompt's ids in front
  for (int b = 0; b < B; b++)
    for (int t = 0; t < T; t++) padded[(size_t)b * 77 + t] = tokens[(size_t)b * T + t];
  return run_model(m, [&]() -> int {
    const int64_t no = (int64_t)B * 77 * m->clip.D;
    int* dt = arena_alloc<int>(ctx, (int64_t)B * 77);
    float* dout = arena_alloc<float>(ctx, no);
    if (!dt || !dout) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, dt, padded.data(), padded.size() * sizeof(int32_t)));
    TSD_TRY(g_clip_forward(m, dt, B, dout));
    return d2h(ctx, context, dout, no * 4);
  });
}

// CLIP vision encoder: pixels on 0 .. 255 -> the 1024-wide image embedding (and, on request, the input of the last layer)
extern "C" int tsd_clip_vision_forward(tsd_model* m, const float* images, int B, int H, int W, float* image_embeds, float* hidden_out) {
  NOTNULL(m); NOTNULL(images); NOTNULL(image_embeds);
  if (!is_clip_vision_kind(m->kind)) TSD_FAIL(TSD_E_ARG, "tsd_clip_vision_forward: model is not a CLIP vision encoder");
  if (B <= 0 || B > 16) TSD_FAIL(TSD_E_SHAPE, "clip vision: B=%d (1..16)", B);
  if (H < 8 || W < 8 || H > 2048 || W > 2048) TSD_FAIL(TSD_E_SHAPE, "clip vision: image sides %d x %d outside 8 .. 2048", H, W);
  tsd_ctx* ctx = m->ctx;
  return run_model(m, [&]() -> int {
    const int64_t ni = (int64_t)B * 3 * H * W, ne = (int64_t)B * CV_EMBED, nh = (int64_t)B * CV_TOKENS * CV_WIDTH;
    float* di = arena_alloc<float>(ctx, ni);
    float* de = arena_alloc<float>(ctx, ne);
    float* dh = hidden_out ? arena_alloc<float>(ctx, nh) : nullptr;
    if (!di || !de || (hidden_out && !dh)) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(h2d(ctx, di, images, (size_t)ni * 4));
    TSD_TRY(g_clip_vision_forward(m, di, B, H, W, de, dh));
    if (hidden_out) TSD_TRY(d2h(ctx, hidden_out, dh, (size_t)nh * 4));
    return d2h(ctx, image_embeds, de, (size_t)ne * 4);
  });
}

extern "C" int tsd_model_context_width(const tsd_model* m) {
  if (!m) TSD_FAIL(TSD_E_ARG, "NULL model");
  const int w = model_context_width(m);
  if (w <= 0) TSD_FAIL(TSD_E_ARG, "tsd_model_context_width: model kind %d neither reads nor writes a context", m->kind);
  return w;
}

// ---- RCCL weight broadcast over xGMI ---------------------------------------
// librccl is resolved lazily with dlopen so single-GPU users never load it (and a process that already
// has torch's RCCL loaded reuses that copy: same SONAME).
namespace {
typedef struct { char internal[128]; } nccl_uid;
typedef int (*fn_get_uid)(nccl_uid*);
typedef int (*fn_init_rank)(void**, int, nccl_uid, int);
typedef int (*fn_bcast)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*fn_destroy)(void*);
typedef const char* (*fn_errstr)(int);
typedef int (*fn_count)(void*, int*);
struct Rccl {
  void* lib = nullptr;
  fn_get_uid get_uid = nullptr; fn_init_rank init_rank = nullptr; fn_bcast bcast = nullptr; fn_destroy destroy = nullptr;
  fn_errstr errstr = nullptr;
  fn_count count = nullptr;
};
Rccl g_rccl;
int rccl_load() {
  if (g_rccl.lib) return TSD_OK;
  // A process must use ONE HIP runtime: torch wheels bundle their own libamdhip64 + librccl, and an RCCL built against the
  // other runtime fails in ncclCommInitRank ("unhandled cuda error": round-1 log, libtsd loaded /opt/rocm's runtime first
  // and a later `import torch` mapped a second one).  So: first take an RCCL that is ALREADY mapped (RTLD_NOLOAD; it belongs
  // to the runtime the process is using - with torch imported first libtsd itself binds to torch's libamdhip64, same
  // SONAME), and only otherwise load the system one.  scripts/diag_rccl_coresident.py shows the three cases.
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) {
    g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
    if (g_rccl.lib) break;
  }
  for (int i = 0; i < 3 && !g_rccl.lib; i++) {
    const char* order[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    g_rccl.lib = dlopen(order[i], RTLD_NOW | RTLD_GLOBAL);
  }
  if (!g_rccl.lib) TSD_FAIL(TSD_E_RCCL, "cannot dlopen librccl: %s", dlerror());
  g_rccl.get_uid = (fn_get_uid)dlsym(g_rccl.lib, "ncclGetUniqueId");
  g_rccl.init_rank = (fn_init_rank)dlsym(g_rccl.lib, "ncclCommInitRank");
  g_rccl.bcast = (fn_bcast)dlsym(g_rccl.lib, "ncclBroadcast");
  g_rccl.destroy = (fn_destroy)dlsym(g_rccl.lib, "ncclCommDestroy");
  g_rccl.errstr = (fn_errstr)dlsym(g_rccl.lib, "ncclGetErrorString");
  g_rccl.count = (fn_count)dlsym(g_rccl.lib, "ncclCommCount");
  if (!g_rccl.get_uid || !g_rccl.init_rank || !g_rccl.bcast || !g_rccl.destroy)
    TSD_FAIL(TSD_E_RCCL, "librccl is missing ncclGetUniqueId/ncclCommInitRank/ncclBroadcast");
  return TSD_OK;
}
#define RCCL_TRY(expr)                                                                                     \
  do {                                                                                                     \
    int r__ = (expr);                                                                                      \
    if (r__ != 0) TSD_FAIL(TSD_E_RCCL, "%s failed: %s", #expr, g_rccl.errstr ? g_rccl.errstr(r__) : "?"); \
  } while (0)
}  // namespace

extern "C" int tsd_dist_unique_id(void* id128) {
  NOTNULL(id128);
  TSD_TRY(rccl_load());
  nccl_uid id;
  RCCL_TRY(g_rccl.get_uid(&id));
  memcpy(id128, &id, 128);
  return TSD_OK;
}

extern "C" int tsd_dist_init(tsd_ctx* ctx, int rank, int nranks, const void* id128) {
  NOTNULL(ctx); NOTNULL(id128);
  if (nranks <= 0 || rank < 0 || rank >= nranks) TSD_FAIL(TSD_E_ARG, "dist: rank %d / %d", rank, nranks);
  if (ctx->rccl_comm)  // a second communicator would overwrite - and so leak - the first; nothing changes
    TSD_FAIL(TSD_E_STATE, "dist: this context already holds a communicator (rank %d / %d); call tsd_dist_finalize first", ctx->rank, ctx->nranks);
  TSD_TRY(rccl_load());
  HIP_TRY(hipSetDevice(ctx->device));
  nccl_uid id;
  memcpy(&id, id128, 128);
  void* comm = nullptr;
  RCCL_TRY(g_rccl.init_rank(&comm, nranks, id, rank));
  ctx->rccl_comm = comm; ctx->rank = rank; ctx->nranks = nranks;
  return TSD_OK;
}

extern "C" int tsd_dist_broadcast_weights(tsd_model* m, int root) {
  NOTNULL(m);
  tsd_ctx* ctx = m->ctx;
  if (!ctx->rccl_comm) TSD_FAIL(TSD_E_STATE, "dist: tsd_dist_init was not called on this context");
  HIP_TRY(hipSetDevice(ctx->device));
  // one broadcast of the whole packed blob (fp16 weights + fp32 biases), ncclInt8 = 0
  RCCL_TRY(g_rccl.bcast(m->blob, m->blob, m->blob_bytes, 0 /*ncclInt8*/, root, ctx->rccl_comm, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return tsd_model_mark_loaded(m);
}

extern "C" int tsd_dist_comm_count(tsd_ctx* ctx, int* nranks) {
  NOTNULL(ctx); NOTNULL(nranks);
  if (!ctx->rccl_comm) TSD_FAIL(TSD_E_STATE, "dist: tsd_dist_init was not called on this context");
  if (!g_rccl.count) TSD_FAIL(TSD_E_RCCL, "librccl has no ncclCommCount");
  RCCL_TRY(g_rccl.count(ctx->rccl_comm, nranks));
  return TSD_OK;
}

void dist_release(tsd_ctx* ctx) {
  if (ctx->rccl_comm && g_rccl.destroy) g_rccl.destroy(ctx->rccl_comm);
  ctx->rccl_comm = nullptr;
}
extern "C" int tsd_dist_finalize(tsd_ctx* ctx) {
  NOTNULL(ctx);
  dist_release(ctx);
  return TSD_OK;
}
