// session.cpp - the device-resident denoise session (pipeline.mojo:57-127 + sampler.mojo:15-124): lockstep steps and slot mode.
// A step's scalars come from one place, sampler_step_plan (sampler.cpp); what the entry points share is the session_* helpers below.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "graph.h"

// Every entry point opens with NOTNULL(p) on its pointer arguments (graph.h): TSD_E_ARG and the argument's name in
// tsd_last_error.

struct tsd_session {
  tsd_model* unet = nullptr;
  tsd_model* dec = nullptr;
  tsd_ctx* ctx = nullptr;
  int B = 0, LH = 0, LW = 0, T = 0, Tp = 0, cfg = 0;  // one shape per session: latents [.,4,LH,LW]
  int Bu = 0;                                         // the UNet's batch: 2B under CFG, else B
  int W = 768;                                        // context width, from the UNet (model_context_width): 1024 for SD-2.x
  // persistent device state (own allocation, not the arena)
  char* state = nullptr;
  float* latents = nullptr;   // [B,4,LH,LW] fp32 CHW (the reference's own layout)
  float* lat2 = nullptr;      // [2B,4,LH,LW] duplicated latents for the CFG batch
  half_t* ctx16 = nullptr;    // [B or 2B][Tp][W]
  float* eps = nullptr;       // [B or 2B,4,LH,LW]
  float* tdev = nullptr;      // [16] timestep per sample
  float* temb = nullptr;      // [16][320]
  float* noise = nullptr;     // [nsteps,B,4,LH,LW] or null
  float* images = nullptr;    // [B,3,8LH,8LW]
  float* hist = nullptr;      // [B,4,LH,LW] fp32: the data prediction x0 of the previous step (DPM-Solver++(2M))
  // masked denoising (tsd_session_set_inpaint): carved from `state` like the rest, filled by set_inpaint, read by the blend of a step
  float* ip_mask = nullptr;   // [B][LH*LW] fp32 in [0,1]: 1 = regenerate, 0 = keep `ip_known`
  float* ip_known = nullptr;  // [B,4,LH,LW] the original latents
  float* ip_noise = nullptr;  // [B,4,LH,LW] the noise they are re-noised with
  double* gr_part = nullptr;  // [16][CFG_RESCALE_GMAX][4] fp64: the partial moments of a step's guidance rescale (kernels_guidance.hip)
  size_t noise_cap = 0;
  // What a step's UNet forward computes from the timestep and the context alone (graph.h UNetPre), made once per upload() by
  // session_build_invariants when the context's session_hoist is on: own allocations, grown at upload() like `noise`, never in a step.
  char* kv = nullptr;         // kc_all [Bu*Tp][CK] | vtc_all [Bu][CK][Tp] fp16: the context K / V^T of all attention blocks
  half_t* kc_all = nullptr;
  half_t* vtc_all = nullptr;
  float* ttab = nullptr;      // [timesteps.size()][tproj.N] fp32: the time projections of every schedule entry (one row serves every sample)
  size_t kv_cap = 0, ttab_cap = 0;
  bool hoist = false;         // the steps of this upload() run on them
  unsigned model_gen = 0;     // generation of the UNet's parameters (tsd_model::gen) at the last upload() / rebuild
  int inv_builds = 0;         // session_build_invariants calls so far (tsd_debug_session_hoist_info)
  // schedule (sampler.mojo:15-44)
  int n_train = 1000, n_infer = 50, start = 0;
  std::vector<float> alphas_cumprod;
  std::vector<int> timesteps;
  // sampler (tsd_session_set_sampler); the default is the reference's DDPMSampler on its own timestep rule
  int sampler = TSD_SAMPLER_DDPM, spacing = TSD_SPACING_LEADING;
  float eta = 0.f;
  // what the model output means and which table alphas_cumprod is (tsd_session_set_prediction); persists across uploads.  Under
  // TSD_PRED_V every plan is SLOT_LMS and step() / advance() launch the v kernels (kernels_vpred.hip)
  int prediction = TSD_PRED_EPSILON, ztsnr = 0;
  // step index for which `hist` holds the previous step's x0: i + 1 after step(i), -1 after upload() / add_noise() / set_*() and
  // after a sampler that keeps no history.  A step with any other index runs first order.
  int hist_valid_for = -1;
  bool uploaded = false, has_noise = false;
  bool ip_has_noise = false;  // lockstep inpainting: ip_noise was given (a slot's always is)
  // seeded device-side noise (tsd_session_set_seeds) belongs to one upload(): while on, a DDPM / DDIM(eta > 0) step draws its noise in the
  // update kernel from stream 16 + i of the sample's seed (counter_rng.h), no buffer and no extra launch.  Slots always draw.
  bool seeded = false;
  size_t plan_unet = 0, plan_dec = 0;
  unsigned opt_gen = 0;  // generation of the context's options the workspace was sized for (upload)
  // Latched when the host scan of a download found inf / NaN in THIS session's latents: the context's counter is cleared once reported,
  // the latents stay what they are - every later step, decode and download of this session fails with TSD_E_NONFINITE until upload()
  // replaces the state.  The context-wide counter alone does not latch it: it also counts other sessions and
  // models of the context (bench.py's scaled "peaked" model copy); its code is still returned at the synchronisation point that sees it.
  bool poisoned = false;
  bool decoded = false;  // decode() has run since the last upload(): images are defined
  // Slot mode (tsd_session_slots_open): every sample is a slot with its own request, schedule index and guidance scale; advance() moves
  // all active slots by one step with one forward.  `uploaded` stays false in slot mode - the lockstep entry points refuse by name
  // (SESSION_NOT_SLOTS) - and upload(), set_schedule and set_sampler leave it.  The index, not a timestep list, is the unit of state.
  bool slots = false;
  // What one request asks of sample b, in both modes: a slot's own, or what upload() and the lockstep setters wrote for all B samples.  It
  // belongs to one slot_start() / one upload(); a default-constructed record is "no request" (session_reset_requests).  state, index and
  // hist_valid are the slot's progress; lockstep keeps its own in hist_valid_for and the step's argument.
  struct Slot {
    int state = 0;            // 0 idle, 1 active, 2 done
    int index = 0;            // next schedule index; num_steps when done
    float cfg_scale = 7.5f;
    uint64_t seed = 0;        // set_seeds / slot_start: the streams of this sample's noise
    bool hist_valid = false;  // `hist` of this sample holds the x0 of the slot's previous step (DPM-Solver++(2M))
    bool inpaint = false;     // set_inpaint / slot_set_inpaint: sample b of ip_mask / ip_known / ip_noise is blended in after every step
    float rescale = 0.f;      // set_guidance_rescale / slot_set_guidance_rescale: phi > 0 puts launch_cfg_rescale before the update
  } slot[16];
  float* trows = nullptr;     // [Bu][tproj.N] fp32: row i_b of ttab per sample, gathered by every advance (own allocation, grown at slots_open)
  size_t trows_cap = 0;
  // ControlNet (tsd_session_set_control): lockstep sessions on a full-size UNet.  It stays until set_control(NULL); upload() rebuilds what
  // depends on the context and the schedule.  A step inside [ctl_first, ctl_last] runs the ControlNet forward at the UNet's batch and then
  // the controlled UNet forward in one arena; every other step enqueues what it always did.
  tsd_model* cn = nullptr;    // nullptr: no control
  int ctl_first = 0, ctl_last = -1;  // ctl_last < 0: to the end of the list
  char* ctl = nullptr;        // scale [16] fp32 | hint features fp16 [Bu][LH*LW][320]: written by set_control, read by every controlled step
  float* ctl_scale = nullptr; // per sample of the UNet's batch: the scale, 0 on the uncond half under cond_only
  half_t* ctl_feat = nullptr;
  size_t ctl_cap = 0;
  char* cn_kv = nullptr;      // the ControlNet's own hoisted context K / V^T and time table, like kv / ttab
  half_t* cn_kc = nullptr; half_t* cn_vtc = nullptr;
  float* cn_ttab = nullptr;
  size_t cn_kv_cap = 0, cn_ttab_cap = 0;
  unsigned cn_gen = 0;        // generation of the ControlNet's parameters at the last build
  // IP-Adapter (tsd_session_set_ip_adapter): lockstep sessions on a full-size SD-1.x UNet.  Everything it needs is built by the setter,
  // once - the image tokens do not depend on the step, the context or the schedule - and stays until set_ip_adapter(NULL): upload()
  // rebuilds nothing of it.  A step inside [ip_first, ip_last] hands the buffers to the forward; every other step enqueues what it always did.
  tsd_model* ip = nullptr;    // nullptr: no adapter
  int ip_first = 0, ip_last = -1, ip_N = 0;
  float ip_scale_host = 0.f;  // the one scale of every sample
  char* ipb = nullptr;        // scale [16] fp32 | K_ip fp16 [Bu*16][IK] | V_ip^T fp16 [Bu][IK][16]
  float* ip_scale = nullptr;
  half_t* ip_k = nullptr; half_t* ip_vt = nullptr;
  size_t ipb_cap = 0;
};

// inf / NaN scan of a downloaded tensor (exponent bits all ones); the buffers at this boundary are 0.5 - 25 MB
static bool host_all_finite(const float* p, size_t n) {
  unsigned bad = 0;
  for (size_t i = 0; i < n; i++) {
    unsigned u;
    memcpy(&u, p + i, 4);
    bad |= ((u & 0x7f800000u) == 0x7f800000u);
  }
  return bad == 0;
}
#define SESSION_NOT_POISONED(s)                                                                                              \
  do {                                                                                                                       \
    if ((s)->poisoned)                                                                                                       \
      TSD_FAIL(TSD_E_NONFINITE, "session: inf / NaN was found in this session's latents or images (reported at an earlier " \
               "download); its state is unusable until upload() replaces it");                                              \
  } while (0)

#define SESSION_NOT_SLOTS(s, what)                                                                                           \
  do {                                                                                                                       \
    if ((s)->slots)                                                                                                          \
      TSD_FAIL(TSD_E_STATE, "session: " what " moves the batch in lockstep and the session is in slot mode (slots_open); use the " \
               "slot entry points, or upload() to leave slot mode");                                                        \
  } while (0)

#define SESSION_IN_SLOTS(s)                                                                                   \
  do {                                                                                                        \
    if (!(s)->slots) TSD_FAIL(TSD_E_STATE, "session: slots_open() first (the session is not in slot mode)"); \
  } while (0)

// The argument checks of the slot and step entry points, in NOTNULL's form (graph.h): slot b exists, is active, step i is in the list
#define SLOT_IN_RANGE(s, b) \
  if ((b) < 0 || (b) >= (s)->B) TSD_FAIL(TSD_E_ARG, "session: slot %d out of range (0..%d)", (b), (s)->B - 1)
#define SLOT_IS_ACTIVE(s, b, what) \
  if ((s)->slot[b].state != 1)     \
  TSD_FAIL(TSD_E_STATE, "session: slot %d is %s; " what " belongs to an active request", (b), (s)->slot[b].state ? "done" : "idle")
#define STEP_IN_RANGE(s, i) \
  if ((i) < 0 || (i) >= (int)(s)->timesteps.size()) TSD_FAIL(TSD_E_ARG, "session: step %d out of range", (i))

// ---- what the entry points share ---------------------------------------------------------------------------------------------
// The workspace was sized under the context's options of upload() / slots_open() (`sized_by`); a tsd_debug_set_* call since then is refused.
static int session_options_unchanged(const tsd_session* s, const char* sized_by) {
  if (s->opt_gen != s->ctx->opt.gen)
    TSD_FAIL(TSD_E_STATE, "session: a tsd_debug_set_* call changed this context's options after %s sized the workspace; %s again",
             sized_by, sized_by);
  return TSD_OK;
}
// What belonged to one upload() / one slot_start() is gone: `count` request records from `first` are "no request" again.
static void session_reset_requests(tsd_session* s, int first = 0, int count = 16) {
  for (int b = first; b < first + count; b++) s->slot[b] = tsd_session::Slot();
}
// The latents are no longer those the history was predicted from, and the images are not theirs any more.
static void session_latents_changed(tsd_session* s) {
  s->hist_valid_for = -1;
  s->decoded = false;
}
// One of the session's own growable device buffers holds `bytes`: kept while large enough, else replaced (the contents are lost).
static int session_grow(tsd_ctx* ctx, void** ptr, size_t* cap, size_t bytes, const char* what) {
  if (bytes <= *cap) return TSD_OK;
  if (*ptr) HIP_TRY(dev_free(*ptr));
  *ptr = nullptr; *cap = 0;
  if (dev_malloc(ptr, bytes) != hipSuccess) TSD_FAIL(TSD_E_ALLOC, "session: allocating the %s buffer (%zu bytes) failed", what, bytes);
  *cap = bytes;
  if (ctx->opt.debug_poison >= 0 && (ctx->opt.debug_poison_what & 8)) HIP_TRY(hipMemsetAsync(*ptr, ctx->opt.debug_poison & 255, bytes, ctx->stream));
  return TSD_OK;
}
// `samples` host contexts [T][W] fp32 -> rows first .. first + samples of ctx16, fp16 [Tp][W] with ZERO pad rows: the conversion the
// V^T pad-column contract rests on (include/tsd.h).  Through the staging buffer, which the caller reserved; synchronises, so `src` and
// the staging buffer are free again on return.
static int session_put_context(tsd_session* s, const float* src, size_t first, int samples) {
  tsd_ctx* ctx = s->ctx;
  const size_t nc = (size_t)s->T * s->W;
  HIP_TRY(hipMemcpyAsync(ctx->staging, src, samples * nc * 4, hipMemcpyHostToDevice, ctx->stream));
  for (int b = 0; b < samples; b++)
    TSD_TRY(launch_f32_to_f16_rows(ctx, (const float*)ctx->staging + b * nc, s->T, s->W, s->ctx16 + (first + b) * s->Tp * s->W, s->W, s->Tp));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}
// add_noise at schedule index i on n floats at `lat` (sampler.mojo:100-124, fp32 scalars like the reference)
static int session_add_noise(tsd_session* s, int i, float* lat, int64_t n, const float* noise) {
  const float a = s->alphas_cumprod[s->timesteps[i]];
  return launch_add_noise(s->ctx, lat, noise, n, sqrtf(a), sqrtf(1.f - a));
}
// n latents leave the device.  What leaves HERE is checked itself: the context's count may have been reported (and cleared) at another
// model's synchronisation point, and it may be another session's - only this session's own buffer latches the poison.
static int session_fetch_latents(tsd_session* s, const float* dev, size_t n, float* host) {
  HIP_TRY(hipMemcpyAsync(host, dev, n * 4, hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  const int r = ctx_check_status(s->ctx);
  if (!host_all_finite(host, n)) s->poisoned = true;
  if (r != TSD_OK) return r;
  SESSION_NOT_POISONED(s);
  return TSD_OK;
}

// The session's configuration: what set_schedule, set_sampler and set_prediction each change a part of.
struct SessionConfig {
  int n_train, n_infer, start, sampler, spacing, prediction, ztsnr;
  float eta;
};
static SessionConfig session_config(const tsd_session* s) {
  return {s->n_train, s->n_infer, s->start, s->sampler, s->spacing, s->prediction, s->ztsnr, s->eta};
}
// the device noise buffer and the workspace plan were sized for the OLD schedule, the history and the images belong to it: a new
// upload() is required
static void schedule_changed(tsd_session* s) {
  s->uploaded = false; s->has_noise = false;
  s->slots = false;
  s->seeded = false;
  session_reset_requests(s);
  session_latents_changed(s);
}
// alphas_cumprod (sampler.mojo:28-32, or its zero-terminal-SNR rescale) and the timestep list of the spacing with `start` entries dropped
// (sampler.cpp), built aside and checked as a whole - epsilon-prediction cannot run a list with a timestep of alpha_bar = 0 - before the
// session takes any of it: a refused configuration leaves the session, its upload included, as it was.
static int session_configure(tsd_session* s, const SessionConfig& c) {
  std::vector<float> ac;
  std::vector<int> ts;
  TSD_TRY(sampler_alphas_cumprod(c.n_train, c.ztsnr, ac));
  TSD_TRY(sampler_timesteps(c.spacing, c.n_train, c.n_infer, c.start, ts));
  TSD_TRY(sampler_prediction_ok(c.prediction, ac, ts));
  s->n_train = c.n_train; s->n_infer = c.n_infer; s->start = c.start;
  s->sampler = c.sampler; s->spacing = c.spacing; s->eta = c.eta;
  s->prediction = c.prediction; s->ztsnr = c.ztsnr;
  s->alphas_cumprod.swap(ac);
  s->timesteps.swap(ts);
  schedule_changed(s);
  return TSD_OK;
}
// Fill the session's step-invariant buffers on the context's stream, with the launches (same kernels, same arguments, same batch) a
// step's forward would make for them, so their contents are the bits the per-step path computes:
//   * context K / V^T: the forward's own projection launch, once;
//   * time table: per schedule entry, the time embedding of its timestep for Bu samples and the three small linears behind it; every
//     sample sees the same timestep, so the Bu rows are equal and row 0 is kept (the forward reads it with a per-sample stride of 0).
// The arena (sized by upload() for this too) is scratch; nothing here synchronises.
static int session_build_invariants_of(tsd_session* s, tsd_model* m, half_t* kc_all, half_t* vtc_all, float* ttab) {
  tsd_ctx* ctx = s->ctx;
  const int Bu = s->Bu, N = m->unet.tproj.N;
  ctx->arena.top = 0;
  TSD_TRY(g_unet_ctx_kv(m, s->ctx16, s->Tp, Bu, kc_all, vtc_all));
  for (size_t i = 0; i < s->timesteps.size(); i++) {
    ctx->arena.top = 0;
    TSD_TRY(launch_time_embedding(ctx, nullptr, (float)s->timesteps[i], Bu, s->temb));
    const float* tvec = nullptr;
    TSD_TRY(g_unet_time_path(m, s->temb, Bu, &tvec));
    HIP_TRY(hipMemcpyAsync(ttab + i * (size_t)N, tvec, (size_t)N * 4, hipMemcpyDeviceToDevice, ctx->stream));
  }
  ctx->arena.top = 0;
  return TSD_OK;
}
static int session_build_invariants(tsd_session* s) {
  TSD_TRY(session_build_invariants_of(s, s->unet, s->kc_all, s->vtc_all, s->ttab));
  s->model_gen = s->unet->gen;
  s->inv_builds++;
  return TSD_OK;
}
// the same for the ControlNet of a session with control: its own weights, the session's context and schedule
static int session_build_control_invariants(tsd_session* s) {
  TSD_TRY(session_build_invariants_of(s, s->cn, s->cn_kc, s->cn_vtc, s->cn_ttab));
  s->cn_gen = s->cn->gen;
  return TSD_OK;
}
static UNetPre session_control_pre(const tsd_session* s, int i) {
  UNetPre p;
  p.tvec = s->cn_ttab + (size_t)i * s->cn->unet.tproj.N; p.tld = 0;
  p.kc_all = s->cn_kc; p.vtc_all = s->cn_vtc;
  return p;
}
static bool session_controls(const tsd_session* s, int i) {
  return s->cn && i >= s->ctl_first && (s->ctl_last < 0 || i <= s->ctl_last);
}
static UNetPre session_pre(const tsd_session* s, int i) {
  UNetPre p;
  p.tvec = s->ttab + (size_t)i * s->unet->unet.tproj.N; p.tld = 0;
  p.kc_all = s->kc_all; p.vtc_all = s->vtc_all;
  return p;
}
// Parameters were set since the last build: the derived weights, then what this session derived from them (all samples).
static int session_refresh(tsd_session* s) {
  if (s->cn && s->cn_gen != s->cn->gen) {
    TSD_TRY(model_check_ready(s->cn));
    if (s->hoist) TSD_TRY(session_build_control_invariants(s));
    s->cn_gen = s->cn->gen;
  }
  if (s->model_gen == s->unet->gen) return TSD_OK;
  TSD_TRY(model_check_ready(s->unet));
  if (s->hoist) TSD_TRY(session_build_invariants(s));
  s->model_gen = s->unet->gen;
  return TSD_OK;
}
// The UNet forward of a step or an advance: latents (twice under CFG: model_input for both passes is the same latents,
// pipeline.mojo:107-108) -> eps.  `pre` is read under the hoist only.  eps stays in the output convolution's layout ([B][LH*LW][4])
// where the forward can write it; the updates read it as such (no conversion launch): *eps_hw is their eps_hw argument.
// control_i >= 0: step control_i lies in the window of a session with control - the ControlNet forward on the same inputs first, its
// residuals in the arena, then the UNet forward with them; no copy from the host and no allocation.
static bool session_adapts(const tsd_session* s, int i) {
  // at scale 0 the adapter adds nothing: such a step is the plain one, as tsd_diffusion_forward_ip_hw with every scale 0 is the plain forward
  return s->ip && s->ip_scale_host != 0.f && i >= s->ip_first && (s->ip_last < 0 || i <= s->ip_last);
}
static IpRun session_ip_run(const tsd_session* s) {
  IpRun r;
  r.ip = s->ip; r.k_all = s->ip_k; r.vt_all = s->ip_vt; r.N = s->ip_N; r.scale = s->ip_scale;
  return r;
}
// adapt: the step lies in the window of a session with an IP-Adapter - the UNet's attention blocks read the keys / values the setter built.
static int session_forward(tsd_session* s, const UNetPre* pre, int* eps_hw, int control_i = -1, bool adapt = false) {
  tsd_ctx* ctx = s->ctx;
  const size_t nl = (size_t)s->B * 4 * s->LH * s->LW;
  const float* lat_in = s->latents;
  if (s->cfg) {
    HIP_TRY(hipMemcpyAsync(s->lat2, s->latents, nl * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(s->lat2 + nl, s->latents, nl * 4, hipMemcpyDeviceToDevice, ctx->stream));
    lat_in = s->lat2;
  }
  ctx->arena.top = 0;
  const bool eps_nhwc = s->unet->unet.final_conv.Opad == 4;  // g_unet_forward's condition for writing that layout
  ControlRes res;
  if (control_i >= 0) {
    Act hf;
    hf.p = s->ctl_feat; hf.B = s->Bu; hf.H = s->LH; hf.W = s->LW; hf.C = 320; hf.ld = 320;
    const UNetPre cpre = s->hoist ? session_control_pre(s, control_i) : UNetPre();
    TSD_TRY(g_controlnet_forward(s->cn, lat_in, s->ctx16, s->T, s->Tp, s->temb, hf, s->Bu, s->LH, s->LW, s->hoist ? &cpre : nullptr, &res));
  }
  const IpRun ipr = adapt ? session_ip_run(s) : IpRun();
  TSD_TRY(g_unet_forward(s->unet, lat_in, s->ctx16, s->T, s->Tp, s->temb, s->Bu, s->LH, s->LW, s->eps, eps_nhwc, s->hoist ? pre : nullptr,
                         control_i >= 0 ? &res : nullptr, control_i >= 0 ? s->ctl_scale : nullptr, adapt ? &ipr : nullptr));
  ctx->arena.top = 0;
  *eps_hw = eps_nhwc ? s->LH * s->LW : 0;
  return TSD_OK;
}

extern "C" int tsd_debug_set_session_hoist(tsd_ctx* ctx, int on) {
  return ctx_set_option(ctx, &TsdOptions::session_hoist, on ? 1 : 0, 0, 1);
}
extern "C" int tsd_debug_session_hoist_info(tsd_session* s, int64_t* info) {
  NOTNULL(s); NOTNULL(info);
  info[0] = (s->uploaded || s->slots) && s->hoist; info[1] = (int64_t)(uintptr_t)s->ttab; info[2] = (int64_t)(uintptr_t)s->kc_all;
  info[3] = (int64_t)(uintptr_t)s->vtc_all; info[4] = (int64_t)(s->kv_cap + s->ttab_cap); info[5] = s->inv_builds;
  return TSD_OK;
}

// Every device buffer a session can own - the state block of create and the eight that session_grow sizes later - released, and the
// object with them.  The one list: tsd_session_destroy and the failure path of create go through it.
static void session_release(tsd_session* s) {
  void* const owned[] = {s->state, s->noise, s->kv, s->ttab, s->trows, s->ctl, s->cn_kv, s->cn_ttab, s->ipb};
  for (void* p : owned)
    if (p) (void)dev_free(p);
  delete s;
}

extern "C" int tsd_session_create_hw(tsd_model* diffusion, tsd_model* decoder, int B, int LH, int LW, int T, int cfg,
                                     tsd_session** out) {
  NOTNULL(diffusion); NOTNULL(out);
  if (!is_diffusion_kind(diffusion->kind)) TSD_FAIL(TSD_E_ARG, "session: first model must be a Diffusion");
  if (decoder && (!is_decoder_kind(decoder->kind) || decoder->ctx != diffusion->ctx))
    TSD_FAIL(TSD_E_ARG, "session: decoder must be a Decoder on the same context");
  const int Bu = cfg ? 2 * B : B;
  const int mult = is_full_unet_kind(diffusion->kind) ? 16 : 8;  // the UNet graph's rule per side (graph.cpp)
  if (B <= 0 || Bu > 16 || LH <= 0 || LW <= 0 || LH % mult || LW % mult || T <= 0)
    TSD_FAIL(TSD_E_SHAPE, "session: B=%d (UNet batch %d <= 16) L=%dx%d (multiples of %d) T=%d", B, Bu, LH, LW, mult, T);
  tsd_ctx* ctx = diffusion->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  tsd_session* s = new tsd_session();
  s->unet = diffusion; s->dec = decoder; s->ctx = ctx;
  s->B = B; s->LH = LH; s->LW = LW; s->T = T; s->Tp = round_up(T, 8); s->cfg = cfg ? 1 : 0; s->Bu = Bu;
  s->W = model_context_width(diffusion);
  const size_t hw = (size_t)LH * LW, nl = (size_t)B * 4 * hw;
  size_t off = 0;
  auto carve = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~size_t(255); return o; };
  const size_t o_lat = carve(nl * 4), o_lat2 = carve(2 * nl * 4), o_ctx = carve((size_t)Bu * s->Tp * s->W * 2),
               o_eps = carve((size_t)Bu * 4 * hw * 4), o_t = carve(16 * 4), o_te = carve(16 * 320 * 4),
               o_img = carve(decoder ? (size_t)B * 3 * 64 * hw * 4 : 0), o_hist = carve(nl * 4),
               o_ipm = carve((size_t)B * hw * 4), o_ipk = carve(nl * 4), o_ipn = carve(nl * 4),
               o_grp = carve((size_t)CFG_RESCALE_PARTIAL_DOUBLES * sizeof(double));
  hipError_t e = dev_malloc((void**)&s->state, off);
  if (e != hipSuccess) { delete s; TSD_FAIL(TSD_E_ALLOC, "session: allocating %zu bytes failed: %s", off, hipGetErrorString(e)); }
  if (ctx->opt.debug_poison >= 0 && (ctx->opt.debug_poison_what & 4)) hipMemsetAsync(s->state, ctx->opt.debug_poison & 255, off, ctx->stream);
  s->latents = (float*)(s->state + o_lat); s->lat2 = (float*)(s->state + o_lat2);
  s->ctx16 = (half_t*)(s->state + o_ctx); s->eps = (float*)(s->state + o_eps);
  s->tdev = (float*)(s->state + o_t); s->temb = (float*)(s->state + o_te);
  s->images = decoder ? (float*)(s->state + o_img) : nullptr;
  s->hist = (float*)(s->state + o_hist);
  s->ip_mask = (float*)(s->state + o_ipm); s->ip_known = (float*)(s->state + o_ipk); s->ip_noise = (float*)(s->state + o_ipn);
  s->gr_part = (double*)(s->state + o_grp);
  if (session_configure(s, session_config(s)) != TSD_OK) { session_release(s); return TSD_E_ARG; }
  dev_handle_count(DEV_SESSION, +1);
  *out = s;
  return TSD_OK;
}
extern "C" int tsd_session_create(tsd_model* diffusion, tsd_model* decoder, int B, int L, int T, int cfg,
                                  tsd_session** out) {
  return tsd_session_create_hw(diffusion, decoder, B, L, L, T, cfg, out);
}
extern "C" int tsd_session_shape(tsd_session* s, int* LH, int* LW) {
  NOTNULL(s); NOTNULL(LH); NOTNULL(LW);
  *LH = s->LH; *LW = s->LW;
  return TSD_OK;
}

extern "C" int tsd_session_destroy(tsd_session* s) {
  if (!s) return TSD_OK;
  hipSetDevice(s->ctx->device);
  hipStreamSynchronize(s->ctx->stream);
  session_release(s);
  dev_handle_count(DEV_SESSION, -1);
  return TSD_OK;
}

extern "C" int tsd_session_set_schedule(tsd_session* s, int num_training_steps, int num_inference_steps,
                                        int start_step) {
  NOTNULL(s);
  if (num_training_steps <= 0 || num_inference_steps <= 0 || num_inference_steps > num_training_steps ||
      start_step < 0 || start_step >= num_inference_steps)
    TSD_FAIL(TSD_E_ARG, "schedule: train=%d infer=%d start=%d", num_training_steps, num_inference_steps, start_step);
  SessionConfig c = session_config(s);
  c.n_train = num_training_steps; c.n_infer = num_inference_steps; c.start = start_step;
  return session_configure(s, c);
}
extern "C" int tsd_session_set_sampler(tsd_session* s, int kind, float eta, int spacing) {
  NOTNULL(s);
  if (kind != TSD_SAMPLER_DDPM && kind != TSD_SAMPLER_DDIM && kind != TSD_SAMPLER_DPMPP_2M)
    TSD_FAIL(TSD_E_ARG, "sampler: kind %d (0 DDPM, 1 DDIM, 2 DPM-Solver++(2M))", kind);
  if (spacing != TSD_SPACING_LEADING && spacing != TSD_SPACING_TRAILING)
    TSD_FAIL(TSD_E_ARG, "sampler: timestep spacing %d (0 leading, 1 trailing)", spacing);
  if (!(eta >= 0.f)) TSD_FAIL(TSD_E_ARG, "sampler: eta %g < 0", (double)eta);
  SessionConfig c = session_config(s);
  c.sampler = kind; c.eta = eta; c.spacing = spacing;
  return session_configure(s, c);  // the timestep list may have changed: as after set_schedule
}
extern "C" int tsd_session_set_prediction(tsd_session* s, int prediction, int zero_terminal_snr) {
  NOTNULL(s);
  if (prediction != TSD_PRED_EPSILON && prediction != TSD_PRED_V)
    TSD_FAIL(TSD_E_ARG, "session: prediction type %d (0 epsilon, 1 v)", prediction);
  if (zero_terminal_snr != 0 && zero_terminal_snr != 1) TSD_FAIL(TSD_E_ARG, "session: zero_terminal_snr %d (0 or 1)", zero_terminal_snr);
  SessionConfig c = session_config(s);
  c.prediction = prediction; c.ztsnr = zero_terminal_snr;
  return session_configure(s, c);  // the table and every step's plan may have changed: as after set_schedule
}
extern "C" int tsd_session_prediction(tsd_session* s, int* prediction, int* zero_terminal_snr) {
  NOTNULL(s); NOTNULL(prediction); NOTNULL(zero_terminal_snr);
  *prediction = s->prediction; *zero_terminal_snr = s->ztsnr;
  return TSD_OK;
}
extern "C" int tsd_session_num_steps(tsd_session* s) { return s ? (int)s->timesteps.size() : TSD_E_ARG; }
extern "C" int tsd_session_timestep(tsd_session* s, int i) {
  if (!s || i < 0 || i >= (int)s->timesteps.size()) return TSD_E_ARG;
  return s->timesteps[i];
}

// A session with control: the workspace for a controlled step (the ControlNet forward and the UNet forward share the arena: the residuals
// live there while the UNet runs) and, under the hoist, the ControlNet's own context K / V^T and time table.  Called by set_control() and
// by every upload() while the control is set - never by a step.
static int session_control_prepare(tsd_session* s) {
  tsd_ctx* ctx = s->ctx;
  const int Bu = s->Bu, LH = s->LH, LW = s->LW, T = s->T, Tp = s->Tp;
  TSD_TRY(model_check_ready(s->cn));
  if (s->hoist) {
    const int CK = s->cn->unet.kproj_all.N, N = s->cn->unet.tproj.N;
    const size_t kc_bytes = ((size_t)Bu * Tp * CK * 2 + 255) & ~size_t(255);
    TSD_TRY(session_grow(ctx, (void**)&s->cn_kv, &s->cn_kv_cap, 2 * kc_bytes, "ControlNet context K/V"));
    s->cn_kc = (half_t*)s->cn_kv; s->cn_vtc = (half_t*)(s->cn_kv + kc_bytes);
    TSD_TRY(session_grow(ctx, (void**)&s->cn_ttab, &s->cn_ttab_cap, s->timesteps.size() * (size_t)N * 4, "ControlNet time table"));
  }
  Arena& a = ctx->arena;
  a.planning = true; a.top = 0; a.peak = 0;
  const UNetPre pre0 = s->hoist ? session_pre(s, 0) : UNetPre();
  const UNetPre cpre0 = s->hoist ? session_control_pre(s, 0) : UNetPre();
  Act hf;
  hf.p = s->ctl_feat; hf.B = Bu; hf.H = LH; hf.W = LW; hf.C = 320; hf.ld = 320;
  ControlRes res;
  int r = g_controlnet_forward(s->cn, s->lat2, s->ctx16, T, Tp, s->temb, hf, Bu, LH, LW, s->hoist ? &cpre0 : nullptr, &res);
  const IpRun ipr = s->ip ? session_ip_run(s) : IpRun();  // with an adapter set as well, the larger of the two forwards
  if (r == TSD_OK)
    r = g_unet_forward(s->unet, s->lat2, s->ctx16, T, Tp, s->temb, Bu, LH, LW, s->eps, false, s->hoist ? &pre0 : nullptr, &res, s->ctl_scale,
                       s->ip ? &ipr : nullptr);
  size_t need = a.peak;
  if (r == TSD_OK && s->hoist) {  // session_build_control_invariants' scratch
    const float* tv = nullptr;
    a.top = 0; a.peak = 0;
    r = g_unet_time_path(s->cn, s->temb, Bu, &tv);
    need = std::max(need, a.peak);
  }
  a.planning = false; a.top = 0; a.peak = 0;
  if (r != TSD_OK) return r;
  TSD_TRY(ctx_reserve_arena(ctx, need));
  s->cn_gen = s->cn->gen;
  if (s->hoist) TSD_TRY(session_build_control_invariants(s));
  return TSD_OK;
}

// What upload() and slots_open() share once the session's buffers hold their data: size the workspace once for this session's shapes (no
// allocation inside the timed loop), size and fill the step-invariant buffers, and mark the session ready.
static int session_prepare(tsd_session* s) {
  tsd_ctx* ctx = s->ctx;
  const int B = s->B, Bu = s->Bu, LH = s->LH, LW = s->LW, T = s->T, Tp = s->Tp;
  // size the workspace once for this session's shapes (no allocation inside the timed loop)
  TSD_TRY(model_check_ready(s->unet));
  if (s->dec) TSD_TRY(model_check_ready(s->dec));
  Arena& a = ctx->arena;
  s->hoist = ctx->opt.session_hoist != 0;
  s->uploaded = false;  // until this upload() is complete: the buffers below may move
  s->seeded = false;    // the seeds belonged to the previous upload(),
  session_reset_requests(s);  // and so did the mask, the known latents, the guidance rescale and the guidance scale
  if (s->hoist) {  // the buffers of session_build_invariants; sizes depend on the session's shape and the schedule's length only
    const int CK = s->unet->unet.kproj_all.N, N = s->unet->unet.tproj.N;
    const size_t kc_bytes = ((size_t)Bu * Tp * CK * 2 + 255) & ~size_t(255);
    TSD_TRY(session_grow(ctx, (void**)&s->kv, &s->kv_cap, 2 * kc_bytes, "context K/V"));
    s->kc_all = (half_t*)s->kv; s->vtc_all = (half_t*)(s->kv + kc_bytes);
    TSD_TRY(session_grow(ctx, (void**)&s->ttab, &s->ttab_cap, s->timesteps.size() * (size_t)N * 4, "time table"));
  }
  a.planning = true; a.top = 0; a.peak = 0;
  const UNetPre pre0 = s->hoist ? session_pre(s, 0) : UNetPre();
  int r = g_unet_forward(s->unet, s->lat2, s->ctx16, T, Tp, s->temb, Bu, LH, LW, s->eps, false, s->hoist ? &pre0 : nullptr);
  size_t need = a.peak;
  if (r == TSD_OK && s->hoist) {  // session_build_invariants' scratch
    const float* tv = nullptr;
    a.top = 0; a.peak = 0;
    r = g_unet_time_path(s->unet, s->temb, Bu, &tv);
    need = std::max(need, a.peak);
  }
  if (r == TSD_OK && s->dec) {
    a.top = 0; a.peak = 0;
    r = g_decoder_forward(s->dec, s->latents, B, LH, LW, s->images);
    need = std::max(need, a.peak);
  }
  a.planning = false; a.top = 0; a.peak = 0;
  if (r != TSD_OK) return r;
  TSD_TRY(ctx_reserve_arena(ctx, need));
  s->model_gen = s->unet->gen;
  if (s->hoist) TSD_TRY(session_build_invariants(s));
  if (s->cn) TSD_TRY(session_control_prepare(s));  // the control outlives an upload(): what depends on the context and the schedule again
  s->opt_gen = ctx->opt.gen;
  s->uploaded = true;
  s->poisoned = false;
  session_latents_changed(s);
  return TSD_OK;
}

extern "C" int tsd_session_upload(tsd_session* s, const float* latents, const float* context,
                                  const float* uncond_context, const float* noise, float cfg_scale) {
  NOTNULL(s); NOTNULL(latents); NOTNULL(context);
  if (s->cfg && !uncond_context) TSD_FAIL(TSD_E_ARG, "session: CFG session needs uncond_context");
  tsd_ctx* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int B = s->B;
  const size_t nl = (size_t)B * 4 * s->LH * s->LW;
  s->slots = false;  // upload() leaves slot mode
  HIP_TRY(hipMemcpyAsync(s->latents, latents, nl * 4, hipMemcpyHostToDevice, ctx->stream));
  // context -> fp16 [Bu][Tp][W], zero padded rows (cond first, then uncond: pipeline.mojo:49)
  TSD_TRY(ctx_reserve_staging(ctx, (size_t)B * s->T * s->W * 4));
  for (int part = 0; part < (s->cfg ? 2 : 1); part++)
    TSD_TRY(session_put_context(s, part == 0 ? context : uncond_context, (size_t)part * B, B));
  s->has_noise = noise != nullptr;
  if (noise) {
    const size_t bytes = s->timesteps.size() * nl * 4;
    TSD_TRY(session_grow(ctx, (void**)&s->noise, &s->noise_cap, bytes, "noise"));
    HIP_TRY(hipMemcpyAsync(s->noise, noise, bytes, hipMemcpyHostToDevice, ctx->stream));
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  TSD_TRY(session_prepare(s));
  for (int b = 0; b < B; b++) s->slot[b].cfg_scale = cfg_scale;  // the one request field upload() itself carries
  return TSD_OK;
}

// Streams of the seeded noise, per sample b with its record's seed: 2 the initial latents, 4 the add_noise / inpainting noise, 16 + i the
// noise of schedule step i; the counter is the element's index inside its sample, (c*LH + y)*LW + x.  Nothing depends on B or on the sample's slot.
enum { NOISE_STREAM_LATENTS = 2, NOISE_STREAM_ADD = 4, NOISE_STREAM_STEP0 = 16 };
static NormalBases session_bases(const tsd_session* s, uint64_t stream) {
  NormalBases nb = {};
  for (int b = 0; b < s->B; b++) nb.base[b] = counter_rng_base(s->slot[b].seed, stream);
  return nb;
}

// Everything the update of one step is told per sample, assembled in one place from the request records: sample b is active at schedule
// index idx[b] (hist_valid[b]: `hist` holds its previous x0), or idx[b] < 0 and its entries stay zero - SLOT_SKIP, on = 0: neither read
// nor written.  advance() passes each slot's own index; step(i) is the same thing with every sample at i.  Host arithmetic only.
struct StepTables {
  SlotTable tab;         // the plan of step idx[b] (sampler_step_plan), the request's cfg_scale, the base of stream 16 + idx[b] of its seed
  SlotBlendTable blend;  // an inpainting request holds its known region at the timestep ITS update reaches
  CfgRescaleTable gr;    // a request with phi > 0 is `on`; everyone else is neither read nor written by the rescale's launches
  bool blending, rescaling;  // some entry of blend / gr is on
};
static int session_step_tables(const tsd_session* s, const int* idx, const bool* hist_valid, StepTables* t) {
  *t = StepTables();
  for (int b = 0; b < s->B; b++) {
    const int i = idx[b];
    if (i < 0) continue;
    const tsd_session::Slot& r = s->slot[b];
    t->tab.e[b].cfg_scale = r.cfg_scale;
    t->tab.bases.base[b] = counter_rng_base(r.seed, NOISE_STREAM_STEP0 + (uint64_t)i);
    TSD_TRY(sampler_step_plan(s->sampler, s->eta, s->spacing, s->n_train, s->n_infer, s->alphas_cumprod, s->timesteps, i, hist_valid[b],
                              s->prediction, &t->tab.e[b]));
    // The blend of a step with inpainting: the known region is replaced by the original latents noised to the timestep the update has
    // just reached - entry i + 1 of the list, the clean sample (1, 0) after the last entry; under LEADING spacing that entry is the
    // reference's t - N // n.  a_prev = sqrt(abar), s_prev = sqrt(1 - abar) in double from the fp32 table, rounded to float once: what
    // tsd_sampler_coeffs reports as out[2], out[3] for step i + 1.  The same rule for all three samplers.
    if (r.inpaint) {
      const double abar = i + 1 < (int)s->timesteps.size() ? s->alphas_cumprod[s->timesteps[i + 1]] : 1.0;
      t->blend.e[b] = {1, (float)sqrt(abar), (float)sqrt(1.0 - abar), 0};
      t->blending = true;
    }
    if (r.rescale > 0.f) {
      t->gr.e[b] = {1, r.cfg_scale, r.rescale, 0};
      t->rescaling = true;
    }
  }
  return TSD_OK;
}

// The launches between a step's forward and its bookkeeping, and the only place that picks among the ten update launchers: the guidance
// rescale (every `on` sample's cond and uncond eps scaled in place before the update reads them), the update, and in lockstep the blend.
// lock_i < 0, an advance: the slot kernels read the tables; with an inpainting slot among the active ones, the kernel that also blends
// (no further launch either way).  lock_i = i, a lockstep step: every entry is the same plan and the lockstep kernels take entry 0 as
// scalars - they read the uploaded noise tensor, which no table carries.  Their noise is read from that tensor, drawn in the kernel (one
// source per upload: has_noise is off under seeds) or absent; only DPM-Solver++(2M) reads or keeps the history, and it takes no noise.
static int session_update(tsd_session* s, const StepTables& t, int eps_hw, int lock_i) {
  tsd_ctx* ctx = s->ctx;
  const int B = s->B;
  const int64_t hw = (int64_t)s->LH * s->LW, chw = 4 * hw, nl = B * chw;
  const float* eps_u = s->cfg ? s->eps + nl : nullptr;
  const bool v = s->prediction == TSD_PRED_V;
  if (t.rescaling) TSD_TRY(launch_cfg_rescale(ctx, s->eps, s->eps + nl, t.gr, B, chw, s->gr_part, nullptr));
  if (lock_i < 0) {
    if (v && t.blending)
      return launch_slot_update_blend_v(ctx, s->latents, s->eps, eps_u, s->hist, t.tab, t.blend, s->ip_mask, s->ip_known, s->ip_noise, B,
                                        chw, eps_hw);
    if (v) return launch_slot_update_v(ctx, s->latents, s->eps, eps_u, s->hist, t.tab, B, chw, eps_hw);
    if (t.blending)
      return launch_slot_update_blend(ctx, s->latents, s->eps, eps_u, s->hist, t.tab, t.blend, s->ip_mask, s->ip_known, s->ip_noise, B,
                                      chw, eps_hw);
    return launch_slot_update(ctx, s->latents, s->eps, eps_u, s->hist, t.tab, B, chw, eps_hw);
  }
  const SlotEntry& p = t.tab.e[0];
  const bool noisy = (p.flags & SLOT_NOISE) != 0, draws = noisy && s->seeded;
  const float* nz = (noisy && s->has_noise) ? s->noise + (size_t)lock_i * nl : nullptr;
  const float* hist_in = (p.flags & SLOT_HIST_IN) ? s->hist : nullptr;
  float* hist_out = (p.flags & SLOT_HIST_OUT) ? s->hist : nullptr;
  const float* c = p.c;
  const SamplerCoeffs sc = {c[0], c[1], c[2], c[3], c[4], c[5]};
  if (v && draws)
    TSD_TRY(launch_sampler_step_v_seeded(ctx, s->latents, s->eps, eps_u, p.cfg_scale, hist_in, t.tab.bases, chw, nl, sc, eps_hw, s->latents, hist_out));
  else if (v)
    TSD_TRY(launch_sampler_step_v(ctx, s->latents, s->eps, eps_u, p.cfg_scale, hist_in, nz, nl, sc, eps_hw, s->latents, hist_out));
  else if (p.mode == SLOT_DDPM && draws)
    TSD_TRY(launch_ddpm_step_seeded(ctx, s->latents, s->eps, eps_u, p.cfg_scale, t.tab.bases, chw, nl, c[0], c[1], c[2], c[3], c[4], eps_hw));
  else if (p.mode == SLOT_DDPM)
    TSD_TRY(launch_ddpm_step(ctx, s->latents, s->eps, eps_u, p.cfg_scale, nz, nl, c[0], c[1], c[2], c[3], c[4], eps_hw));
  else if (draws)
    TSD_TRY(launch_sampler_step_seeded(ctx, s->latents, s->eps, eps_u, p.cfg_scale, hist_in, t.tab.bases, chw, nl, sc, eps_hw, s->latents, hist_out));
  else
    TSD_TRY(launch_sampler_step(ctx, s->latents, s->eps, eps_u, p.cfg_scale, hist_in, nz, nl, sc, eps_hw, s->latents, hist_out));
  if (t.blending)
    TSD_TRY(launch_inpaint_blend(ctx, s->latents, s->ip_mask, s->ip_known, s->ip_has_noise ? s->ip_noise : nullptr, B, hw,
                                 t.blend.e[0].a_prev, t.blend.e[0].s_prev, s->latents));
  return TSD_OK;
}

extern "C" int tsd_session_step(tsd_session* s, int i) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "step()");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before step()");
  SESSION_NOT_POISONED(s);
  TSD_TRY(session_options_unchanged(s, "upload()"));
  STEP_IN_RANGE(s, i);
  const bool had_hist = s->hist_valid_for == i;
  session_latents_changed(s);  // no valid history until this step's update is enqueued
  TSD_TRY(session_refresh(s));
  // time embedding on the device (get_time_embedding, pipeline.mojo:89): same t for every sample
  if (!s->hoist) TSD_TRY(launch_time_embedding(s->ctx, nullptr, (float)s->timesteps[i], s->Bu, s->temb));
  const UNetPre pre = s->hoist ? session_pre(s, i) : UNetPre();
  int eps_hw = 0;
  TSD_TRY(session_forward(s, &pre, &eps_hw, session_controls(s, i) ? i : -1, session_adapts(s, i)));
  int idx[16];
  bool hist_valid[16];
  std::fill(idx, idx + 16, i);  // an advance with every sample at index i, under the lockstep history rule
  std::fill(hist_valid, hist_valid + 16, had_hist);
  StepTables t;
  TSD_TRY(session_step_tables(s, idx, hist_valid, &t));
  TSD_TRY(session_update(s, t, eps_hw, i));  // a failed step leaves no valid history
  // the blend changed the latents, not the prediction the next step extrapolates from
  if (t.tab.e[0].flags & SLOT_HIST_OUT) s->hist_valid_for = i + 1;
  return TSD_OK;
}

// ControlNet for the steps first_step <= i <= last_step (last_step < 0: to the end) of a lockstep session on a full-size UNet; cn == NULL
// turns it off.  hint: host fp32 [B,3,8LH,8LW].  The hint encoder runs here, once, at the UNet's batch (under CFG on the hint twice, the
// launches of tsd_diffusion_forward_control_hw at that batch) and its features stay on the device; the per-sample scales - `scale`, and 0
// on the uncond half under cond_only - are built here and uploaded once.  Synchronous.
extern "C" int tsd_session_set_control(tsd_session* s, tsd_model* cn, const float* hint, float scale, int cond_only, int first_step,
                                       int last_step) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "set_control()");
  if (!cn) { s->cn = nullptr; return TSD_OK; }
  NOTNULL(hint);
  if (!is_full_unet_kind(s->unet->kind)) TSD_FAIL(TSD_E_ARG, "session: set_control needs a full-size UNet (the Tiny-SD graph has no ControlNet)");
  if (!is_controlnet_kind(cn->kind)) TSD_FAIL(TSD_E_ARG, "session: set_control: the model is not a ControlNet");
  if (model_context_width(cn) != s->W)
    TSD_FAIL(TSD_E_ARG, "session: set_control: the ControlNet kinds are SD-1.x networks (context width %d); this session's UNet reads a %d-wide context",
             model_context_width(cn), s->W);
  if (cn->ctx != s->ctx) TSD_FAIL(TSD_E_ARG, "session: set_control: the ControlNet belongs to another context (the residuals live in the session's arena)");
  if (!(fabsf(scale) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "session: set_control: the scale is not finite");
  if (first_step < 0 || (last_step >= 0 && last_step < first_step)) TSD_FAIL(TSD_E_ARG, "session: set_control: window [%d, %d]", first_step, last_step);
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before set_control() (the ControlNet reads the uploaded context)");
  SESSION_NOT_POISONED(s);
  TSD_TRY(session_options_unchanged(s, "upload()"));
  tsd_ctx* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(model_check_ready(cn));
  const int B = s->B, Bu = s->Bu, LH = s->LH, LW = s->LW;
  const size_t hw = (size_t)LH * LW, nh = (size_t)B * 3 * 64 * hw, feat_bytes = (size_t)Bu * hw * 320 * 2;
  s->cn = nullptr;  // until everything below succeeded
  TSD_TRY(session_grow(ctx, (void**)&s->ctl, &s->ctl_cap, 256 + feat_bytes, "control"));
  s->ctl_scale = (float*)s->ctl; s->ctl_feat = (half_t*)(s->ctl + 256);
  float sc[16] = {};
  for (int b = 0; b < Bu; b++) sc[b] = (b >= B && cond_only) ? 0.f : scale;
  TSD_TRY(ctx_reserve_staging(ctx, (size_t)Bu * 3 * 64 * hw * 4));
  float* dh = (float*)ctx->staging;
  HIP_TRY(hipMemcpyAsync(s->ctl_scale, sc, sizeof(sc), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dh, hint, nh * 4, hipMemcpyHostToDevice, ctx->stream));
  if (s->cfg) HIP_TRY(hipMemcpyAsync(dh + nh, dh, nh * 4, hipMemcpyDeviceToDevice, ctx->stream));
  Act hf;
  TSD_TRY(run_planned(ctx, [&]() -> int {
    TSD_TRY(g_controlnet_hint(cn, dh, Bu, LH, LW, &hf));
    if (ctx->launch()) HIP_TRY(hipMemcpyAsync(s->ctl_feat, hf.p, feat_bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return TSD_OK;
  }));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  s->cn = cn; s->ctl_first = first_step; s->ctl_last = last_step;
  const int r = session_control_prepare(s);
  if (r != TSD_OK) { s->cn = nullptr; return r; }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ctx_check_status(ctx);
}
extern "C" int tsd_session_control_active(tsd_session* s) { return s ? (s->cn ? 1 : 0) : TSD_E_ARG; }

// IP-Adapter for the steps first_step <= i <= last_step (last_step < 0: to the end) of a lockstep session on a full-size SD-1.x UNet;
// ip == NULL turns it off.  tokens / uncond_tokens: host fp32 [B][N][768] for the two halves of the UNet's batch (uncond_tokens is read
// under CFG only).  The tokens are staged and K_ip / V_ip^T of all 16 blocks are projected here, once, at the UNet's batch - the launches
// of tsd_diffusion_forward_ip_hw at that batch - into buffers of the session; the per-sample scales are uploaded once.  Synchronous.
extern "C" int tsd_session_set_ip_adapter(tsd_session* s, tsd_model* ip, const float* tokens, const float* uncond_tokens, int N, float scale,
                                          int first_step, int last_step) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "set_ip_adapter()");
  if (!ip) { s->ip = nullptr; return TSD_OK; }
  NOTNULL(tokens);
  if (s->unet->kind != TSD_MODEL_DIFFUSION_SD15 && s->unet->kind != TSD_MODEL_DIFFUSION_SD15_TORCH)
    TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter needs a full-size SD-1.x UNet (an IP-Adapter of this kind fits no other graph)");
  if (!is_ip_adapter_kind(ip->kind)) TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter: the model is not an IP-Adapter");
  if (ip->ctx != s->ctx) TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter: the IP-Adapter belongs to another context");
  if (N < 1 || N > IP_MAX_TOKENS) TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter: %d image tokens (1..%d)", N, IP_MAX_TOKENS);
  if (!(fabsf(scale) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter: the scale is not finite");
  if (first_step < 0 || (last_step >= 0 && last_step < first_step)) TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter: window [%d, %d]", first_step, last_step);
  if (s->cfg && !uncond_tokens) TSD_FAIL(TSD_E_ARG, "session: set_ip_adapter: a CFG session needs uncond_tokens (the projection of a zero embedding)");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before set_ip_adapter() (the workspace is sized for the uploaded session)");
  SESSION_NOT_POISONED(s);
  TSD_TRY(session_options_unchanged(s, "upload()"));
  tsd_ctx* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(model_check_ready(ip));
  if (s->cn) TSD_TRY(model_check_ready(s->cn));
  const int B = s->B, Bu = s->Bu, LH = s->LH, LW = s->LW, T = s->T, Tp = s->Tp;
  const int IK = ip->unet.kproj_all.N;
  const size_t ntok = (size_t)B * N * IP_CTX_DIM, k_bytes = ((size_t)Bu * IP_MAX_TOKENS * IK * 2 + 255) & ~size_t(255);
  s->ip = nullptr;  // until everything below succeeded
  TSD_TRY(session_grow(ctx, (void**)&s->ipb, &s->ipb_cap, 256 + 2 * k_bytes, "IP-Adapter K/V"));
  s->ip_scale = (float*)s->ipb; s->ip_k = (half_t*)(s->ipb + 256); s->ip_vt = (half_t*)(s->ipb + 256 + k_bytes);
  float sc[16] = {};
  for (int b = 0; b < Bu; b++) sc[b] = scale;
  TSD_TRY(ctx_reserve_staging(ctx, (size_t)Bu * N * IP_CTX_DIM * 4));
  float* dtok = (float*)ctx->staging;
  HIP_TRY(hipMemcpyAsync(s->ip_scale, sc, sizeof(sc), hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(dtok, tokens, ntok * 4, hipMemcpyHostToDevice, ctx->stream));
  if (s->cfg) HIP_TRY(hipMemcpyAsync(dtok + ntok, uncond_tokens, ntok * 4, hipMemcpyHostToDevice, ctx->stream));
  TSD_TRY(run_planned(ctx, [&]() -> int {
    half_t* tok16 = arena_alloc<half_t>(ctx, (int64_t)Bu * IP_MAX_TOKENS * IP_CTX_DIM);
    if (!tok16) TSD_FAIL(TSD_E_ALLOC, "workspace arena exhausted");
    TSD_TRY(g_ip_stage_tokens(ctx, dtok, Bu, N, tok16));
    return g_ip_kv(ip, tok16, Bu, s->ip_k, s->ip_vt);
  }));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  s->ip = ip; s->ip_N = N; s->ip_first = first_step; s->ip_last = last_step; s->ip_scale_host = scale;
  // the workspace of an adapted step (every attention block op by op), with the ControlNet's forward in front where one is set
  Arena& a = ctx->arena;
  a.planning = true; a.top = 0; a.peak = 0;
  const UNetPre pre0 = s->hoist ? session_pre(s, 0) : UNetPre();
  const IpRun ipr = session_ip_run(s);
  ControlRes res;
  int r = TSD_OK;
  if (s->cn) {
    const UNetPre cpre0 = s->hoist ? session_control_pre(s, 0) : UNetPre();
    Act hf;
    hf.p = s->ctl_feat; hf.B = Bu; hf.H = LH; hf.W = LW; hf.C = 320; hf.ld = 320;
    r = g_controlnet_forward(s->cn, s->lat2, s->ctx16, T, Tp, s->temb, hf, Bu, LH, LW, s->hoist ? &cpre0 : nullptr, &res);
  }
  if (r == TSD_OK)
    r = g_unet_forward(s->unet, s->lat2, s->ctx16, T, Tp, s->temb, Bu, LH, LW, s->eps, false, s->hoist ? &pre0 : nullptr, s->cn ? &res : nullptr,
                       s->cn ? s->ctl_scale : nullptr, &ipr);
  const size_t need = a.peak;
  a.planning = false; a.top = 0; a.peak = 0;
  if (r == TSD_OK) r = ctx_reserve_arena(ctx, need);
  if (r != TSD_OK) { s->ip = nullptr; return r; }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ctx_check_status(ctx);
}
extern "C" int tsd_session_ip_adapter_active(tsd_session* s) { return s ? (s->ip ? 1 : 0) : TSD_E_ARG; }

extern "C" int tsd_session_add_noise(tsd_session* s, int i, const float* noise) {
  NOTNULL(s); NOTNULL(noise);
  SESSION_NOT_SLOTS(s, "add_noise()");
  STEP_IN_RANGE(s, i);
  tsd_ctx* ctx = s->ctx;
  const size_t nl = (size_t)s->B * 4 * s->LH * s->LW;
  TSD_TRY(ctx_reserve_staging(ctx, nl * 4));
  session_latents_changed(s);
  HIP_TRY(hipMemcpyAsync(ctx->staging, noise, nl * 4, hipMemcpyHostToDevice, ctx->stream));
  TSD_TRY(session_add_noise(s, i, s->latents, (int64_t)nl, (const float*)ctx->staging));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}

// seeds: one per sample, or NULL = off.  One source of noise per upload(): refused when the upload carried a noise tensor.
extern "C" int tsd_session_set_seeds(tsd_session* s, const uint64_t* seeds) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "set_seeds()");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before set_seeds() (the seeds belong to one upload)");
  if (seeds && s->has_noise) TSD_FAIL(TSD_E_STATE, "session: this upload() carried a noise tensor; one source of noise per upload");
  s->seeded = seeds != nullptr;
  for (int b = 0; seeds && b < s->B; b++) s->slot[b].seed = seeds[b];
  session_latents_changed(s);  // as after add_noise()
  return TSD_OK;
}
extern "C" int tsd_session_seeds_active(tsd_session* s) { return s ? (s->uploaded && s->seeded ? 1 : 0) : TSD_E_ARG; }

// phi in [0, 1]: 0 = off.  Only a flag of the steps that follow: the latents, the history and the decoded images stay what they are.
static int rescale_phi_ok(float phi) {
  if (!(phi >= 0.f && phi <= 1.f)) TSD_FAIL(TSD_E_ARG, "session: guidance rescale %g is not in [0, 1]", (double)phi);
  return TSD_OK;
}
extern "C" int tsd_session_set_guidance_rescale(tsd_session* s, float phi) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "set_guidance_rescale()");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before set_guidance_rescale() (it belongs to one upload)");
  if (!s->cfg) TSD_FAIL(TSD_E_STATE, "session: guidance rescale needs a session created with cfg != 0");
  TSD_TRY(rescale_phi_ok(phi));
  for (int b = 0; b < s->B; b++) s->slot[b].rescale = phi;
  return TSD_OK;
}
extern "C" int tsd_session_guidance_rescale(tsd_session* s, float* phi) {
  NOTNULL(s); NOTNULL(phi);
  *phi = s->uploaded ? s->slot[0].rescale : 0.f;
  return TSD_OK;
}

// the latents become stream 2 of each sample's seed: what a txt2img caller would have uploaded, drawn on the device.  Asynchronous.
extern "C" int tsd_session_seed_latents(tsd_session* s) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "seed_latents()");
  if (!s->uploaded || !s->seeded) TSD_FAIL(TSD_E_STATE, "session: upload() and set_seeds() before seed_latents()");
  HIP_TRY(hipSetDevice(s->ctx->device));
  const int64_t chw = (int64_t)4 * s->LH * s->LW;
  session_latents_changed(s);
  return launch_fill_normal(s->ctx, s->latents, s->B * chw, chw, session_bases(s, NOISE_STREAM_LATENTS), 0);
}

// add_noise at index i with stream 4 of each sample's seed instead of a host tensor: the same scalars and the same kernel
extern "C" int tsd_session_add_noise_seeded(tsd_session* s, int i) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "add_noise_seeded()");
  if (!s->uploaded || !s->seeded) TSD_FAIL(TSD_E_STATE, "session: upload() and set_seeds() before add_noise_seeded()");
  STEP_IN_RANGE(s, i);
  tsd_ctx* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int64_t chw = (int64_t)4 * s->LH * s->LW, nl = s->B * chw;
  TSD_TRY(ctx_reserve_staging(ctx, (size_t)nl * 4));
  session_latents_changed(s);
  TSD_TRY(launch_fill_normal(ctx, (float*)ctx->staging, nl, chw, session_bases(s, NOISE_STREAM_ADD), 0));
  TSD_TRY(session_add_noise(s, i, s->latents, nl, (const float*)ctx->staging));
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the staging buffer is the context's again on return, as after add_noise()
  return TSD_OK;
}

// An inpainting request for samples [first, first + n) of ip_mask / ip_known / ip_noise: checked as a whole - the mask finite and in
// [0, 1], the known latents and the optional noise finite - before the first copy, so a refused call leaves the previous mask, tensors and
// history as they were; then copied, ip_noise from `noise` or drawn from `draw` (base k for sample first + k) or left alone.  Synchronises:
// the host tensors are the caller's again on return.  `who` names the entry point in the message.
static int session_put_inpaint(tsd_session* s, int first, int n, const float* mask, const float* known, const float* noise,
                               const NormalBases* draw, const char* who) {
  tsd_ctx* ctx = s->ctx;
  const size_t hw = (size_t)s->LH * s->LW, nm = n * hw, nl = 4 * nm, m0 = first * hw, l0 = 4 * m0;
  bool in_range = true;
  for (size_t k = 0; k < nm; k++) in_range &= (mask[k] >= 0.f) & (mask[k] <= 1.f);  // false for NaN
  if (!in_range) TSD_FAIL(TSD_E_ARG, "session: every inpainting mask value must be finite and in [0, 1]");
  if (!host_all_finite(known, nl)) TSD_FAIL(TSD_E_ARG, "session: inf / NaN in the known latents of %s", who);
  if (noise && !host_all_finite(noise, nl)) TSD_FAIL(TSD_E_ARG, "session: inf / NaN in the noise of %s", who);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(s->ip_mask + m0, mask, nm * 4, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(hipMemcpyAsync(s->ip_known + l0, known, nl * 4, hipMemcpyHostToDevice, ctx->stream));
  if (noise) HIP_TRY(hipMemcpyAsync(s->ip_noise + l0, noise, nl * 4, hipMemcpyHostToDevice, ctx->stream));
  if (draw) TSD_TRY(launch_fill_normal(ctx, s->ip_noise + l0, (int64_t)nl, (int64_t)(4 * hw), *draw, 0));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return TSD_OK;
}
// set_inpaint and set_inpaint_seeded: `seeded` fills ip_noise with stream 4 of each sample's seed on the device instead of copying `noise`
static int session_set_inpaint(tsd_session* s, const float* mask, const float* known, const float* noise, bool seeded) {
  SESSION_NOT_SLOTS(s, "set_inpaint()");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before set_inpaint() (inpainting belongs to one upload)");
  if (seeded && mask && !s->seeded) TSD_FAIL(TSD_E_STATE, "session: set_seeds() before set_inpaint_seeded()");
  if (mask) {
    NOTNULL(known);
    const NormalBases nb = session_bases(s, NOISE_STREAM_ADD);
    TSD_TRY(session_put_inpaint(s, 0, s->B, mask, known, noise, seeded ? &nb : nullptr, "set_inpaint()"));
  }
  for (int b = 0; b < s->B; b++) s->slot[b].inpaint = mask != nullptr;
  s->ip_has_noise = mask && (noise || seeded);
  session_latents_changed(s);  // the steps that follow run on other latents than the history was predicted for: as after add_noise()
  return TSD_OK;
}
extern "C" int tsd_session_set_inpaint(tsd_session* s, const float* mask, const float* known, const float* noise) {
  NOTNULL(s);
  return session_set_inpaint(s, mask, known, noise, false);
}
extern "C" int tsd_session_set_inpaint_seeded(tsd_session* s, const float* mask, const float* known) {
  NOTNULL(s);
  return session_set_inpaint(s, mask, known, nullptr, true);
}
extern "C" int tsd_session_inpaint_active(tsd_session* s) { return s ? (s->uploaded && s->slot[0].inpaint ? 1 : 0) : TSD_E_ARG; }

extern "C" int tsd_session_decode(tsd_session* s) {
  NOTNULL(s);
  SESSION_NOT_SLOTS(s, "decode()");
  if (!s->dec) TSD_FAIL(TSD_E_STATE, "session: created without a decoder");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before decode()");
  SESSION_NOT_POISONED(s);
  TSD_TRY(session_options_unchanged(s, "upload()"));
  s->ctx->arena.top = 0;
  int r = g_decoder_forward(s->dec, s->latents, s->B, s->LH, s->LW, s->images);
  s->ctx->arena.top = 0;
  if (r == TSD_OK) s->decoded = true;
  return r;
}

extern "C" int tsd_session_download_latents(tsd_session* s, float* latents) {
  NOTNULL(s); NOTNULL(latents);
  SESSION_NOT_SLOTS(s, "download_latents()");
  if (!s->uploaded) TSD_FAIL(TSD_E_STATE, "session: upload() before download_latents() (the state is not defined yet)");
  return session_fetch_latents(s, s->latents, (size_t)s->B * 4 * s->LH * s->LW, latents);
}

extern "C" int tsd_session_download_images(tsd_session* s, int rescale_0_255, float* images) {
  NOTNULL(s); NOTNULL(images);
  SESSION_NOT_SLOTS(s, "download_images()");
  if (!s->dec) TSD_FAIL(TSD_E_STATE, "session: created without a decoder");
  if (!s->decoded) TSD_FAIL(TSD_E_STATE, "session: decode() before download_images() (no image has been computed since upload())");
  tsd_ctx* ctx = s->ctx;
  const int64_t n = (int64_t)s->B * 3 * 64 * s->LH * s->LW;
  const float* src = s->images;
  if (rescale_0_255) {  // pipeline.mojo:127
    TSD_TRY(ctx_reserve_staging(ctx, (size_t)n * 4));
    TSD_TRY(launch_unary_f32(ctx, 2, s->images, n, (float*)ctx->staging));
    src = (const float*)ctx->staging;
  }
  HIP_TRY(hipMemcpyAsync(images, src, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  const int r = ctx_check_status(ctx);
  if (r != TSD_OK) return r;
  SESSION_NOT_POISONED(s);
  // a non-finite IMAGE is reported, it does not poison latents that may be fine (decode again after the cause is removed)
  if (!host_all_finite(images, (size_t)n)) TSD_FAIL(TSD_E_NONFINITE, "session: inf / NaN in the decoded images");
  return TSD_OK;
}

// ---- slot sessions: the body of `pipeline.generate`'s loop (pipeline.mojo:86-124), per sample ---------------------------------------
// Every sample of the session is a slot with its own request (context, seed, guidance scale) and its own index into the session's
// timestep list.  advance() runs ONE forward over all Bu samples and one update launch whose per-sample table gives each active slot
// the step of its own index; a finished slot is refilled by slot_start while the others keep going.  What the lockstep step() passes
// as scalars for the whole batch is the same plan (entry 0 of the tables session_step_tables fills for both), and applied by the same per-element functions
// (update_element.h): a slot's latents are bit for bit those of a lockstep session of the same batch shape running its request.
extern "C" int tsd_session_slots_open(tsd_session* s) {
  NOTNULL(s);
  if (s->cn) TSD_FAIL(TSD_E_STATE, "session: slots_open() on a session with a ControlNet (per-slot control is not supported); set_control(NULL) first");
  if (s->ip) TSD_FAIL(TSD_E_STATE, "session: slots_open() on a session with an IP-Adapter (per-slot adapters are not supported); set_ip_adapter(NULL) first");
  tsd_ctx* ctx = s->ctx;
  HIP_TRY(hipSetDevice(ctx->device));
  const int B = s->B, Bu = s->Bu;
  s->slots = false;
  s->has_noise = false;
  // idle slots ride through every forward: zero latents and a zero context keep them finite
  HIP_TRY(hipMemsetAsync(s->latents, 0, (size_t)B * 4 * s->LH * s->LW * 4, ctx->stream));
  HIP_TRY(hipMemsetAsync(s->ctx16, 0, (size_t)Bu * s->Tp * s->W * 2, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (ctx->opt.session_hoist)  // the per-sample time rows of an advance: sized by the session's shape alone
    TSD_TRY(session_grow(ctx, (void**)&s->trows, &s->trows_cap, (size_t)Bu * s->unet->unet.tproj.N * 4, "time rows"));
  // the planning pass and the hoist buffers of upload(), K / V^T of the zero context, the whole time table; every slot idle, no request
  TSD_TRY(session_prepare(s));
  s->uploaded = false;  // the lockstep entry points stay closed
  s->slots = true;
  return TSD_OK;
}

extern "C" int tsd_session_slot_start(tsd_session* s, int b, const float* context, const float* uncond_context, const float* latents,
                                      int noise_at_start, uint64_t seed, int start_index, float cfg_scale) {
  NOTNULL(s); NOTNULL(context);
  SESSION_IN_SLOTS(s);
  SESSION_NOT_POISONED(s);
  tsd_ctx* ctx = s->ctx;
  const int B = s->B, T = s->T, Tp = s->Tp;
  const size_t chw = (size_t)4 * s->LH * s->LW, nc = (size_t)T * s->W;
  // every refusal comes before the first copy: a refused call leaves the slot, and everyone else's, as it was
  SLOT_IN_RANGE(s, b);
  if (start_index < 0 || start_index >= (int)s->timesteps.size())
    TSD_FAIL(TSD_E_ARG, "session: start index %d out of range (0..%d)", start_index, (int)s->timesteps.size() - 1);
  if (s->cfg && !uncond_context) TSD_FAIL(TSD_E_ARG, "session: a slot of a CFG session needs uncond_context");
  if (!host_all_finite(&cfg_scale, 1)) TSD_FAIL(TSD_E_ARG, "session: cfg_scale of slot_start() is not finite");
  if (!host_all_finite(context, nc)) TSD_FAIL(TSD_E_ARG, "session: inf / NaN in the context of slot_start()");
  if (s->cfg && !host_all_finite(uncond_context, nc)) TSD_FAIL(TSD_E_ARG, "session: inf / NaN in the uncond_context of slot_start()");
  if (latents && !host_all_finite(latents, chw)) TSD_FAIL(TSD_E_ARG, "session: inf / NaN in the latents of slot_start()");
  HIP_TRY(hipSetDevice(ctx->device));
  TSD_TRY(ctx_reserve_staging(ctx, std::max(nc, chw) * 4));
  tsd_session::Slot& sl = s->slot[b];
  session_reset_requests(s, b, 1);  // idle until the request is in place; a refilled slot inherits no mask, rescale or history
  // context rows b and B + b: upload()'s conversion, one sample
  for (int part = 0; part < (s->cfg ? 2 : 1); part++)
    TSD_TRY(session_put_context(s, part == 0 ? context : uncond_context, (size_t)part * B + b, 1));
  // Under the hoist only this sample's K / V^T change: the forward's own projection at batch 1, into the sample's region.  The GEMM's
  // summation tree keys on the layer, never on the batch (gemm_plan.cpp), so these are the bits of the all-sample build.  After a
  // parameter change the next advance() rebuilds every sample from ctx16, this one included.
  if (s->hoist && s->model_gen == s->unet->gen) {
    const int CK = s->unet->unet.kproj_all.N;
    for (int part = 0; part < (s->cfg ? 2 : 1); part++) {
      const size_t row = (size_t)part * B + b;
      ctx->arena.top = 0;
      TSD_TRY(g_unet_ctx_kv(s->unet, s->ctx16 + row * Tp * s->W, Tp, 1, s->kc_all + row * Tp * CK, s->vtc_all + row * CK * Tp));
    }
    ctx->arena.top = 0;
  }
  float* lat = s->latents + (size_t)b * chw;
  NormalBases nb = {};
  if (!latents) {  // seed_latents()' rule for one sample: stream 2 of the seed
    nb.base[0] = counter_rng_base(seed, NOISE_STREAM_LATENTS);
    TSD_TRY(launch_fill_normal(ctx, lat, (int64_t)chw, (int64_t)chw, nb, 0));
  } else {
    HIP_TRY(hipMemcpyAsync(lat, latents, chw * 4, hipMemcpyHostToDevice, ctx->stream));
    if (noise_at_start) {  // add_noise_seeded(start_index) on this slot: stream 4 of the seed, the same scalars, the same kernel
      nb.base[0] = counter_rng_base(seed, NOISE_STREAM_ADD);
      TSD_TRY(launch_fill_normal(ctx, (float*)ctx->staging, (int64_t)chw, (int64_t)chw, nb, 0));
      TSD_TRY(session_add_noise(s, start_index, lat, (int64_t)chw, (const float*)ctx->staging));
    }
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));  // the host tensors and the staging buffer are free again on return
  sl.index = start_index; sl.cfg_scale = cfg_scale; sl.seed = seed;
  sl.state = 1;
  return TSD_OK;
}

// Inpainting for the request of ACTIVE slot b, right after slot_start or mid-flight: what set_inpaint_seeded does for sample b of a
// lockstep session, on this sample's regions of the three buffers alone.  mask [LH][LW], known [4][LH][LW]; the noise is stream 4 of the slot's
// seed, the values slot_start(noise_at_start) added.  mask == NULL turns it off.  Either way the slot's history is dropped, as set_inpaint
// drops the session's.  Every refusal comes before the first copy and leaves all slots as they were.  Synchronous.
extern "C" int tsd_session_slot_set_inpaint(tsd_session* s, int b, const float* mask, const float* known) {
  NOTNULL(s);
  SESSION_IN_SLOTS(s);
  SLOT_IN_RANGE(s, b);
  SLOT_IS_ACTIVE(s, b, "slot_set_inpaint()");
  tsd_session::Slot& sl = s->slot[b];
  if (mask) {
    NOTNULL(known);
    NormalBases nb = {};
    nb.base[0] = counter_rng_base(sl.seed, NOISE_STREAM_ADD);
    TSD_TRY(session_put_inpaint(s, b, 1, mask, known, nullptr, &nb, "slot_set_inpaint()"));
  }
  sl.inpaint = mask != nullptr;
  sl.hist_valid = false;  // the steps that follow run on other latents than the history was predicted for
  return TSD_OK;
}
extern "C" int tsd_session_slot_inpaint_active(tsd_session* s, int b) {
  NOTNULL(s);
  SESSION_IN_SLOTS(s);
  SLOT_IN_RANGE(s, b);
  return s->slot[b].state == 1 && s->slot[b].inpaint ? 1 : 0;
}

// Guidance rescale for the request of ACTIVE slot b, like cfg_scale per request.  Only a flag of the advances that follow: the slot's
// latents and history stay what they are.
extern "C" int tsd_session_slot_set_guidance_rescale(tsd_session* s, int b, float phi) {
  NOTNULL(s);
  SESSION_IN_SLOTS(s);
  SLOT_IN_RANGE(s, b);
  SLOT_IS_ACTIVE(s, b, "slot_set_guidance_rescale()");
  if (!s->cfg) TSD_FAIL(TSD_E_STATE, "session: guidance rescale needs a session created with cfg != 0");
  TSD_TRY(rescale_phi_ok(phi));
  s->slot[b].rescale = phi;
  return TSD_OK;
}
extern "C" int tsd_session_slot_guidance_rescale(tsd_session* s, int b, float* phi) {
  NOTNULL(s); NOTNULL(phi);
  SESSION_IN_SLOTS(s);
  SLOT_IN_RANGE(s, b);
  *phi = s->slot[b].state == 1 ? s->slot[b].rescale : 0.f;
  return TSD_OK;
}

extern "C" int tsd_session_advance(tsd_session* s, uint32_t* finished_mask) {
  NOTNULL(s);
  SESSION_IN_SLOTS(s);
  SESSION_NOT_POISONED(s);
  TSD_TRY(session_options_unchanged(s, "slots_open()"));
  tsd_ctx* ctx = s->ctx;
  const int B = s->B, Bu = s->Bu, n = (int)s->timesteps.size();
  if (!tsd_session_slots_active(s)) TSD_FAIL(TSD_E_STATE, "session: advance() with no active slot");
  int idx[16];  // each slot's own index; an idle or finished slot is inactive
  bool hist_valid[16];
  for (int b = 0; b < B; b++) {
    idx[b] = s->slot[b].state == 1 ? s->slot[b].index : -1;
    hist_valid[b] = s->slot[b].hist_valid;
  }
  TSD_TRY(session_refresh(s));
  // the tables, built before anything is enqueued: the per-slot scalars travel as kernel arguments
  StepTables t;
  TSD_TRY(session_step_tables(s, idx, hist_valid, &t));
  // per-sample time rows (cond and uncond halves alike); an idle or finished slot reads entry 0
  UNetPre pre;
  if (s->hoist) {
    SlotRows rows = {};
    for (int b = 0; b < Bu; b++) rows.row[b] = std::max(idx[b % B], 0);
    const int N = s->unet->unet.tproj.N;
    TSD_TRY(launch_slot_time_rows(ctx, s->ttab, N, rows, Bu, s->trows));
    pre.tvec = s->trows; pre.tld = N; pre.kc_all = s->kc_all; pre.vtc_all = s->vtc_all;
  } else {
    SlotTimes ts = {};
    for (int b = 0; b < Bu; b++) ts.t[b] = (float)s->timesteps[std::max(idx[b % B], 0)];
    TSD_TRY(launch_slot_timesteps(ctx, ts, Bu, s->tdev));
    TSD_TRY(launch_time_embedding(ctx, s->tdev, 0.f, Bu, s->temb));
  }
  int eps_hw = 0;
  TSD_TRY(session_forward(s, &pre, &eps_hw));
  TSD_TRY(session_update(s, t, eps_hw, -1));
  uint32_t done = 0;
  for (int b = 0; b < B; b++) {
    tsd_session::Slot& sl = s->slot[b];
    if (sl.state != 1) continue;
    sl.hist_valid = (t.tab.e[b].flags & SLOT_HIST_OUT) != 0;
    if (++sl.index >= n) { sl.state = 2; done |= 1u << b; }
  }
  if (finished_mask) *finished_mask = done;
  return TSD_OK;
}

extern "C" int tsd_session_slot_state(tsd_session* s, int b, int* index, int* state) {
  NOTNULL(s);
  SESSION_IN_SLOTS(s);
  SLOT_IN_RANGE(s, b);
  if (index) *index = s->slot[b].index;
  if (state) *state = s->slot[b].state;
  return TSD_OK;
}

extern "C" int tsd_session_slot_download(tsd_session* s, int b, float* latents) {
  NOTNULL(s); NOTNULL(latents);
  SESSION_IN_SLOTS(s);
  SLOT_IN_RANGE(s, b);
  if (s->slot[b].state == 0) TSD_FAIL(TSD_E_STATE, "session: slot %d is idle (no request has defined its latents)", b);
  const size_t chw = (size_t)4 * s->LH * s->LW;
  return session_fetch_latents(s, s->latents + (size_t)b * chw, chw, latents);  // download_latents()' check, on this slot's buffer alone
}

extern "C" int tsd_session_slots_active(tsd_session* s) {
  if (!s) return TSD_E_ARG;
  int n = 0;
  if (s->slots)
    for (int b = 0; b < s->B; b++) n += s->slot[b].state == 1;
  return n;
}

// the raw latent buffer [B,4,LH,LW], whatever the mode and the slot states, unchecked: lets a test see that an idle slot is never written
extern "C" int tsd_debug_session_latents(tsd_session* s, float* latents) {
  NOTNULL(s); NOTNULL(latents);
  HIP_TRY(hipSetDevice(s->ctx->device));
  HIP_TRY(hipMemcpyAsync(latents, s->latents, (size_t)s->B * 4 * s->LH * s->LW * 4, hipMemcpyDeviceToHost, s->ctx->stream));
  HIP_TRY(hipStreamSynchronize(s->ctx->stream));
  return TSD_OK;
}
