// api_ops.cpp - op-level and block-level C-ABI entry points (host fp32 in/out, reference layouts).
// Each call uploads its operands, converts to the device layout (NHWC / K-major fp16), runs the same
// kernels the module path uses, converts back and synchronises - these are the parity/drop-in
// surface of the individual reference structs, not the measured path.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "graph.h"

namespace {
struct Dev {
  tsd_ctx* c;
  int err = TSD_OK;
  template <class T>
  T* buf(int64_t n) {
    T* d = arena_alloc<T>(c, n > 0 ? n : 1);
    if (!d && err == TSD_OK) { tsd_set_error("workspace arena exhausted"); err = TSD_E_ALLOC; }
    return d;
  }
  template <class T>
  T* in(const T* host, int64_t n) {
    T* d = buf<T>(n);
    if (d && c->launch() && err == TSD_OK) {
      hipError_t e = hipMemcpyAsync(d, host, (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream);
      if (e != hipSuccess) { tsd_set_error("H2D copy failed: %s", hipGetErrorString(e)); err = TSD_E_HIP; }
    }
    return d;
  }
  template <class T>
  int out(T* host, const T* dev, int64_t n) {
    if (err != TSD_OK) return err;
    if (c->launch()) HIP_TRY(hipMemcpyAsync(host, dev, (size_t)n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return TSD_OK;
  }
  int out2d(float* host, const float* dev, int rows, int cols, int ld) {
    if (err != TSD_OK) return err;
    if (c->launch())
      HIP_TRY(hipMemcpy2DAsync(host, (size_t)cols * 4, dev, (size_t)ld * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToHost,
                               c->stream));
    return TSD_OK;
  }
  int zero(void* p, size_t bytes) {
    if (c->launch()) HIP_TRY(hipMemsetAsync(p, 0, bytes, c->stream));
    return TSD_OK;
  }
  // pack host weights into the arena
  int conv(const float* w, const float* b, int O, int I, int k, int Opad, ConvW* o) {
    const int Ipad = round_up(I, 64);
    float* dw = in(w, (int64_t)O * I * k * k);
    half_t* pw = buf<half_t>((int64_t)Opad * k * k * Ipad);
    float* pb = buf<float>(Opad);
    if (err) return err;
    TSD_TRY(launch_pack_conv(c, dw, O, I, k, pw, Opad, Ipad));
    if (b) {
      float* db = in(b, O);
      if (err) return err;
      TSD_TRY(launch_pack_bias(c, db, O, pb, Opad, 0));
    } else TSD_TRY(zero(pb, (size_t)Opad * 4));
    o->w = pw; o->b = pb; o->I = I; o->O = O; o->k = k; o->Ipad = Ipad; o->Opad = Opad;
    return TSD_OK;
  }
  int lin(const float* w, const float* b, int N, int K, int interleave, LinW* o) {
    const int Kpad = round_up(K, 64), Npad = round_up(N, 4);
    float* dw = in(w, (int64_t)N * K);
    half_t* pw = buf<half_t>((int64_t)Npad * Kpad);
    if (err) return err;
    if (Npad != N) TSD_TRY(zero(pw + (int64_t)N * Kpad, (size_t)(Npad - N) * Kpad * 2));
    TSD_TRY(launch_pack_linear(c, dw, N, K, pw, Kpad, interleave));
    o->w = pw; o->N = N; o->K = K; o->Kpad = Kpad; o->b = nullptr;
    if (b) {
      float* db = in(b, N);
      float* pb = buf<float>(Npad);
      if (err) return err;
      TSD_TRY(launch_pack_bias(c, db, N, pb, Npad, interleave));
      o->b = pb;
    }
    return TSD_OK;
  }
};

template <class F>
int run_op(tsd_ctx* ctx, F&& fn) {
  if (!ctx) TSD_FAIL(TSD_E_ARG, "ctx is NULL");
  HIP_TRY(hipSetDevice(ctx->device));
  int r = run_planned(ctx, fn);
  if (r != TSD_OK) {
    hipStreamSynchronize(ctx->stream);
    return r;
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return ctx_check_status(ctx);  // split-K hand-off time-outs, non-finite outputs (fp16 overflow): never silent
}
}  // namespace

// Every entry point opens with NOTNULL(p) on its pointer arguments: TSD_E_ARG and the argument's name in tsd_last_error.
// The macro is in graph.h; the replay entries (api_replay.cpp) use it as well.

extern "C" int tsd_conv2d_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, const float* w, const float* bias,
                              int I, int O, int k, int pad_h, int pad_w, int stride_h, int stride_w, float* y) {
  NOTNULL(x); NOTNULL(w); NOTNULL(y);
  if (C <= 0 || H <= 0 || W <= 0 || O <= 0 || I <= 0 || I > C) TSD_FAIL(TSD_E_SHAPE, "conv2d: bad dims C=%d I=%d O=%d", C, I, O);
  if (k != 1 && k != 3) TSD_FAIL(TSD_E_SHAPE, "conv2d: kernel size %d unsupported (1 or 3)", k);
  if (pad_h != pad_w || stride_h != stride_w || stride_h < 1 || pad_h < 0)
    TSD_FAIL(TSD_E_SHAPE, "conv2d: only square padding/stride are on the path");
  if (k == 1 && (pad_h != 0 || stride_h != 1)) TSD_FAIL(TSD_E_SHAPE, "conv2d: 1x1 conv with padding/stride unsupported");
  const int Ho = (H + 2 * pad_h - k) / stride_h + 1, Wo = (W + 2 * pad_w - k) / stride_w + 1;
  if (Ho <= 0 || Wo <= 0) TSD_FAIL(TSD_E_SHAPE, "conv2d: empty output");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    const int Opad = round_up(O, 4);
    ConvW cw;
    TSD_TRY(d.conv(w, bias, O, I, k, Opad, &cw));
    float* dx = d.in(x, (int64_t)C * H * W);
    Act xa = act_alloc(ctx, 1, H, W, cw.Ipad);
    float* y32 = d.buf<float>((int64_t)Ho * Wo * Opad);
    float* ychw = d.buf<float>((int64_t)O * Ho * Wo);
    if (d.err || !xa.p) return d.err ? d.err : TSD_E_ALLOC;
    TSD_TRY(launch_chw_f32_to_nhwc_f16(ctx, dx, 1, C, H, W, I, 1.f, xa.p, cw.Ipad));
    if (k == 3) TSD_TRY(g_conv3x3(ctx, xa, cw, stride_h, pad_h, pad_h, 0, nullptr, 0, nullptr, 0, true, y32, Opad));
    else {
      GemmArgs g;
      g.A0 = xa.p; g.lda0 = xa.ld; g.Wt = cw.w; g.ldw = cw.Ipad; g.M = H * W; g.N = Opad; g.K = cw.Ipad;
      g.epi = EPI_BIAS_N | EPI_OUT_F32; g.bias = cw.b; g.C = y32; g.ldc = Opad;
      TSD_TRY(launch_gemm(ctx, g));
    }
    TSD_TRY(launch_nhwc_f32_to_chw_f32(ctx, y32, 1, O, Ho, Wo, Opad, ychw));
    return d.out(y, ychw, (int64_t)O * Ho * Wo);
  });
}

extern "C" int tsd_pad_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int top, int bottom, int left, int right,
                           float* y) {
  NOTNULL(x); NOTNULL(y);
  if (C <= 0 || H <= 0 || W <= 0 || top < 0 || bottom < 0 || left < 0 || right < 0) TSD_FAIL(TSD_E_SHAPE, "pad: bad dims");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    const int64_t n_out = (int64_t)C * (H + top + bottom) * (W + left + right);
    float* dx = d.in(x, (int64_t)C * H * W);
    float* dy = d.buf<float>(n_out);
    if (d.err) return d.err;
    TSD_TRY(launch_pad_f32(ctx, dx, C, H, W, top, bottom, left, right, dy));
    return d.out(y, dy, n_out);
  });
}

extern "C" int tsd_groupnorm_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int groups, int num_channels,
                                 float eps, float gamma, float* y) {
  NOTNULL(x); NOTNULL(y);
  // reference checks, helpers/utils.mojo:1847-1853 ("Returning null matrix")
  if (num_channels > C) TSD_FAIL(TSD_E_SHAPE, "groupnorm: num_channels %d exceeds input channels %d", num_channels, C);
  if (groups <= 0 || num_channels % groups) TSD_FAIL(TSD_E_SHAPE, "groupnorm: %d channels not divisible by %d groups", num_channels, groups);
  if (num_channels % 8) TSD_FAIL(TSD_E_SHAPE, "groupnorm: num_channels %d must be a multiple of 8 on the device path", num_channels);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    const int Cn = num_channels;
    float* dx = d.in(x, (int64_t)C * H * W);
    half_t* x16 = d.buf<half_t>((int64_t)H * W * Cn);
    half_t* y16 = d.buf<half_t>((int64_t)H * W * Cn);
    float* dy = d.buf<float>((int64_t)Cn * H * W);
    if (d.err) return d.err;
    TSD_TRY(launch_chw_f32_to_nhwc_f16(ctx, dx, 1, C, H, W, Cn, 1.f, x16, Cn));
    NormSrc s; s.x0 = x16; s.ld0 = Cn; s.C0 = Cn;
    TSD_TRY(launch_groupnorm(ctx, s, 1, H * W, Cn, groups, eps, gamma, 0, y16, Cn));
    TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, y16, 1, Cn, H, W, Cn, dy));
    return d.out(y, dy, (int64_t)Cn * H * W);
  });
}

extern "C" int tsd_layernorm_f32(tsd_ctx* ctx, const float* x, int M, int C, float eps, float* y) {
  NOTNULL(x); NOTNULL(y);
  if (M <= 0 || C <= 0 || C % 8) TSD_FAIL(TSD_E_SHAPE, "layernorm: C=%d must be a positive multiple of 8", C);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, (int64_t)M * C);
    half_t* x16 = d.buf<half_t>((int64_t)M * C);
    half_t* y16 = d.buf<half_t>((int64_t)M * C);
    float* dy = d.buf<float>((int64_t)M * C);
    if (d.err) return d.err;
    TSD_TRY(launch_f32_to_f16_rows(ctx, dx, M, C, x16, C, M));
    TSD_TRY(launch_layernorm(ctx, x16, M, C, C, eps, y16, C));
    TSD_TRY(launch_f16_to_f32_rows(ctx, y16, M, C, C, dy));
    return d.out(y, dy, (int64_t)M * C);
  });
}

extern "C" int tsd_groupnorm_affine_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, int groups, float eps,
                                        const float* weight, const float* bias, int silu, float* y) {
  NOTNULL(x); NOTNULL(y);
  if (groups <= 0 || C % groups) TSD_FAIL(TSD_E_SHAPE, "groupnorm: %d channels not divisible by %d groups", C, groups);
  if (C % 8) TSD_FAIL(TSD_E_SHAPE, "groupnorm: C=%d must be a multiple of 8 on the device path", C);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, (int64_t)C * H * W);
    float* dw = weight ? d.in(weight, C) : nullptr;
    float* db = bias ? d.in(bias, C) : nullptr;
    half_t* x16 = d.buf<half_t>((int64_t)H * W * C);
    half_t* y16 = d.buf<half_t>((int64_t)H * W * C);
    float* dy = d.buf<float>((int64_t)C * H * W);
    if (d.err) return d.err;
    TSD_TRY(launch_chw_f32_to_nhwc_f16(ctx, dx, 1, C, H, W, C, 1.f, x16, C));
    NormSrc s; s.x0 = x16; s.ld0 = C; s.C0 = C;
    NormAffine a; a.w = dw; a.b = db; a.torch_rstd = 1;
    TSD_TRY(launch_groupnorm(ctx, s, 1, H * W, C, groups, eps, 1.f, silu ? 1 : 0, y16, C, nullptr, 0, &a));
    TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, y16, 1, C, H, W, C, dy));
    return d.out(y, dy, (int64_t)C * H * W);
  });
}

extern "C" int tsd_layernorm_affine_f32(tsd_ctx* ctx, const float* x, int M, int C, float eps, const float* weight,
                                        const float* bias, float* y) {
  NOTNULL(x); NOTNULL(y);
  if (M <= 0 || C <= 0 || C % 8) TSD_FAIL(TSD_E_SHAPE, "layernorm: C=%d must be a positive multiple of 8", C);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, (int64_t)M * C);
    float* dw = weight ? d.in(weight, C) : nullptr;
    float* db = bias ? d.in(bias, C) : nullptr;
    half_t* x16 = d.buf<half_t>((int64_t)M * C);
    half_t* y16 = d.buf<half_t>((int64_t)M * C);
    float* dy = d.buf<float>((int64_t)M * C);
    if (d.err) return d.err;
    TSD_TRY(launch_f32_to_f16_rows(ctx, dx, M, C, x16, C, M));
    NormAffine a; a.w = dw; a.b = db; a.torch_rstd = 1;
    TSD_TRY(launch_layernorm(ctx, x16, M, C, C, eps, y16, C, &a));
    TSD_TRY(launch_f16_to_f32_rows(ctx, y16, M, C, C, dy));
    return d.out(y, dy, (int64_t)M * C);
  });
}

static int unary_op(tsd_ctx* ctx, int op, const float* x, int64_t n, float* y) {
  if (!x || !y) TSD_FAIL(TSD_E_ARG, "unary op: NULL argument");
  if (n <= 0) TSD_FAIL(TSD_E_SHAPE, "unary op: n=%lld", (long long)n);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, n);
    float* dy = d.buf<float>(n);
    if (d.err) return d.err;
    TSD_TRY(launch_unary_f32(ctx, op, dx, n, dy));
    return d.out(y, dy, n);
  });
}
extern "C" int tsd_silu_f32(tsd_ctx* ctx, const float* x, int64_t n, float* y) { return unary_op(ctx, 0, x, n, y); }
extern "C" int tsd_gelu_tanh_f32(tsd_ctx* ctx, const float* x, int64_t n, float* y) { return unary_op(ctx, 1, x, n, y); }
extern "C" int tsd_rescale_images_f32(tsd_ctx* ctx, const float* x, int64_t n, float* y) { return unary_op(ctx, 2, x, n, y); }

// one update of the linear-multistep samplers (kernels_sampler.hip) on host tensors: the kernel the denoise session launches
extern "C" int tsd_sampler_step_f32(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                                    const float* hist, const float* noise, int64_t n, const float* c, float* x_out,
                                    float* hist_out) {
  NOTNULL(x); NOTNULL(eps); NOTNULL(c); NOTNULL(x_out);
  if (n <= 0) TSD_FAIL(TSD_E_SHAPE, "sampler step: n=%lld", (long long)n);
  const SamplerCoeffs sc = {c[0], c[1], c[2], c[3], c[4], c[5]};
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, n);
    float* de = d.in(eps, n);
    float* du = eps_uncond ? d.in(eps_uncond, n) : nullptr;
    float* dh = hist ? d.in(hist, n) : nullptr;
    float* dz = noise ? d.in(noise, n) : nullptr;
    float* dy = d.buf<float>(n);
    float* dho = hist_out ? d.buf<float>(n) : nullptr;
    if (d.err) return d.err;
    TSD_TRY(launch_sampler_step(ctx, dx, de, du, cfg_scale, dh, dz, n, sc, 0, dy, dho));
    if (hist_out) TSD_TRY(d.out(hist_out, dho, n));
    return d.out(x_out, dy, n);
  });
}

// one update of a v-prediction session (kernels_vpred.hip k_sampler_step_v) on host tensors: tsd_sampler_step_f32's twin
extern "C" int tsd_sampler_step_v_f32(tsd_ctx* ctx, const float* x, const float* v, const float* v_uncond, float cfg_scale,
                                      const float* hist, const float* noise, int64_t n, const float* c, float* x_out,
                                      float* hist_out) {
  NOTNULL(x); NOTNULL(v); NOTNULL(c); NOTNULL(x_out);
  if (n <= 0) TSD_FAIL(TSD_E_SHAPE, "sampler step (v): n=%lld", (long long)n);
  const SamplerCoeffs sc = {c[0], c[1], c[2], c[3], c[4], c[5]};
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, n);
    float* dv = d.in(v, n);
    float* du = v_uncond ? d.in(v_uncond, n) : nullptr;
    float* dh = hist ? d.in(hist, n) : nullptr;
    float* dz = noise ? d.in(noise, n) : nullptr;
    float* dy = d.buf<float>(n);
    float* dho = hist_out ? d.buf<float>(n) : nullptr;
    if (d.err) return d.err;
    TSD_TRY(launch_sampler_step_v(ctx, dx, dv, du, cfg_scale, dh, dz, n, sc, 0, dy, dho));
    if (hist_out) TSD_TRY(d.out(hist_out, dho, n));
    return d.out(x_out, dy, n);
  });
}

// the update of step i of a DDPM session (kernels_elementwise.hip k_ddpm_step, the scalars of sampler_step_plan) on host tensors;
// like the session, the noise is added only on a step that does not land on t = 0
extern "C" int tsd_ddpm_step_f32(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                                 const float* noise, int64_t n, int spacing, int n_train, int n_infer, int start_step, int i,
                                 float* x_out) {
  NOTNULL(x); NOTNULL(eps); NOTNULL(x_out);
  if (n <= 0) TSD_FAIL(TSD_E_SHAPE, "ddpm step: n=%lld", (long long)n);
  std::vector<int> ts;
  TSD_TRY(sampler_timesteps(spacing, n_train, n_infer, start_step, ts));
  std::vector<float> ac;
  sampler_alphas_cumprod(n_train, ac);
  SlotEntry p;
  TSD_TRY(sampler_step_plan(TSD_SAMPLER_DDPM, 0.0, spacing, n_train, n_infer, ac, ts, i, false, TSD_PRED_EPSILON, &p));
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, n);
    float* de = d.in(eps, n);
    float* du = eps_uncond ? d.in(eps_uncond, n) : nullptr;
    float* dz = (noise && (p.flags & SLOT_NOISE)) ? d.in(noise, n) : nullptr;
    if (d.err) return d.err;
    TSD_TRY(launch_ddpm_step(ctx, dx, de, du, cfg_scale, dz, n, p.c[0], p.c[1], p.c[2], p.c[3], p.c[4], 0));
    return d.out(x_out, dx, n);
  });
}

// guidance rescale (kernels_guidance.hip) on host tensors: the two launches a session with tsd_session_set_guidance_rescale adds to a step
extern "C" int tsd_cfg_rescale_f32(tsd_ctx* ctx, const float* eps, const float* eps_uncond, int B, int64_t chw, const float* cfg_scale,
                                   const float* phi, float* eps_out, float* eps_uncond_out, float* g_out) {
  NOTNULL(eps); NOTNULL(eps_uncond); NOTNULL(cfg_scale); NOTNULL(phi); NOTNULL(eps_out); NOTNULL(eps_uncond_out);
  if (B <= 0 || B > 16 || chw <= 0) TSD_FAIL(TSD_E_SHAPE, "cfg rescale: B=%d (1..16) chw=%lld", B, (long long)chw);
  CfgRescaleTable tab = {};
  for (int b = 0; b < B; b++) {
    if (!(phi[b] >= 0.f && phi[b] <= 1.f)) TSD_FAIL(TSD_E_ARG, "cfg rescale: phi[%d] = %g is not in [0, 1]", b, (double)phi[b]);
    if (!(fabsf(cfg_scale[b]) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "cfg rescale: cfg_scale[%d] is not finite", b);
    tab.e[b].on = phi[b] > 0.f;
    tab.e[b].cfg_scale = cfg_scale[b];
    tab.e[b].phi = phi[b];
  }
  const int64_t n = (int64_t)B * chw;
  float ones[16];
  for (int b = 0; b < 16; b++) ones[b] = 1.f;
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dc = d.in(eps, n);
    float* du = d.in(eps_uncond, n);
    float* dg = d.in(ones, B);  // a sample with phi = 0 is not touched: its g stays 1
    double* part = d.buf<double>(CFG_RESCALE_PARTIAL_DOUBLES);
    if (d.err) return d.err;
    TSD_TRY(launch_cfg_rescale(ctx, dc, du, tab, B, chw, part, dg));
    if (g_out) TSD_TRY(d.out(g_out, dg, B));
    TSD_TRY(d.out(eps_uncond_out, du, n));
    return d.out(eps_out, dc, n);
  });
}

// ControlNet injection (kernels_control.hip) on host fp16 tensors: the ONE launch a controlled UNet forward adds, over a table of n tensors.
// x[i] / r[i] / y_out[i]: fp16 bits [B][HW[i]][C[i]]; partial_out[i]: fp32 [B][nslab[i]][groups[i]][2], ignored (may be NULL) for an entry
// with groups[i] == 0 - that entry gets no statistics.  Every sample is computed, a scale of exactly 0 included.
extern "C" int tsd_control_inject_f16(tsd_ctx* ctx, int n, const void* const* x, const void* const* r, int B, const int* HW, const int* C,
                                      const int* groups, const int* nslab, const float* scale, void* const* y_out, float* const* partial_out) {
  NOTNULL(ctx); NOTNULL(x); NOTNULL(r); NOTNULL(HW); NOTNULL(C); NOTNULL(groups); NOTNULL(nslab); NOTNULL(scale); NOTNULL(y_out);
  if (n <= 0 || n > CONTROL_MAX_ENTRIES || B <= 0 || B > 16) TSD_FAIL(TSD_E_SHAPE, "control inject: %d entries (1..%d), B=%d (1..16)", n, CONTROL_MAX_ENTRIES, B);
  for (int i = 0; i < n; i++) {
    if (!x[i] || !r[i] || !y_out[i]) TSD_FAIL(TSD_E_ARG, "control inject: entry %d: x, r and y_out are required", i);
    if (HW[i] <= 0 || C[i] <= 0 || groups[i] < 0 || nslab[i] <= 0) TSD_FAIL(TSD_E_SHAPE, "control inject: entry %d: HW=%d C=%d groups=%d nslab=%d", i, HW[i], C[i], groups[i], nslab[i]);
    if (groups[i] > 0 && (!partial_out || !partial_out[i])) TSD_FAIL(TSD_E_ARG, "control inject: entry %d has groups but no partial_out", i);
  }
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    ControlTable tab = {};
    tab.n = n;
    float* ds = d.in(scale, B);
    float* dp[CONTROL_MAX_ENTRIES] = {};
    for (int i = 0; i < n; i++) {
      ControlEntry& e = tab.e[i];
      const int64_t ne = (int64_t)B * HW[i] * C[i];
      e.x = (half_t*)d.in((const uint16_t*)x[i], ne);
      e.r = (const half_t*)d.in((const uint16_t*)r[i], ne);
      if (groups[i] > 0) dp[i] = d.buf<float>((int64_t)B * nslab[i] * groups[i] * 2);
      e.part = dp[i];
      e.ldx = e.ldr = e.C = C[i]; e.HW = HW[i]; e.groups = groups[i]; e.nslab = nslab[i];
    }
    if (d.err) return d.err;
    TSD_TRY(launch_control_inject(ctx, tab, B, ds));
    for (int i = 0; i < n; i++) {
      TSD_TRY(d.out((uint16_t*)y_out[i], (const uint16_t*)tab.e[i].x, (int64_t)B * HW[i] * C[i]));
      if (dp[i]) TSD_TRY(d.out(partial_out[i], (const float*)dp[i], (int64_t)B * nslab[i] * groups[i] * 2));
    }
    return TSD_OK;
  });
}

// IP-Adapter's decoupled cross attention (kernels_ipattn.hip) on host fp16 tensors: the ONE launch an adapted attention block adds.
// q / o [B][S][H*d], k_ip [B][16][H*d], vt_ip [B][H*d][16], scale [B]; o_out receives o updated in place on the device.
extern "C" int tsd_ip_attn_add_f16(tsd_ctx* ctx, const void* q, const void* k_ip, const void* vt_ip, const void* o, const float* scale, int B,
                                   int H, int d, int S, int N, float softmax_scale, void* o_out) {
  NOTNULL(ctx); NOTNULL(q); NOTNULL(k_ip); NOTNULL(vt_ip); NOTNULL(o); NOTNULL(scale); NOTNULL(o_out);
  if (B <= 0 || B > 16 || H <= 0 || H > 64 || d <= 0 || d > 1024 || S <= 0 || S > (1 << 20)) TSD_FAIL(TSD_E_SHAPE, "ip attention: B=%d (1..16) H=%d d=%d S=%d", B, H, d, S);
  return run_op(ctx, [&]() -> int {
    Dev dv{ctx};
    const int C = H * d;
    const int64_t nq = (int64_t)B * S * C, nk = (int64_t)B * IP_MAX_TOKENS * C;
    IpAttnArgs a;
    a.Q = (const half_t*)dv.in((const uint16_t*)q, nq); a.ldq = C; a.sQ = (int64_t)S * C;
    a.K = (const half_t*)dv.in((const uint16_t*)k_ip, nk); a.ldk = C; a.sK = (int64_t)IP_MAX_TOKENS * C;
    a.Vt = (const half_t*)dv.in((const uint16_t*)vt_ip, nk); a.ldvt = IP_MAX_TOKENS; a.sVt = (int64_t)C * IP_MAX_TOKENS;
    a.O = (half_t*)dv.in((const uint16_t*)o, nq); a.ldo = C; a.sO = (int64_t)S * C;
    a.s = dv.in(scale, B);
    a.B = B; a.H = H; a.d = d; a.S = S; a.N = N; a.scale = softmax_scale;
    if (dv.err) return dv.err;
    TSD_TRY(launch_ip_attn_add(ctx, a));
    return dv.out((uint16_t*)o_out, (const uint16_t*)a.O, nq);
  });
}

// FreeU (kernels_freeu.hip) on host fp16 tensors: the launch a decoder block with an active table entry adds (two in the modulated mode).
// h [B][H][W][Ch], r [B][H][W][Cr]; h_out / r_out receive the tensors as the launch left them.
extern "C" int tsd_freeu_f16(tsd_ctx* ctx, const void* h, const void* r, int B, int H, int W, int Ch, int Cr, float b, float s, int mode,
                             void* h_out, void* r_out) {
  NOTNULL(ctx);
  if (!h != !h_out || !r != !r_out || (!h && !r)) TSD_FAIL(TSD_E_ARG, "freeu: h / h_out and r / r_out are given in pairs, at least one pair");
  if (B <= 0 || B > 64 || H < 2 || W < 2 || H > 4096 || W > 4096) TSD_FAIL(TSD_E_SHAPE, "freeu: B=%d (1..64) plane %d x %d (sides 2..4096)", B, H, W);
  if ((h && (Ch <= 0 || Ch % 16)) || (r && (Cr <= 0 || Cr % 8))) TSD_FAIL(TSD_E_SHAPE, "freeu: Ch=%d (a multiple of 16) Cr=%d (a multiple of 8)", Ch, Cr);
  return run_op(ctx, [&]() -> int {
    Dev dv{ctx};
    const int64_t nh = (int64_t)B * H * W * Ch, nr = (int64_t)B * H * W * Cr;
    FreeuOp op;
    op.B = B; op.H = H; op.W = W; op.mode = mode;
    if (h) { op.h = (half_t*)dv.in((const uint16_t*)h, nh); op.Ch = op.ldh = Ch; op.b = b; }
    if (r) { op.r = (half_t*)dv.in((const uint16_t*)r, nr); op.Cr = op.ldr = Cr; op.s = s; }
    op.mean = dv.buf<float>((int64_t)B * H * W);
    if (dv.err) return dv.err;
    TSD_TRY(launch_freeu(ctx, op));
    if (h) TSD_TRY(dv.out((uint16_t*)h_out, (const uint16_t*)op.h, nh));
    if (r) TSD_TRY(dv.out((uint16_t*)r_out, (const uint16_t*)op.r, nr));
    return TSD_OK;
  });
}

extern "C" int tsd_debug_freeu_run(tsd_ctx* ctx, const void* h, const void* r, int B, int H, int W, int Ch, int Cr, int ldh, int ldr, int guard,
                                   float b, float s, int mode, void* h_out, void* r_out) {
  NOTNULL(ctx); NOTNULL(h); NOTNULL(r); NOTNULL(h_out); NOTNULL(r_out);
  if (B <= 0 || B > 64 || H < 2 || W < 2 || H > 4096 || W > 4096 || guard < 0 || guard % 8 || guard > (1 << 20))
    TSD_FAIL(TSD_E_SHAPE, "freeu run: B=%d (1..64) plane %d x %d (sides 2..4096) guard %d (a multiple of 8)", B, H, W, guard);
  if (Ch <= 0 || Ch % 16 || Cr <= 0 || Cr % 8 || ldh < Ch || ldr < Cr || ldh % 8 || ldr % 8 || ldh > 8192 || ldr > 8192)
    TSD_FAIL(TSD_E_SHAPE, "freeu run: Ch=%d (a multiple of 16) Cr=%d (a multiple of 8) pitches %d / %d", Ch, Cr, ldh, ldr);
  return run_op(ctx, [&]() -> int {
    Dev dv{ctx};
    const int64_t nh = (int64_t)B * H * W * ldh + 2 * guard, nr = (int64_t)B * H * W * ldr + 2 * guard;
    uint16_t* dh = dv.in((const uint16_t*)h, nh);
    uint16_t* dr = dv.in((const uint16_t*)r, nr);
    FreeuOp op;
    op.B = B; op.H = H; op.W = W; op.mode = mode;
    op.h = (half_t*)dh + guard; op.Ch = Ch; op.ldh = ldh; op.b = b;
    op.r = (half_t*)dr + guard; op.Cr = Cr; op.ldr = ldr; op.s = s;
    op.mean = dv.buf<float>((int64_t)B * H * W);
    if (dv.err) return dv.err;
    TSD_TRY(launch_freeu(ctx, op));
    TSD_TRY(dv.out((uint16_t*)h_out, (const uint16_t*)dh, nh));
    return dv.out((uint16_t*)r_out, (const uint16_t*)dr, nr);
  });
}

// The CLIP vision encoder's image front end (kernels_vision.hip) on host tensors: images fp32 [B][3][H][W] on 0 .. 255 -> patch rows fp16
// [B * 256][592], the ONE launch in front of the patch-embedding GEMM.
extern "C" int tsd_clip_image_patches_f16(tsd_ctx* ctx, const float* images, int B, int H, int W, void* patches_out) {
  NOTNULL(ctx); NOTNULL(images); NOTNULL(patches_out);
  if (B <= 0 || B > 64) TSD_FAIL(TSD_E_SHAPE, "clip image patches: B=%d (1..64)", B);
  if (H < 8 || W < 8 || H > 2048 || W > 2048) TSD_FAIL(TSD_E_SHAPE, "clip image patches: sides %d x %d outside 8 .. 2048", H, W);
  return run_op(ctx, [&]() -> int {
    Dev dv{ctx};
    const int64_t no = (int64_t)B * CV_PATCHES * CV_PATCH_LD;
    const float* di = dv.in(images, (int64_t)B * 3 * H * W);
    uint16_t* dp = dv.buf<uint16_t>(no);
    if (dv.err) return dv.err;
    TSD_TRY(launch_clip_image_patches(ctx, di, B, H, W, (half_t*)dp, CV_PATCH_LD));
    return dv.out((uint16_t*)patches_out, (const uint16_t*)dp, no);
  });
}

// N(0,1) of the counter RNG (kernels_sampler.hip k_fill_normal, counter_rng.h) on a host tensor: element e is value offset + e of the
// stream (seed, stream) - the values a seeded denoise session draws on the device
extern "C" int tsd_normal_fill_f32(tsd_ctx* ctx, uint64_t seed, uint64_t stream, uint64_t offset, int64_t n, float* out) {
  NOTNULL(ctx); NOTNULL(out);
  if (n <= 0) TSD_FAIL(TSD_E_SHAPE, "normal fill: n=%lld", (long long)n);
  NormalBases nb = {};
  nb.base[0] = counter_rng_base(seed, stream);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dy = d.buf<float>(n);
    if (d.err) return d.err;
    TSD_TRY(launch_fill_normal(ctx, dy, n, n, nb, offset));
    return d.out(out, dy, n);
  });
}

// inf / NaN or a value outside [lo, hi] in a host tensor (the argument scans of the masked-denoising entries)
static bool host_all_in_range(const float* p, size_t n, float lo, float hi) {
  bool ok = true;
  for (size_t i = 0; i < n; i++) ok &= (p[i] >= lo) & (p[i] <= hi);  // false for NaN
  return ok;
}

// pixel mask -> latent mask (kernels_sampler.hip k_latent_mask) on host tensors
extern "C" int tsd_latent_mask_hw_f32(tsd_ctx* ctx, const float* mask_px, int B, int LH, int LW, int mode, float* mask_lat) {
  NOTNULL(ctx); NOTNULL(mask_px); NOTNULL(mask_lat);
  if (mode != TSD_MASK_AREA && mode != TSD_MASK_ANY) TSD_FAIL(TSD_E_ARG, "latent mask: mode %d (0 area, 1 any)", mode);
  if (B <= 0 || LH <= 0 || LW <= 0) TSD_FAIL(TSD_E_SHAPE, "latent mask: B=%d L=%dx%d", B, LH, LW);
  const int64_t npx = (int64_t)B * 64 * LH * LW, nl = (int64_t)B * LH * LW;
  if (!host_all_in_range(mask_px, (size_t)npx, 0.f, 1.f)) TSD_FAIL(TSD_E_ARG, "latent mask: every mask value must be finite and in [0, 1]");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dm = d.in(mask_px, npx);
    float* dy = d.buf<float>(nl);
    if (d.err) return d.err;
    TSD_TRY(launch_latent_mask(ctx, dm, B, LH, LW, mode, dy));
    return d.out(mask_lat, dy, nl);
  });
}
extern "C" int tsd_latent_mask_f32(tsd_ctx* ctx, const float* mask_px, int B, int L, int mode, float* mask_lat) {
  return tsd_latent_mask_hw_f32(ctx, mask_px, B, L, L, mode, mask_lat);
}

// the masked-denoising blend (kernels_sampler.hip k_inpaint_blend) on host tensors: the launch a session with inpainting adds to a step.
// On the device the blend runs in place (x_out is x) when the host pointers are the same, as the session runs it.
extern "C" int tsd_inpaint_blend_f32(tsd_ctx* ctx, const float* x, const float* mask, const float* known, const float* noise, int B,
                                     int64_t hw, float a_prev, float s_prev, float* x_out) {
  NOTNULL(ctx); NOTNULL(x); NOTNULL(mask); NOTNULL(known); NOTNULL(x_out);
  if (B <= 0 || hw <= 0) TSD_FAIL(TSD_E_SHAPE, "inpaint blend: B=%d hw=%lld", B, (long long)hw);
  const int64_t n = (int64_t)B * 4 * hw;
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, n);
    float* dm = d.in(mask, (int64_t)B * hw);
    float* dk = d.in(known, n);
    float* dz = noise ? d.in(noise, n) : nullptr;
    float* dy = x_out == x ? dx : d.buf<float>(n);
    if (d.err) return d.err;
    TSD_TRY(launch_inpaint_blend(ctx, dx, dm, dk, dz, B, hw, a_prev, s_prev, dy));
    return d.out(x_out, dy, n);
  });
}

// the low-rank merge (kernels_lora.hip k_lora_merge) on host tensors: `w` is packed as a model packs it - launch_pack_linear for k = 0
// ([O][I], `interleave`: GEGLU rows), launch_pack_conv for k = 1, 3 ([O][I][k][k], Opad as model_spec.cpp pads a convolution) - merged in
// place by the kernel tsd_model_lora_add runs, and returned unpacked in the reference layout: every value of `out` is exactly an fp16.
extern "C" int tsd_lora_merge_f32(tsd_ctx* ctx, const float* w, int O, int I, int k, int interleave, int row0, int rows, const float* up,
                                  const float* down, int rank, float scale, float* out) {
  NOTNULL(ctx); NOTNULL(w); NOTNULL(up); NOTNULL(down); NOTNULL(out);
  if (k != 0 && k != 1 && k != 3) TSD_FAIL(TSD_E_ARG, "lora merge: kernel size %d (0 linear, 1 or 3)", k);
  if (rank < 1 || rank > 1024) TSD_FAIL(TSD_E_ARG, "lora merge: rank %d outside 1..1024", rank);
  if (!(fabsf(scale) <= 3.4028235e38f)) TSD_FAIL(TSD_E_ARG, "lora merge: scale is not finite");
  if (interleave && (k != 0 || (O & 1))) TSD_FAIL(TSD_E_ARG, "lora merge: the GEGLU interleave needs a linear layer with an even row count");
  if (O <= 0 || I <= 0 || (int64_t)O * I * (k ? k * k : 1) > (int64_t)1 << 28) TSD_FAIL(TSD_E_SHAPE, "lora merge: bad dims O=%d I=%d", O, I);
  if (row0 < 0 || rows <= 0 || row0 > O - rows) TSD_FAIL(TSD_E_SHAPE, "lora merge: rows [%d, %d) outside %d rows", row0, row0 + rows, O);
  const int kk = k ? k * k : 1, ld = round_up(I, 64), Opad = k ? ((O < 64) ? 64 : round_up(O, 4)) : O;
  const int64_t npacked = (int64_t)Opad * kk * ld, nw = (int64_t)O * I * kk;
  std::vector<uint16_t> packed((size_t)npacked);
  HIP_TRY(hipSetDevice(ctx->device));
  int r = run_planned(ctx, [&]() -> int {
    Dev d{ctx};
    float* dw = d.in(w, nw);
    float* du = d.in(up, (int64_t)rows * rank);
    float* dd = d.in(down, (int64_t)rank * I * kk);
    half_t* pw = d.buf<half_t>(npacked);
    if (d.err) return d.err;
    if (k) TSD_TRY(launch_pack_conv(ctx, dw, O, I, k, pw, Opad, ld));
    else TSD_TRY(launch_pack_linear(ctx, dw, O, I, pw, ld, interleave));
    TSD_TRY(launch_lora_merge(ctx, pw, O, I, k, ld, interleave, row0, rows, du, dd, rank, scale));
    return d.out((uint16_t*)packed.data(), (const uint16_t*)pw, npacked);
  });
  if (r != TSD_OK) {
    hipStreamSynchronize(ctx->stream);
    return r;
  }
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  TSD_TRY(ctx_check_status(ctx));
  unpack_weight_host(packed.data(), O, I, k, ld, interleave, out);
  return TSD_OK;
}

extern "C" int tsd_linear_f32(tsd_ctx* ctx, const float* x, int M, int K, const float* w, const float* bias, int N,
                              float* y) {
  NOTNULL(x); NOTNULL(w); NOTNULL(y);
  if (M <= 0 || K <= 0 || N <= 0) TSD_FAIL(TSD_E_SHAPE, "linear: bad dims M=%d K=%d N=%d", M, K, N);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    LinW lw;
    TSD_TRY(d.lin(w, bias, N, K, 0, &lw));
    const int Npad = round_up(N, 4);
    float* dx = d.in(x, (int64_t)M * K);
    half_t* x16 = d.buf<half_t>((int64_t)M * lw.Kpad);
    float* y32 = d.buf<float>((int64_t)M * Npad);
    if (d.err) return d.err;
    TSD_TRY(launch_f32_to_f16_rows(ctx, dx, M, K, x16, lw.Kpad, M));
    GemmArgs g;
    g.A0 = x16; g.lda0 = lw.Kpad; g.Wt = lw.w; g.ldw = lw.Kpad; g.M = M; g.N = Npad; g.K = lw.Kpad;
    g.epi = EPI_OUT_F32 | (lw.b ? EPI_BIAS_N : 0); g.bias = lw.b; g.C = y32; g.ldc = Npad;
    TSD_TRY(launch_gemm(ctx, g));
    return d.out2d(y, y32, M, N, Npad);
  });
}

extern "C" int tsd_matmul_f32(tsd_ctx* ctx, const float* a, const float* bmat, int batch, int b_batch, int M, int K,
                              int N, float* c) {
  NOTNULL(a); NOTNULL(bmat); NOTNULL(c);
  if (batch <= 0 || M <= 0 || K <= 0 || N <= 0 || (b_batch != 1 && b_batch != batch))
    TSD_FAIL(TSD_E_SHAPE, "matmul: bad dims batch=%d b_batch=%d M=%d K=%d N=%d", batch, b_batch, M, K, N);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    const int Kpad = round_up(K, 64), Npad = round_up(N, 4);
    float* da = d.in(a, (int64_t)batch * M * K);
    float* db = d.in(bmat, (int64_t)b_batch * K * N);
    half_t* a16 = d.buf<half_t>((int64_t)batch * M * Kpad);
    half_t* b16 = d.buf<half_t>((int64_t)b_batch * Npad * Kpad);
    float* c32 = d.buf<float>((int64_t)batch * M * Npad);
    if (d.err) return d.err;
    TSD_TRY(launch_f32_to_f16_rows(ctx, da, (int64_t)batch * M, K, a16, Kpad, (int64_t)batch * M));
    TSD_TRY(launch_transpose_f32_to_f16(ctx, db, b_batch, K, N, b16, Kpad, Npad));
    GemmArgs g;
    g.A0 = a16; g.lda0 = Kpad; g.sA = (int64_t)M * Kpad;
    g.Wt = b16; g.ldw = Kpad; g.sW = b_batch == 1 ? 0 : (int64_t)Npad * Kpad;
    g.M = M; g.N = Npad; g.K = Kpad; g.batch = batch;
    g.epi = EPI_OUT_F32; g.C = c32; g.ldc = Npad; g.sC = (int64_t)M * Npad;
    TSD_TRY(launch_gemm(ctx, g));
    return d.out2d(c, c32, batch * M, N, Npad);
  });
}

extern "C" int tsd_upsample_nearest2x_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, float* y) {
  NOTNULL(x); NOTNULL(y);
  if (C <= 0 || H <= 0 || W <= 0) TSD_FAIL(TSD_E_SHAPE, "upsample: bad dims");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    const int64_t n = (int64_t)C * H * W;
    float* dx = d.in(x, n);
    float* dy = d.buf<float>(4 * n);
    if (d.err) return d.err;
    TSD_TRY(launch_upsample_f32(ctx, dx, C, H, W, dy));
    return d.out(y, dy, 4 * n);
  });
}

extern "C" int tsd_softmax_lastdim_f32(tsd_ctx* ctx, const float* x, int64_t rows, int cols, float* y) {
  NOTNULL(x); NOTNULL(y);
  if (rows <= 0 || cols <= 0) TSD_FAIL(TSD_E_SHAPE, "softmax: bad dims");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dx = d.in(x, rows * cols);
    float* dy = d.buf<float>(rows * cols);
    if (d.err) return d.err;
    TSD_TRY(launch_softmax_rows_f32(ctx, dx, rows, cols, dy));
    return d.out(y, dy, rows * cols);
  });
}

extern "C" int tsd_time_embedding_f32(tsd_ctx* ctx, float t, float* out320) {
  NOTNULL(out320);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dy = d.buf<float>(320);
    if (d.err) return d.err;
    TSD_TRY(launch_time_embedding(ctx, nullptr, t, 1, dy));
    return d.out(out320, dy, 320);
  });
}

// shared by self/cross attention: x16 [T][Dpad] -> out
static int attention_tail(tsd_ctx* ctx, Dev& d, const AttnArgs& fa, const LinW& wo, int T, int D, float* y) {
  TSD_TRY(g_attn_core(ctx, fa));
  const int Npad = round_up(D, 4);
  float* y32 = d.buf<float>((int64_t)T * Npad);
  if (d.err) return d.err;
  GemmArgs g;
  g.A0 = fa.O; g.lda0 = fa.ldo; g.Wt = wo.w; g.ldw = wo.Kpad; g.M = T; g.N = Npad; g.K = wo.Kpad;
  g.epi = EPI_OUT_F32 | (wo.b ? EPI_BIAS_N : 0); g.bias = wo.b; g.C = y32; g.ldc = Npad;
  TSD_TRY(launch_gemm(ctx, g));
  return d.out2d(y, y32, T, D, Npad);
}

extern "C" int tsd_self_attention_f32(tsd_ctx* ctx, const float* x, int T, int D, int heads, const float* w_in,
                                      const float* b_in, const float* w_out, const float* b_out, int causal,
                                      float* y) {
  NOTNULL(x); NOTNULL(w_in); NOTNULL(w_out); NOTNULL(y);
  if (causal) TSD_FAIL(TSD_E_SHAPE, "self_attention: causal masking is CLIP-only and not on the device path");
  if (T <= 0 || D <= 0 || heads <= 0 || D % heads || D % 64 || T % 8)
    TSD_FAIL(TSD_E_SHAPE, "self_attention: T=%d D=%d heads=%d unsupported (D %% 64, T %% 8)", T, D, heads);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    LinW wi, wo;
    TSD_TRY(d.lin(w_in, b_in, 3 * D, D, 0, &wi));
    TSD_TRY(d.lin(w_out, b_out, D, D, 0, &wo));
    float* dx = d.in(x, (int64_t)T * D);
    half_t* x16 = d.buf<half_t>((int64_t)T * D);
    half_t* qk = d.buf<half_t>((int64_t)T * 2 * D);
    half_t* vt = d.buf<half_t>((int64_t)D * T);
    half_t* ao = d.buf<half_t>((int64_t)T * D);
    if (d.err) return d.err;
    TSD_TRY(launch_f32_to_f16_rows(ctx, dx, T, D, x16, D, T));
    TSD_TRY(g_qkv_proj(ctx, x16, 1, T, D, wi, qk, vt, T));
    AttnArgs fa;
    fa.Q = qk; fa.ldq = 2 * D; fa.K = qk + D; fa.ldk = 2 * D; fa.Vt = vt; fa.ldvt = T; fa.O = ao; fa.ldo = D;
    fa.B = 1; fa.H = heads; fa.d = D / heads; fa.Sq = T; fa.Sk = T; fa.scale = 1.f / sqrtf((float)(D / heads));
    return attention_tail(ctx, d, fa, wo, T, D, y);
  });
}

extern "C" int tsd_cross_attention_f32(tsd_ctx* ctx, const float* x, int Tq, int D, const float* context, int Tk,
                                       int Dc, int heads, const float* wq, const float* bq, const float* wk,
                                       const float* bk, const float* wv, const float* bv, const float* wo,
                                       const float* bo, float* y) {
  NOTNULL(x); NOTNULL(context); NOTNULL(wq); NOTNULL(wk); NOTNULL(wv); NOTNULL(wo); NOTNULL(y);
  if (Tq <= 0 || Tk <= 0 || D <= 0 || Dc <= 0 || heads <= 0 || D % heads || D % 64)
    TSD_FAIL(TSD_E_SHAPE, "cross_attention: Tq=%d Tk=%d D=%d Dc=%d heads=%d unsupported", Tq, Tk, D, Dc, heads);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    LinW lq, lk, lv, lo;
    TSD_TRY(d.lin(wq, bq, D, D, 0, &lq));
    TSD_TRY(d.lin(wk, bk, D, Dc, 0, &lk));
    TSD_TRY(d.lin(wv, bv, D, Dc, 0, &lv));
    TSD_TRY(d.lin(wo, bo, D, D, 0, &lo));
    const int Tp = round_up(Tk, 8);
    float* dx = d.in(x, (int64_t)Tq * D);
    float* dc = d.in(context, (int64_t)Tk * Dc);
    half_t* x16 = d.buf<half_t>((int64_t)Tq * D);
    half_t* c16 = d.buf<half_t>((int64_t)Tp * lk.Kpad);
    half_t* q = d.buf<half_t>((int64_t)Tq * D);
    half_t* kc = d.buf<half_t>((int64_t)Tp * D);
    half_t* vtc = d.buf<half_t>((int64_t)D * Tp);
    half_t* ao = d.buf<half_t>((int64_t)Tq * D);
    if (d.err) return d.err;
    TSD_TRY(launch_f32_to_f16_rows(ctx, dx, Tq, D, x16, D, Tq));
    TSD_TRY(launch_f32_to_f16_rows(ctx, dc, Tk, Dc, c16, lk.Kpad, Tp));
    CatSrc a; a.p0 = x16; a.ld0 = D; a.C0 = D;
    TSD_TRY(g_linear(ctx, a, Tq, lq.w, lq.Kpad, D, D, lq.b, nullptr, 0, 0, q, D));
    CatSrc ac; ac.p0 = c16; ac.ld0 = lk.Kpad; ac.C0 = lk.Kpad;
    TSD_TRY(g_linear(ctx, ac, Tp, lk.w, lk.Kpad, D, lk.Kpad, lk.b, nullptr, 0, 0, kc, D));
    {
      GemmArgs g;  // V^T = W_v . ctx^T (+ b_v per row)
      g.A0 = lv.w; g.lda0 = lv.Kpad; g.Wt = c16; g.ldw = lv.Kpad; g.M = D; g.N = Tp; g.K = lv.Kpad;
      if (lv.b) { g.epi = EPI_BIAS_M; g.bias = lv.b; }
      g.C = vtc; g.ldc = Tp;
      TSD_TRY(launch_gemm(ctx, g));
    }
    AttnArgs fa;
    fa.Q = q; fa.ldq = D; fa.K = kc; fa.ldk = D; fa.Vt = vtc; fa.ldvt = Tp; fa.O = ao; fa.ldo = D;
    fa.B = 1; fa.H = heads; fa.d = D / heads; fa.Sq = Tq; fa.Sk = Tk; fa.scale = 1.f / sqrtf((float)(D / heads));
    return attention_tail(ctx, d, fa, lo, Tq, D, y);
  });
}

// ---- block level ------------------------------------------------------------------------------------
extern "C" int tsd_time_embedding_mlp_f32(tsd_ctx* ctx, const float* t320, const float* w1, const float* b1,
                                          const float* w2, const float* b2, float* out1280) {
  NOTNULL(t320); NOTNULL(w1); NOTNULL(b1); NOTNULL(w2); NOTNULL(b2); NOTNULL(out1280);
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    LinW l1, l2;
    TSD_TRY(d.lin(w1, b1, 1280, 320, 0, &l1));
    TSD_TRY(d.lin(w2, b2, 1280, 1280, 0, &l2));
    float* dt = d.in(t320, 320);
    float* h = d.buf<float>(1280);
    float* o = d.buf<float>(1280);
    if (d.err) return d.err;
    TSD_TRY(launch_small_linear(ctx, dt, 1, 320, 320, l1.w, l1.Kpad, l1.b, 1280, 0, h, 1280));
    TSD_TRY(launch_small_linear(ctx, h, 1, 1280, 1280, l2.w, l2.Kpad, l2.b, 1280, 1, o, 1280));
    return d.out(out1280, o, 1280);
  });
}

static int res_block_common(tsd_ctx* ctx, const float* x, int Cx, int H, int W, const float* time, int cin, int cout,
                            int groups, const float* conv1_w, const float* conv1_b, const float* lin_w,
                            const float* lin_b, const float* conv2_w, const float* conv2_b, const float* skip_w,
                            const float* skip_b, float* y) {
  if (cin % 64 || cout % 64 || Cx < cin || H <= 0 || W <= 0)
    TSD_FAIL(TSD_E_SHAPE, "residual block: cin=%d cout=%d Cx=%d unsupported (multiples of 64)", cin, cout, Cx);
  if (cin != cout && !skip_w) TSD_FAIL(TSD_E_ARG, "residual block: skip conv weights required when cin != cout");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    ResW rw;
    rw.cin = cin; rw.cout = cout; rw.groups = groups; rw.has_skip = cin != cout;
    TSD_TRY(d.conv(conv1_w, conv1_b, cout, cin, 3, cout, &rw.conv1));
    TSD_TRY(d.conv(conv2_w, conv2_b, cout, cout, 3, cout, &rw.conv2));
    if (rw.has_skip) TSD_TRY(d.conv(skip_w, skip_b, cout, cin, 1, cout, &rw.skip));
    float* tvec = nullptr;
    if (time) {
      LinW lt;
      TSD_TRY(d.lin(lin_w, lin_b, cout, 1280, 0, &lt));
      float* dt = d.in(time, 1280);
      tvec = d.buf<float>(cout);
      if (d.err) return d.err;
      TSD_TRY(launch_small_linear(ctx, dt, 1, 1280, 1280, lt.w, lt.Kpad, lt.b, cout, 1, tvec, cout));  // diffusion.mojo:61-62
    }
    float* dx = d.in(x, (int64_t)Cx * H * W);
    Act xa = act_alloc(ctx, 1, H, W, cin);
    Act out = act_alloc(ctx, 1, H, W, cout);
    float* dy = d.buf<float>((int64_t)cout * H * W);
    if (d.err || !xa.p || !out.p) return d.err ? d.err : TSD_E_ALLOC;
    TSD_TRY(launch_chw_f32_to_nhwc_f16(ctx, dx, 1, Cx, H, W, cin, 1.f, xa.p, cin));
    TSD_TRY(g_resblock(ctx, cat1(xa), 1, H, W, 0, rw, tvec, cout, out));
    TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, out.p, 1, cout, H, W, cout, dy));
    return d.out(y, dy, (int64_t)cout * H * W);
  });
}

extern "C" int tsd_unet_residual_block_f32(tsd_ctx* ctx, const float* x, int Cx, int H, int W, const float* time,
                                           int cin, int cout, const float* conv1_w, const float* conv1_b,
                                           const float* lin_w, const float* lin_b, const float* conv2_w,
                                           const float* conv2_b, const float* skip_w, const float* skip_b, float* y) {
  NOTNULL(x); NOTNULL(time); NOTNULL(conv1_w); NOTNULL(conv1_b); NOTNULL(lin_w); NOTNULL(lin_b); NOTNULL(conv2_w);
  NOTNULL(conv2_b); NOTNULL(y);
  return res_block_common(ctx, x, Cx, H, W, time, cin, cout, 32, conv1_w, conv1_b, lin_w, lin_b, conv2_w, conv2_b,
                          skip_w, skip_b, y);
}

extern "C" int tsd_vae_res_block_f32(tsd_ctx* ctx, const float* x, int H, int W, int cin, int cout,
                                     const float* conv1_w, const float* conv1_b, const float* conv2_w,
                                     const float* conv2_b, const float* skip_w, const float* skip_b, float* y) {
  NOTNULL(x); NOTNULL(conv1_w); NOTNULL(conv1_b); NOTNULL(conv2_w); NOTNULL(conv2_b); NOTNULL(y);
  return res_block_common(ctx, x, cin, H, W, nullptr, cin, cout, 16, conv1_w, conv1_b, nullptr, nullptr, conv2_w,
                          conv2_b, skip_w, skip_b, y);
}

extern "C" int tsd_unet_attention_block_f32(tsd_ctx* ctx, const float* x, int n_head, int n_embed, int H, int W,
                                            const float* context, int Tk, int Dc, const float* const* w, int nw,
                                            float* y) {
  NOTNULL(x); NOTNULL(context); NOTNULL(w); NOTNULL(y);
  if (nw != 16) TSD_FAIL(TSD_E_ARG, "attention block: expected 16 weight pointers, got %d", nw);
  for (int i = 0; i < 16; i++) if (!w[i]) TSD_FAIL(TSD_E_ARG, "attention block: weight pointer %d is NULL", i);
  const int C = n_head * n_embed;
  if (C <= 0 || C % 64 || H <= 0 || W <= 0 || Tk <= 0 || Dc <= 0) TSD_FAIL(TSD_E_SHAPE, "attention block: bad dims");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    AttnW aw;
    aw.n_head = n_head; aw.n_embed = n_embed; aw.C = C; aw.d_ctx = Dc;
    TSD_TRY(d.conv(w[0], w[1], C, C, 1, C, &aw.conv_in));
    TSD_TRY(d.lin(w[2], nullptr, 3 * C, C, 0, &aw.sa_in));      // in_bias=False, diffusion.mojo:92
    TSD_TRY(d.lin(w[3], w[4], C, C, 0, &aw.sa_out));
    TSD_TRY(d.lin(w[5], nullptr, C, C, 0, &aw.ca_q));           // in_bias=False, diffusion.mojo:94
    TSD_TRY(d.lin(w[6], nullptr, C, Dc, 0, &aw.ca_k));
    TSD_TRY(d.lin(w[7], nullptr, C, Dc, 0, &aw.ca_v));
    TSD_TRY(d.lin(w[8], w[9], C, C, 0, &aw.ca_out));
    TSD_TRY(d.lin(w[10], w[11], 8 * C, C, 1, &aw.geglu1));
    TSD_TRY(d.lin(w[12], w[13], C, 4 * C, 0, &aw.geglu2));
    TSD_TRY(d.conv(w[14], w[15], C, C, 1, C, &aw.conv_out));
    const int Tp = round_up(Tk, 8);
    float* dx = d.in(x, (int64_t)C * H * W);
    float* dc = d.in(context, (int64_t)Tk * Dc);
    Act xa = act_alloc(ctx, 1, H, W, C);
    Act out = act_alloc(ctx, 1, H, W, C);
    half_t* c16 = d.buf<half_t>((int64_t)Tp * aw.ca_k.Kpad);
    float* dy = d.buf<float>((int64_t)C * H * W);
    if (d.err || !xa.p || !out.p) return d.err ? d.err : TSD_E_ALLOC;
    TSD_TRY(launch_chw_f32_to_nhwc_f16(ctx, dx, 1, C, H, W, C, 1.f, xa.p, C));
    TSD_TRY(launch_f32_to_f16_rows(ctx, dc, Tk, Dc, c16, aw.ca_k.Kpad, Tp));
    TSD_TRY(g_unet_attn(ctx, xa, aw, c16, Tk, Tp, out));
    TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, out.p, 1, C, H, W, C, dy));
    return d.out(y, dy, (int64_t)C * H * W);
  });
}

extern "C" int tsd_vae_attention_block_f32(tsd_ctx* ctx, const float* x, int C, int H, int W, const float* w_in,
                                           const float* b_in, const float* w_out, const float* b_out, float* y) {
  NOTNULL(x); NOTNULL(w_in); NOTNULL(b_in); NOTNULL(w_out); NOTNULL(b_out); NOTNULL(y);
  if (C <= 0 || C % 64 || H <= 0 || W <= 0) TSD_FAIL(TSD_E_SHAPE, "vae attention block: bad dims");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    VaeAttnW vw;
    vw.C = C;
    TSD_TRY(d.lin(w_in, b_in, 3 * C, C, 0, &vw.in_proj));
    TSD_TRY(d.lin(w_out, b_out, C, C, 0, &vw.out_proj));
    float* dx = d.in(x, (int64_t)C * H * W);
    Act xa = act_alloc(ctx, 1, H, W, C);
    Act out = act_alloc(ctx, 1, H, W, C);
    float* dy = d.buf<float>((int64_t)C * H * W);
    if (d.err || !xa.p || !out.p) return d.err ? d.err : TSD_E_ALLOC;
    TSD_TRY(launch_chw_f32_to_nhwc_f16(ctx, dx, 1, C, H, W, C, 1.f, xa.p, C));
    TSD_TRY(g_vae_attn(ctx, xa, vw, out));
    TSD_TRY(launch_nhwc_f16_to_chw_f32(ctx, out.p, 1, C, H, W, C, dy));
    return d.out(y, dy, (int64_t)C * H * W);
  });
}

// the jitter build shows that it makes a hazard visible: n launches of k_jitter_selftest, the number of distinct words they stored
extern "C" int tsd_debug_jitter_selftest(tsd_ctx* ctx, int n) {
  NOTNULL(ctx);
  if (n < 1 || n > 64) TSD_FAIL(TSD_E_ARG, "jitter_selftest: n=%d (1..64)", n);
  unsigned seen[64];
  const int r = run_op(ctx, [&]() -> int {
    Dev d{ctx};
    unsigned* dv = d.buf<unsigned>(n);
    if (d.err) return d.err;
    TSD_TRY(launch_jitter_selftest(ctx, dv, n));
    return d.out(seen, dv, n);
  });
  if (r != TSD_OK) return r;
  int distinct = 0;
  for (int i = 0; i < n; i++) {
    bool first = true;
    for (int j = 0; j < i; j++) first &= seen[j] != seen[i];
    distinct += first;
  }
  return distinct;
}

extern "C" int tsd_debug_gn_path_counts(tsd_ctx* ctx, int64_t* counts, int n, int reset) {
  NOTNULL(ctx); NOTNULL(counts);
  if (n < 8) TSD_FAIL(TSD_E_ARG, "gn_path_counts: %d slots (8 needed)", n);
  for (int i = 0; i < 8; i++) counts[i] = ctx->gn_paths[i];
  if (reset) for (int i = 0; i < 8; i++) ctx->gn_paths[i] = 0;
  return TSD_OK;
}
