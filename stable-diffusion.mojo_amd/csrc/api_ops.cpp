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

#define NOTNULL(p) \
  if (!(p)) TSD_FAIL(TSD_E_ARG, "%s: argument '%s' is NULL", __func__, #p)

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
extern "C" int tsd_latent_mask_f32(tsd_ctx* ctx, const float* mask_px, int B, int L, int mode, float* mask_lat) {
  NOTNULL(ctx); NOTNULL(mask_px); NOTNULL(mask_lat);
  if (mode != TSD_MASK_AREA && mode != TSD_MASK_ANY) TSD_FAIL(TSD_E_ARG, "latent mask: mode %d (0 area, 1 any)", mode);
  if (B <= 0 || L <= 0) TSD_FAIL(TSD_E_SHAPE, "latent mask: B=%d L=%d", B, L);
  const int64_t npx = (int64_t)B * 64 * L * L, nl = (int64_t)B * L * L;
  if (!host_all_in_range(mask_px, (size_t)npx, 0.f, 1.f)) TSD_FAIL(TSD_E_ARG, "latent mask: every mask value must be finite and in [0, 1]");
  return run_op(ctx, [&]() -> int {
    Dev d{ctx};
    float* dm = d.in(mask_px, npx);
    float* dy = d.buf<float>(nl);
    if (d.err) return d.err;
    TSD_TRY(launch_latent_mask(ctx, dm, B, L, mode, dy));
    return d.out(mask_lat, dy, nl);
  });
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
constexpr size_t GD_GUARD = 4096;                     // bytes of NaN pattern before and after every operand
constexpr uint16_t GD_NAN16 = 0x7E5A;                 // fp16 quiet NaN
constexpr uint32_t GD_NAN32 = 0x7FC5A5A5u;            // fp32 quiet NaN (a byte-wise fill that is an fp16 NaN is a finite fp32)
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
int gd_extents(const int64_t* d, int64_t* e) {
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
  for (int s = 0; s < TSD_GO_COUNT; s++) GD_REQ(e[s] >= 0 && e[s] <= lim);
#undef GD_REQ
  return TSD_OK;
}
// Elements of output slot s that the launch may write (1) - everything else of its extent is a pitch gap
std::vector<char> gd_logical(int s, const int64_t* d, int64_t ext) {
  std::vector<char> m((size_t)ext, s == TSD_GO_GN ? 1 : 0);
  if (s == TSD_GO_C) {
    const int64_t cols = gd_c_cols(d);
    for (int64_t b = 0; b < d[TSD_GD_BATCH]; b++)
      for (int64_t r = 0; r < d[TSD_GD_M]; r++) memset(&m[(size_t)(b * d[TSD_GD_SC] + r * d[TSD_GD_LDC])], 1, (size_t)cols);
  } else if (s == TSD_GO_VT) {
    for (int64_t b = 0; b < d[TSD_GD_M] / d[TSD_GD_VT_S]; b++)
      for (int64_t c = 0; c < d[TSD_GD_N] - d[TSD_GD_VT_N0]; c++)
        memset(&m[(size_t)(b * d[TSD_GD_VT_SB] + c * d[TSD_GD_VT_LD])], 1, (size_t)d[TSD_GD_VT_S]);
  }
  return m;
}
struct GdBufs {
  char* p[TSD_GO_COUNT + 2] = {};  // + the K-tile-major weight copy, + the upsample-folded copies
  ~GdBufs() { for (char* q : p) if (q) (void)hipFree(q); }
};
}  // namespace

extern "C" int tsd_debug_gemm_run(tsd_ctx* ctx, const int64_t* desc, int n, int cfg, const void* const* host_in,
                                  void* const* host_out, int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  if (n < TSD_GD_COUNT || cfg >= 64) TSD_FAIL(TSD_E_ARG, "gemm_run: %d descriptor fields, cfg %d", n, cfg);
  TSD_TRY(gd_extents(desc, ext));
  if (!host_in) return TSD_OK;  // sizing only: no context or device needed
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  const int64_t* d = desc;
  const bool alias = (d[TSD_GD_EPI] & EPI_RESIDUAL) && (d[TSD_GD_ALIAS] & 1);
  for (int s = 0; s < TSD_GO_COUNT; s++) {
    if (!ext[s]) continue;
    if (s < TSD_GO_C ? !host_in[s] : !host_out[s - TSD_GO_C]) TSD_FAIL(TSD_E_ARG, "gemm_run: operand slot %d is NULL", s);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  GdBufs bufs;
  std::vector<char> init[TSD_GO_COUNT];  // outputs: guards + extent as filled before the launch
  auto fill = [&](char* p, size_t elems, int es) -> int {
    if (es == 2) HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)p, GD_NAN16, elems, st));
    else HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)p, (int)GD_NAN32, elems, st));
    return TSD_OK;
  };
  for (int s = 0; s < TSD_GO_COUNT; s++) {
    if (!ext[s] || (s == TSD_GO_R && alias)) continue;
    const int es = gd_elem_bytes(s, d);
    const size_t bytes = 2 * GD_GUARD + (size_t)ext[s] * es;
    HIP_TRY(hipMalloc((void**)&bufs.p[s], bytes));
    TSD_TRY(fill(bufs.p[s], bytes / es, es));
    if (s < TSD_GO_C) HIP_TRY(hipMemcpyAsync(bufs.p[s] + GD_GUARD, host_in[s], (size_t)ext[s] * es, hipMemcpyHostToDevice, st));
    else {
      init[s].resize(bytes);
      for (size_t i = 0; i < bytes; i += es) {
        if (es == 2) memcpy(&init[s][i], &GD_NAN16, 2);
        else memcpy(&init[s][i], &GD_NAN32, 4);
      }
      if (s == TSD_GO_C && alias) {
        HIP_TRY(hipMemcpyAsync(bufs.p[s] + GD_GUARD, host_in[TSD_GO_R], (size_t)ext[s] * es, hipMemcpyHostToDevice, st));
        memcpy(&init[s][GD_GUARD], host_in[TSD_GO_R], (size_t)ext[s] * es);
      }
    }
  }
  auto at = [&](int s) -> void* { return bufs.p[s] ? (void*)(bufs.p[s] + GD_GUARD) : nullptr; };
  GemmArgs g;
  g.conv = (int)d[TSD_GD_CONV]; g.M = (int)d[TSD_GD_M]; g.N = (int)d[TSD_GD_N]; g.K = (int)d[TSD_GD_K];
  g.A0 = (const half_t*)at(TSD_GO_A0); g.lda0 = (int)d[TSD_GD_LDA0];
  g.A1 = (const half_t*)at(TSD_GO_A1); g.lda1 = (int)d[TSD_GD_LDA1]; g.K0 = (int)d[TSD_GD_K0];
  g.A2 = (const half_t*)at(TSD_GO_A2); g.lda2 = (int)d[TSD_GD_LDA2];
  g.Wt = (const half_t*)at(TSD_GO_W); g.ldw = (int)d[TSD_GD_LDW];
  g.Wt1 = (const half_t*)at(TSD_GO_WT1); g.ldw1 = (int)d[TSD_GD_LDW1];
  g.batch = (int)d[TSD_GD_BATCH]; g.sA = d[TSD_GD_SA]; g.sW = d[TSD_GD_SW]; g.sC = d[TSD_GD_SC]; g.sR = d[TSD_GD_SR];
  if (g.conv) {
    g.Hs = (int)d[TSD_GD_HS]; g.Ws = (int)d[TSD_GD_WS]; g.Ho = (int)d[TSD_GD_HO]; g.Wo = (int)d[TSD_GD_WO]; g.Cin = (int)d[TSD_GD_CIN];
    g.stride = (int)d[TSD_GD_STRIDE]; g.pad = (int)d[TSD_GD_PAD]; g.ups = (int)d[TSD_GD_UPS];
    g.Cin1 = (int)d[TSD_GD_CIN1]; g.Cin2 = (int)d[TSD_GD_CIN2];
  }
  g.epi = (int)d[TSD_GD_EPI];
  const uint32_t bits = (uint32_t)d[TSD_GD_OUT_SCALE];
  memcpy(&g.out_scale, &bits, 4);
  g.bias = (const float*)at(TSD_GO_BIAS);
  g.rowvec = (const float*)at(TSD_GO_ROWVEC); g.rowvec_ld = (int)d[TSD_GD_ROWVEC_LD]; g.rows_per_batch = (int)d[TSD_GD_ROWS_PER_BATCH];
  g.R = (const half_t*)(alias ? at(TSD_GO_C) : at(TSD_GO_R)); g.ldr = (int)d[TSD_GD_LDR];
  g.C = at(TSD_GO_C); g.ldc = (int)d[TSD_GD_LDC];
  if (d[TSD_GD_VT]) { g.Vt = (half_t*)at(TSD_GO_VT); g.vt_n0 = (int)d[TSD_GD_VT_N0]; g.vt_ld = (int)d[TSD_GD_VT_LD]; g.vt_S = (int)d[TSD_GD_VT_S]; g.vt_sB = d[TSD_GD_VT_SB]; }
  g.gn_part = (float*)at(TSD_GO_GN); g.gn_groups = (int)d[TSD_GD_GN_GROUPS]; g.gn_rows_per_sample = (int)d[TSD_GD_GN_RPS]; g.gn_nslab = (int)d[TSD_GD_GN_NSLAB];
  g.rows_per_sample_hint = (int)d[TSD_GD_RPS_HINT];
  if (d[TSD_GD_W_KTS]) {  // the K-tile-major copy the model path builds for weight-heavy layers
    const int KW = g.conv ? 9 * g.Cin : g.K;
    HIP_TRY(hipMalloc((void**)&bufs.p[TSD_GO_COUNT], 2 * GD_GUARD + (size_t)g.N * KW * 2));
    TSD_TRY(fill(bufs.p[TSD_GO_COUNT], (2 * GD_GUARD) / 2 + (size_t)g.N * KW, 2));
    half_t* tm = (half_t*)(bufs.p[TSD_GO_COUNT] + GD_GUARD);
    TSD_TRY(launch_pack_tile_major(ctx, g.Wt, g.N, KW, tm));
    g.Wt = tm; g.ldw = 64; g.w_kts = g.N * 128;
  }
  if (g.conv && g.ups == 2 && g.Cin % 64 == 0 && host_in[TSD_GO_W]) {
    // the folded parity copies, made from the row-major W the caller passed by the routine tsd_model_prepare uses (model.cpp); whether the
    // launch may run them is launch_gemm's decision
    const int ld = d[TSD_GD_W_KTS] ? 9 * g.Cin : (int)d[TSD_GD_LDW];
    const size_t nf = (size_t)16 * g.N * g.Cin;
    std::vector<uint16_t> folded(nf);
    (void)ups_fold_pack_host((const uint16_t*)host_in[TSD_GO_W], g.N, g.Cin, ld, folded.data());
    HIP_TRY(hipMalloc((void**)&bufs.p[TSD_GO_COUNT + 1], 2 * GD_GUARD + nf * 2));
    TSD_TRY(fill(bufs.p[TSD_GO_COUNT + 1], (2 * GD_GUARD) / 2 + nf, 2));
    HIP_TRY(hipMemcpyAsync(bufs.p[TSD_GO_COUNT + 1] + GD_GUARD, folded.data(), nf * 2, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    g.Wuf = (const half_t*)(bufs.p[TSD_GO_COUNT + 1] + GD_GUARD);
  }
  // the dispatcher's choice (with the recorded graph's long-K split) or a forced tile; a replay is not recorded
  const int prev_force = ctx->opt.force_cfg, prev_big = ctx->opt.sk_big_graph;
  const bool prev_rec = ctx->gemm_rec_on;
  ctx->opt.force_cfg = cfg >= 0 ? cfg : -1;
  if (cfg < 0) ctx->opt.sk_big_graph = (int)d[TSD_GD_SK_BIG];
  ctx->gemm_rec_on = false;
  ctx->gemm_last_cfg = -1; ctx->gemm_last_ways = 0;
  const int r = run_planned(ctx, [&]() -> int { return launch_gemm(ctx, g); });
  ctx->opt.force_cfg = prev_force; ctx->opt.sk_big_graph = prev_big; ctx->gemm_rec_on = prev_rec;
  HIP_TRY(hipStreamSynchronize(st));
  info[0] = ctx->gemm_last_cfg; info[1] = ctx->gemm_last_ways;
  int64_t changed = 0;
  for (int s = TSD_GO_C; s < TSD_GO_COUNT; s++) {
    if (!ext[s]) continue;
    const int es = gd_elem_bytes(s, d);
    std::vector<char> got(init[s].size());
    HIP_TRY(hipMemcpy(got.data(), bufs.p[s], got.size(), hipMemcpyDeviceToHost));
    const std::vector<char> logical = gd_logical(s, d, ext[s]);
    const int64_t g0 = (int64_t)(GD_GUARD / es), total = (int64_t)(got.size() / es);
    for (int64_t i = 0; i < total; i++) {
      const int64_t j = i - g0;
      if (j >= 0 && j < ext[s] && logical[(size_t)j]) continue;
      if (memcmp(&got[(size_t)i * es], &init[s][(size_t)i * es], es)) changed++;
    }
    memcpy(host_out[s - TSD_GO_C], &got[GD_GUARD], (size_t)ext[s] * es);
  }
  info[2] = changed;
  return r;
}

// ---- GroupNorm / LayerNorm launches on caller operands (tests/norm_ref.py holds every statistics path to an fp64 reference) ------
namespace {
float nd_float(int64_t bits) {
  const uint32_t b = (uint32_t)bits;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
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
struct NdBufs {
  char* p[TSD_NO_COUNT] = {};
  ~NdBufs() { for (char* q : p) if (q) (void)hipFree(q); }
};
}  // namespace

extern "C" int tsd_debug_norm_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                  int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  if (n < TSD_ND_COUNT) TSD_FAIL(TSD_E_ARG, "norm_run: %d descriptor fields", n);
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
  for (int s = 0; s < TSD_NO_COUNT; s++) {
    if (!ext[s]) continue;
    if (s < TSD_NO_Y ? !host_in[s] : !host_out[s - TSD_NO_Y]) TSD_FAIL(TSD_E_ARG, "norm_run: operand slot %d is NULL", s);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  NdBufs bufs;
  for (int s = 0; s < TSD_NO_COUNT; s++) {
    if (!ext[s]) continue;
    const int es = nd_elem_bytes(s);
    const size_t bytes = 2 * GD_GUARD + (size_t)ext[s] * es;
    HIP_TRY(hipMalloc((void**)&bufs.p[s], bytes));
    if (es == 2) HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)bufs.p[s], GD_NAN16, bytes / 2, st));
    else HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)bufs.p[s], (int)GD_NAN32, bytes / 4, st));
    if (s < TSD_NO_Y) HIP_TRY(hipMemcpyAsync(bufs.p[s] + GD_GUARD, host_in[s], (size_t)ext[s] * es, hipMemcpyHostToDevice, st));
  }
  auto at = [&](int s) -> void* { return bufs.p[s] ? (void*)(bufs.p[s] + GD_GUARD) : nullptr; };
  const float eps = nd_float(d[TSD_ND_EPS]), gamma = nd_float(d[TSD_ND_GAMMA]);
  NormAffine aff;
  aff.w = (const float*)at(TSD_NO_W); aff.b = (const float*)at(TSD_NO_BIAS); aff.torch_rstd = (int)d[TSD_ND_TORCH_RSTD];
  const NormAffine* affp = (aff.w || aff.b || aff.torch_rstd) ? &aff : nullptr;
  ctx->gn_last = GnPlan();
  const int r = run_planned(ctx, [&]() -> int {
    if (mode == TSD_NM_LAYERNORM)
      return launch_layernorm(ctx, (const half_t*)at(TSD_NO_X0), d[TSD_ND_ROWS], C, (int)d[TSD_ND_LD0], eps, (half_t*)at(TSD_NO_Y),
                              (int)d[TSD_ND_LDY], affp);
    if (mode == TSD_NM_GN_FINALIZE)
      return launch_gn_finalize(ctx, (const float*)at(TSD_NO_PART0), ns, B, HW, C, G, eps, gamma, (float*)at(TSD_NO_STATS));
    if (mode == TSD_NM_GN_STATS)
      return launch_gn_stats(ctx, (const half_t*)at(TSD_NO_X0), (int)d[TSD_ND_LD0], B, HW, C, G, eps, gamma, (float*)at(TSD_NO_STATS));
    NormSrc src;
    src.x0 = (const half_t*)at(TSD_NO_X0); src.ld0 = (int)d[TSD_ND_LD0]; src.C0 = (int)d[TSD_ND_C0];
    src.x1 = (const half_t*)at(TSD_NO_X1); src.ld1 = (int)d[TSD_ND_LD1];
    const int sm = (int)d[TSD_ND_STATS];
    const GnComposite gc = composite_of((const float*)at(TSD_NO_PART0), (const float*)at(TSD_NO_PART1));
    return launch_groupnorm(ctx, src, B, HW, C, G, eps, gamma, (int)d[TSD_ND_SILU], (half_t*)at(TSD_NO_Y), (int)d[TSD_ND_LDY],
                            sm == 1 ? (const float*)at(TSD_NO_PART0) : nullptr, sm == 1 ? ns : 0, affp, sm == 2 ? &gc : nullptr);
  });
  HIP_TRY(hipStreamSynchronize(st));
  nd_plan_info(ctx->gn_last, info);  // what the launch itself planned (zeros when it was refused)
  int64_t changed = 0;
  for (int s = 0; s < TSD_NO_COUNT; s++) {  // inputs too: a norm launch writes none of them
    if (!ext[s]) continue;
    const int es = nd_elem_bytes(s);
    const size_t bytes = 2 * GD_GUARD + (size_t)ext[s] * es;
    std::vector<char> got(bytes);
    HIP_TRY(hipMemcpy(got.data(), bufs.p[s], bytes, hipMemcpyDeviceToHost));
    const int64_t g0 = (int64_t)(GD_GUARD / es), total = (int64_t)(bytes / es);
    const int64_t width = C, pitch = s == TSD_NO_Y ? d[TSD_ND_LDY] : 0;
    for (int64_t i = 0; i < total; i++) {
      const int64_t j = i - g0;
      const bool inside = j >= 0 && j < ext[s];
      if (inside && s < TSD_NO_Y) continue;                              // input payload
      if (inside && s == TSD_NO_STATS) continue;                         // dense output
      if (inside && s == TSD_NO_Y && j % pitch < width) continue;        // logical element of y
      const bool same = es == 2 ? memcmp(&got[(size_t)i * 2], &GD_NAN16, 2) == 0 : memcmp(&got[(size_t)i * 4], &GD_NAN32, 4) == 0;
      if (!same) changed++;
    }
    if (s >= TSD_NO_Y) memcpy(host_out[s - TSD_NO_Y], &got[GD_GUARD], (size_t)ext[s] * es);
  }
  info[TSD_NI_CHANGED] = changed;
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
  AD_REQ(d[TSD_AD_VERSION] == TSD_AD_VERSION_1);
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
struct AdBufs {
  char* p[TSD_AO_COUNT] = {};
  ~AdBufs() { for (char* q : p) if (q) (void)hipFree(q); }
};
}  // namespace

extern "C" int tsd_debug_attn_run(tsd_ctx* ctx, const int64_t* desc, int n, const void* const* host_in, void* const* host_out,
                                  int64_t* ext, int64_t* info) {
  NOTNULL(desc); NOTNULL(ext);
  if (n < TSD_AD_COUNT) TSD_FAIL(TSD_E_ARG, "attn_run: %d descriptor fields", n);
  TSD_TRY(ad_extents(desc, ext));
  const int64_t* d = desc;
  const bool attn = d[TSD_AD_MODE] == TSD_AM_ATTN;
  if (info) for (int i = 0; i < TSD_AI_COUNT; i++) info[i] = 0;
  if (!host_in) {  // sizing only: no context or device needed; the dispatcher's choice under the default options
    if (info && attn && attn_fused_supported((int)d[TSD_AD_D]) && d[TSD_AD_SQ] > 0 && d[TSD_AD_SK] > 0) {
      TsdOptions o;
      o.attn_qb_force = (int)d[TSD_AD_KERNEL]; o.attn_diag = (int)d[TSD_AD_DIAG];
      const AttnPlan p = attn_plan(o, (int)d[TSD_AD_B], (int)d[TSD_AD_H], (int)d[TSD_AD_D], (int)d[TSD_AD_SQ], (int)d[TSD_AD_SK]);
      info[TSD_AI_KERNEL] = p.kernel; info[TSD_AI_DIAG] = p.diag; info[TSD_AI_XCD_MAP] = p.xcd_map;
    }
    return TSD_OK;
  }
  NOTNULL(ctx); NOTNULL(host_out); NOTNULL(info);
  const bool inplace = !attn && d[TSD_AD_DTYPE] == 1;
  for (int s = 0; s < TSD_AO_COUNT; s++) {
    if (!ext[s]) continue;
    if (s < TSD_AO_O ? !host_in[s] : !host_out[0]) TSD_FAIL(TSD_E_ARG, "attn_run: operand slot %d is NULL", s);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  AdBufs bufs;
  for (int s = 0; s < TSD_AO_COUNT; s++) {
    if (!ext[s]) continue;
    const int es = ad_elem_bytes(s, d);
    const size_t bytes = 2 * GD_GUARD + (size_t)ext[s] * es;
    HIP_TRY(hipMalloc((void**)&bufs.p[s], bytes));
    if (es == 2) HIP_TRY(hipMemsetD16Async((hipDeviceptr_t)bufs.p[s], GD_NAN16, bytes / 2, st));
    else HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)bufs.p[s], (int)GD_NAN32, bytes / 4, st));
    const void* src = s < TSD_AO_O ? host_in[s] : (inplace ? host_in[TSD_AO_X] : nullptr);  // fp16 rows are overwritten in place: O starts as X
    if (src) HIP_TRY(hipMemcpyAsync(bufs.p[s] + GD_GUARD, src, (size_t)ext[s] * es, hipMemcpyHostToDevice, st));
  }
  auto at = [&](int s) -> void* { return bufs.p[s] ? (void*)(bufs.p[s] + GD_GUARD) : nullptr; };
  int exact0 = 0, exact1 = 0;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(&exact0, ctx->status + 2, sizeof(int), hipMemcpyDeviceToHost));
  const int prev_force = ctx->opt.attn_qb_force, prev_diag = ctx->opt.attn_diag;
  ctx->attn_last = AttnPlan();
  int r;
  if (attn) {
    ctx->opt.attn_qb_force = (int)d[TSD_AD_KERNEL]; ctx->opt.attn_diag = (int)d[TSD_AD_DIAG];
    AttnArgs a;
    a.Q = (const half_t*)at(TSD_AO_Q); a.ldq = (int)d[TSD_AD_LDQ]; a.sQ = d[TSD_AD_SQB];
    a.K = (const half_t*)at(TSD_AO_K); a.ldk = (int)d[TSD_AD_LDK]; a.sK = d[TSD_AD_SKB];
    a.Vt = (const half_t*)at(TSD_AO_VT); a.ldvt = (int)d[TSD_AD_LDVT]; a.sVt = d[TSD_AD_SVTB];
    a.O = (half_t*)at(TSD_AO_O); a.ldo = (int)d[TSD_AD_LDO]; a.sO = d[TSD_AD_SOB];
    a.B = (int)d[TSD_AD_B]; a.H = (int)d[TSD_AD_H]; a.d = (int)d[TSD_AD_D]; a.Sq = (int)d[TSD_AD_SQ]; a.Sk = (int)d[TSD_AD_SK];
    a.scale = nd_float(d[TSD_AD_SCALE]);
    r = run_planned(ctx, [&]() -> int { return launch_flash_attention(ctx, a); });
    ctx->opt.attn_qb_force = prev_force; ctx->opt.attn_diag = prev_diag;
  } else {
    const int64_t rows = d[TSD_AD_ROWS];
    const int cols = (int)d[TSD_AD_COLS], ld = (int)d[TSD_AD_LD];
    r = run_planned(ctx, [&]() -> int {
      if (d[TSD_AD_DTYPE] == 0) return launch_softmax_rows_f32(ctx, (const float*)at(TSD_AO_X), rows, cols, (float*)at(TSD_AO_O));
      if (d[TSD_AD_CAUSAL] > 0)
        return launch_softmax_rows_f16_causal(ctx, (half_t*)at(TSD_AO_O), rows, cols, ld, (int)d[TSD_AD_CAUSAL], (int)d[TSD_AD_ZERO_TO]);
      return launch_softmax_rows_f16(ctx, (half_t*)at(TSD_AO_O), rows, cols, ld);
    });
  }
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipMemcpy(&exact1, ctx->status + 2, sizeof(int), hipMemcpyDeviceToHost));
  info[TSD_AI_KERNEL] = attn ? ctx->attn_last.kernel : ctx->attn_last.softmax;
  info[TSD_AI_DIAG] = ctx->attn_last.diag; info[TSD_AI_XCD_MAP] = ctx->attn_last.xcd_map;
  info[TSD_AI_EXACT_WGS] = exact1 - exact0;
  int64_t changed = 0;
  for (int s = 0; s < TSD_AO_COUNT; s++) {  // inputs too: the launch writes none of them
    if (!ext[s]) continue;
    const int es = ad_elem_bytes(s, d);
    const size_t bytes = 2 * GD_GUARD + (size_t)ext[s] * es;
    std::vector<char> got(bytes);
    HIP_TRY(hipMemcpy(got.data(), bufs.p[s], bytes, hipMemcpyDeviceToHost));
    const int64_t g0 = (int64_t)(GD_GUARD / es), total = (int64_t)(bytes / es);
    const char* x0 = inplace ? (const char*)host_in[TSD_AO_X] : nullptr;
    for (int64_t i = 0; i < total; i++) {
      const int64_t j = i - g0;
      const bool inside = j >= 0 && j < ext[s];
      if (inside && s < TSD_AO_O) continue;  // input payload
      if (inside && attn) {                  // logical element of O: [b][q][c < H*d]
        const int64_t jb = j % d[TSD_AD_SOB], b = j / d[TSD_AD_SOB];
        if (b < d[TSD_AD_B] && jb / d[TSD_AD_LDO] < d[TSD_AD_SQ] && jb % d[TSD_AD_LDO] < d[TSD_AD_H] * d[TSD_AD_D]) continue;
      }
      if (inside && !attn) {
        if (j % d[TSD_AD_LD] < std::max(d[TSD_AD_COLS], d[TSD_AD_ZERO_TO])) continue;
        if (x0) {  // a pitch gap of rows processed in place keeps what the caller put there
          if (memcmp(&got[(size_t)i * 2], x0 + (size_t)j * 2, 2)) changed++;
          continue;
        }
      }
      const bool same = es == 2 ? memcmp(&got[(size_t)i * 2], &GD_NAN16, 2) == 0 : memcmp(&got[(size_t)i * 4], &GD_NAN32, 4) == 0;
      if (!same) changed++;
    }
    if (s == TSD_AO_O) memcpy(host_out[0], &got[GD_GUARD], (size_t)ext[s] * es);
  }
  info[TSD_AI_CHANGED] = changed;
  return r;
}

extern "C" int tsd_debug_gn_path_counts(tsd_ctx* ctx, int64_t* counts, int n, int reset) {
  NOTNULL(ctx); NOTNULL(counts);
  if (n < 8) TSD_FAIL(TSD_E_ARG, "gn_path_counts: %d slots (8 needed)", n);
  for (int i = 0; i < 8; i++) counts[i] = ctx->gn_paths[i];
  if (reset) for (int i = 0; i < 8; i++) ctx->gn_paths[i] = 0;
  return TSD_OK;
}
