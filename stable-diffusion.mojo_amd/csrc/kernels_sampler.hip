// kernels_sampler.hip - the per-element update shared by the linear-multistep samplers of the denoise session: DDIM(eta)
// (Song et al. 2021, eq. 12) and DPM-Solver++(2M) (Lu et al. 2022, alg. 2, data prediction).  Both are
//   e     = (e_c - e_u) * s + e_u                    CFG combine (pipeline.mojo:117-119); e = e_c without it
//   x0    = (x - sigma_t e) / alpha_t                the data prediction
//   x_out = c_x x + c_e e + c_h h + c_n z            h = the data prediction of the previous step, z ~ N(0,1)
//   h_out = x0
// with per-step scalars from sampler.cpp.  The reference's DDPM step keeps its own kernel (k_ddpm_step, kernels_elementwise.hip): its
// x0 * c_x0 + x * c_xt rounds differently from this collapsed form.
#include <algorithm>

#include "common.h"
#include "update_element.h"

#define GRID1D(n, bs) dim3((unsigned)std::min<int64_t>(((n) + (bs)-1) / (bs), 1 << 20))

// One element of the update: sampler_step_element (update_element.h, with its rounding order), shared with the per-slot kernel.
__global__ void k_sampler_step(const float* x, const float* __restrict__ eps, const float* __restrict__ eps_u, float cfg_scale,
                               const float* hist_in, const float* __restrict__ noise, int64_t n, SamplerCoeffs c, int eps_hw,
                               float* x_out, float* hist_out, int* __restrict__ nonfinite) {
  int nbad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    nbad += sampler_step_element<false>(i, x, eps, eps_u, cfg_scale, hist_in, noise, NormalBases(), 0, c, eps_hw, x_out, hist_out);
  nonfinite_report(nonfinite, nbad);
}
__global__ void k_sampler_step_seeded(const float* x, const float* __restrict__ eps, const float* __restrict__ eps_u, float cfg_scale,
                                      const float* hist_in, NormalBases bases, int64_t chw, int64_t n, SamplerCoeffs c, int eps_hw,
                                      float* x_out, float* hist_out, int* __restrict__ nonfinite) {
  int nbad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    nbad += sampler_step_element<true>(i, x, eps, eps_u, cfg_scale, hist_in, nullptr, bases, chw, c, eps_hw, x_out, hist_out);
  nonfinite_report(nonfinite, nbad);
}
int launch_sampler_step(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                        const float* hist_in, const float* noise, int64_t n, const SamplerCoeffs& c, int eps_hw, float* x_out,
                        float* hist_out) {
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_sampler_step, GRID1D(n, 256), dim3(256), 0, ctx->stream, x, eps, eps_uncond, cfg_scale, hist_in, noise, n,
                     c, eps_hw, x_out, hist_out, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
int launch_sampler_step_seeded(tsd_ctx* ctx, const float* x, const float* eps, const float* eps_uncond, float cfg_scale,
                               const float* hist_in, const NormalBases& bases, int64_t chw, int64_t n, const SamplerCoeffs& c,
                               int eps_hw, float* x_out, float* hist_out) {
  if (chw <= 0 || n > 16 * chw) TSD_FAIL(TSD_E_SHAPE, "seeded sampler step: n=%lld is more than 16 samples of %lld", (long long)n, (long long)chw);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_sampler_step_seeded, GRID1D(n, 256), dim3(256), 0, ctx->stream, x, eps, eps_uncond, cfg_scale, hist_in, bases,
                     chw, n, c, eps_hw, x_out, hist_out, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// ---- N(0,1) fill from the counter RNG (counter_rng.h): the latents, the add_noise / inpainting noise and the op-level entry -------------
// Grid-stride over n elements in CHW per sample: element j of sample b is value first + j of the stream bases.base[b].  The seeded updates
// above call the same normal_counter with first = 0, so a buffer filled here and read by the unseeded update gives their bits.
__global__ void k_fill_normal(float* __restrict__ dst, int64_t n, int64_t per_sample, NormalBases bases, uint64_t first) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / per_sample;
    dst[i] = normal_counter(bases.base[b], first + (uint64_t)(i - b * per_sample));
  }
}
int launch_fill_normal(tsd_ctx* ctx, float* dst, int64_t n, int64_t per_sample, const NormalBases& bases, uint64_t first) {
  if (per_sample <= 0 || n > 16 * per_sample) TSD_FAIL(TSD_E_SHAPE, "normal fill: n=%lld is more than 16 samples of %lld", (long long)n, (long long)per_sample);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_fill_normal, GRID1D(n, 256), dim3(256), 0, ctx->stream, dst, n, per_sample, bases, first);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// ---- masked denoising (inpainting): hold the known region of the latents after a sampler update -------------------------------------
//   k     = a_prev * known + s_prev * noise        the original latents noised to the timestep the update has just reached
//   x_out = m * x + (1 - m) * k                    m = 1: regenerate (keep the sampler's x), m = 0: keep the known region
// x / known / noise / x_out are CHW [B][4][hw] fp32, mask is [B][hw] and serves the 4 channels of its sample.  noise may be nullptr:
// its term is skipped and k = a_prev * known.  Every product, sum and difference is ONE fp32 rounding (contraction into fma is off), in
// this order:
//   ka = a_prev * known ; kn = s_prev * noise ; k = ka + kn ; om = 1 - m ; tx = m * x ; tk = om * k ; x_out = tx + tk
// Roundings that reach the output through its worst term (a_prev * known, or s_prev * noise): the product, k's sum, om, tk and the final
// sum = 5 (4 without noise: no sum in k; the m * x term sees 2).  The dependency chain itself is 4 deep, om rounds beside k; 5 is what
// tests/test_gpu_inpaint.py bounds the kernel with.  This form, not k + m (x - k), has exact ends for finite operands: m = 1 gives
// om = 0, tk = +-0 and x_out = x bitwise (an x of -0 comes out as +0 or -0, equal as floats); m = 0 gives tx = +-0 and x_out = k bitwise.
// A non-finite x under m = 0 is 0 * inf = NaN in the output and is counted, never replaced.
// x_out may be x: element i is read and written by the same thread only.
__global__ void k_inpaint_blend(const float* x, const float* __restrict__ mask, const float* __restrict__ known,
                                const float* __restrict__ noise, int64_t n, int64_t hw, float a_prev, float s_prev, float* x_out,
                                int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  int nbad = 0;
  const int64_t chw = 4 * hw;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / chw, pix = (i - b * chw) % hw;
    const float m = mask[b * hw + pix];
    float k = a_prev * known[i];
    if (noise) {
      const float kn = s_prev * noise[i];
      k = k + kn;
    }
    const float om = 1.f - m;
    const float tx = m * x[i];
    const float tk = om * k;
    const float o = tx + tk;
    nbad += nonfinite_f(o);
    x_out[i] = o;
  }
  nonfinite_report(nonfinite, nbad);
}
int launch_inpaint_blend(tsd_ctx* ctx, const float* x, const float* mask, const float* known, const float* noise, int B, int64_t hw,
                         float a_prev, float s_prev, float* x_out) {
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  const int64_t n = (int64_t)B * 4 * hw;
  hipLaunchKernelGGL(k_inpaint_blend, GRID1D(n, 256), dim3(256), 0, ctx->stream, x, mask, known, noise, n, hw, a_prev, s_prev, x_out,
                     ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// Pixel mask [B][8LH][8LW] -> latent mask [B][LH][LW]: one thread per latent cell reduces its 8x8 block, rows top to bottom and left to
// right within a row (a fixed order; one rounding per addition).
//   TSD_MASK_AREA: the sum of the 64 values times 1/64 (a power of two: exact)
//   TSD_MASK_ANY:  1 if the block's maximum is >= 0.5, else 0 - a latent cell that touches any masked pixel is regenerated
__global__ void k_latent_mask(const float* __restrict__ mask_px, int B, int LH, int LW, int mode, float* __restrict__ mask_lat) {
#pragma clang fp contract(off)
  const int64_t hw = (int64_t)LH * LW, n = B * hw;
  const int H = 8 * LH, W = 8 * LW;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = i / hw;
    const int cell = (int)(i - b * hw), cy = cell / LW, cx = cell - cy * LW;
    const float* src = mask_px + (b * H + (int64_t)cy * 8) * W + cx * 8;
    float sum = 0.f, mx = 0.f;
    for (int r = 0; r < 8; r++)
      for (int c = 0; c < 8; c++) {
        const float v = src[(int64_t)r * W + c];
        sum = sum + v;
        mx = fmaxf(mx, v);
      }
    mask_lat[i] = mode == TSD_MASK_ANY ? (mx >= 0.5f ? 1.f : 0.f) : sum * 0.015625f;
  }
}
int launch_latent_mask(tsd_ctx* ctx, const float* mask_px, int B, int LH, int LW, int mode, float* mask_lat) {
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_latent_mask, GRID1D((int64_t)B * LH * LW, 256), dim3(256), 0, ctx->stream, mask_px, B, LH, LW, mode, mask_lat);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
