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

#define GRID1D(n, bs) dim3((unsigned)std::min<int64_t>(((n) + (bs)-1) / (bs), 1 << 20))

// Every product and sum below is ONE fp32 rounding, in this order, whatever the eps layout and whichever optional pointers are set
// (contraction into fma is off: an absent term is skipped, the others round as before).  Roundings on the longest path
//   x_out: e (sub, mul, add) -> * c_e -> + c_x x -> + c_h h -> + c_n z = 7;   h_out: e (3) -> * sigma_t -> x - . -> / alpha_t = 6
// which is what tests/test_gpu_sampler.py bounds the kernel with.
// eps_hw > 0: eps / eps_u are the UNet output convolution's own layout [B][eps_hw][4] (x, hist and noise stay CHW [B][4][eps_hw]).
// x_out may be x and hist_out may be hist_in: element i is read and written by the same thread only.
__global__ void k_sampler_step(const float* x, const float* __restrict__ eps, const float* __restrict__ eps_u, float cfg_scale,
                               const float* hist_in, const float* __restrict__ noise, int64_t n, SamplerCoeffs c, int eps_hw,
                               float* x_out, float* hist_out, int* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  int nbad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t ie = i;
    if (eps_hw > 0) {
      const int64_t bc = i / eps_hw, pix = i - bc * eps_hw, b = bc >> 2;
      ie = (b * eps_hw + pix) * 4 + (bc & 3);
    }
    float e = eps[ie];
    if (eps_u) {
      const float u = eps_u[ie];
      const float d = e - u;
      const float ds = d * cfg_scale;
      e = ds + u;
    }
    const float xv = x[i];
    float o = c.c_x * xv;
    const float te = c.c_e * e;
    o = o + te;
    if (hist_in) {
      const float th = c.c_h * hist_in[i];
      o = o + th;
    }
    if (noise) {
      const float tn = c.c_n * noise[i];
      o = o + tn;
    }
    if (hist_out) {
      const float se = c.sigma_t * e;
      const float xs = xv - se;
      hist_out[i] = xs / c.alpha_t;
    }
    nbad += nonfinite_f(o);  // a non-finite UNet output (fp16 overflow upstream) lands here every step
    x_out[i] = o;
  }
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
