// kernels_guidance.hip - guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", eq. 15-16):
// per sample, the classifier-free-guidance combine is scaled back towards the standard deviation of the conditional prediction.
//     e_i   = (c_i - u_i) * s + u_i                       sampler_step_element's combine: three fp32 roundings, no fma
//     var_c = sum c^2 / n - (sum c / n)^2,  var_e likewise over e                          n = chw, sums and moments in fp64
//     g     = phi * sqrt(var_c / var_e) + (1 - phi)       in fp64, rounded ONCE to fp32
//     c'_i  = g * c_i,  u'_i = g * u_i                    one fp32 rounding each, in place
// The update kernel that follows combines c' and u' as it always did and gets g * e up to rounding: no update kernel changes.
// g = 1 exactly (the sample passes through unscaled) when var_e is not finite, var_e <= 0 or var_c is not finite; a var_c that the
// cancellation left below zero counts as zero.
//   k_cfg_moments   grid (G, B): block (g, b) sums c, c^2, e, e^2 over its share of sample b in fp64 - a product of two fp32 values is
//                   exact there - and stores ONE partial [b][g][4]; lanes, waves and blocks are combined in a fixed order, no atomics
//   k_cfg_rescale   the same grid: every block adds the G partials of its sample in index order, computes g and scales its share
// G depends on chw alone and a block's share on (g, chw) alone, so a sample's g and outputs are the same bits at every B and in every
// position of the batch, run after run.  The per-sample scalars arrive as a by-value table (CfgRescaleTable, like SlotTable): the sample
// is blockIdx.y, so the entry is read with scalar loads from the argument segment.  An entry that is off returns before its first load:
// such a sample is neither read nor written.  A sample's chw floats are contiguous in CHW and in the output convolution's [hw][4]
// layout alike, and every operation here is per element or a sum over the sample: no layout flag.
#include <algorithm>

#include "common.h"
#include "lds_dma.h"

constexpr int CFG_THREADS = 256, CFG_WAVES = CFG_THREADS / 64;

// sum over the 64 lanes, in every lane: a butterfly whose pairing is fixed by the lane ids (a + b == b + a bitwise)
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ void __launch_bounds__(CFG_THREADS) k_cfg_moments(const float* __restrict__ eps, const float* __restrict__ eps_u,
                                                             CfgRescaleTable tab, int64_t chw, double* __restrict__ partial) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const CfgRescaleEntry& e = tab.e[b];
  if (!e.on) return;
  const float s = e.cfg_scale;
  const float* c = eps + b * chw;
  const float* u = eps_u + b * chw;
  const int64_t stride = (int64_t)gridDim.x * CFG_THREADS;
  double sc = 0.0, scc = 0.0, se = 0.0, see = 0.0;
  for (int64_t j = blockIdx.x * (int64_t)CFG_THREADS + threadIdx.x; j < chw; j += stride) {
    const float cv = c[j], uv = u[j];
    const float d = cv - uv;
    const float ds = d * s;
    const float ev = ds + uv;
    const double cd = (double)cv, ed = (double)ev;
    const double c2 = cd * cd, e2 = ed * ed;
    sc = sc + cd; scc = scc + c2;
    se = se + ed; see = see + e2;
  }
  sc = wave_sum_f64(sc); scc = wave_sum_f64(scc); se = wave_sum_f64(se); see = wave_sum_f64(see);
  __shared__ double wsum[CFG_WAVES][4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { wsum[wave][0] = sc; wsum[wave][1] = scc; wsum[wave][2] = se; wsum[wave][3] = see; }
  tsd_jitter();
  __syncthreads();
  if (threadIdx.x < 4) {  // thread k adds moment k of the waves in wave order
    double t = wsum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < CFG_WAVES; w++) t = t + wsum[w][threadIdx.x];
    partial[((int64_t)b * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = t;
  }
}

__global__ void __launch_bounds__(CFG_THREADS) k_cfg_rescale(float* __restrict__ eps, float* __restrict__ eps_u, CfgRescaleTable tab,
                                                             int64_t chw, const double* __restrict__ partial,
                                                             float* __restrict__ g_out) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const CfgRescaleEntry& e = tab.e[b];
  if (!e.on) return;
  // the G partials of the sample in index order: the address is uniform for the block
  const double* p = partial + (int64_t)b * gridDim.x * 4;
  double sc = 0.0, scc = 0.0, se = 0.0, see = 0.0;
  for (unsigned k = 0; k < gridDim.x; k++) {
    sc = sc + p[4 * k]; scc = scc + p[4 * k + 1];
    se = se + p[4 * k + 2]; see = see + p[4 * k + 3];
  }
  const double n = (double)chw, phi = (double)e.phi;
  const double mc = sc / n, me = se / n;
  const double mc2 = mc * mc, me2 = me * me;
  double var_c = scc / n - mc2;
  const double var_e = see / n - me2;
  float g = 1.f;
  if (var_e > 0.0 && var_e <= 1.7976931348623157e308 && fabs(var_c) <= 1.7976931348623157e308) {  // false for NaN
    if (var_c < 0.0) var_c = 0.0;
    const double r = sqrt(var_c / var_e);
    const double t = phi * r;
    g = (float)(t + (1.0 - phi));
  }
  if (g_out && blockIdx.x == 0 && threadIdx.x == 0) g_out[b] = g;
  float* c = eps + b * chw;
  float* u = eps_u + b * chw;
  const int64_t stride = (int64_t)gridDim.x * CFG_THREADS;
  for (int64_t j = blockIdx.x * (int64_t)CFG_THREADS + threadIdx.x; j < chw; j += stride) {
    c[j] = g * c[j];
    u[j] = g * u[j];
  }
}

// blocks per sample: one per 2048 elements, at most CFG_RESCALE_GMAX - a function of chw alone
int cfg_rescale_blocks(int64_t chw) { return (int)std::min<int64_t>((chw + 2047) / 2048, CFG_RESCALE_GMAX); }

int launch_cfg_rescale(tsd_ctx* ctx, float* eps, float* eps_uncond, const CfgRescaleTable& tab, int B, int64_t chw, double* partial,
                       float* g_out) {
  if (B <= 0 || B > 16 || chw <= 0) TSD_FAIL(TSD_E_SHAPE, "cfg rescale: B=%d (1..16) chw=%lld", B, (long long)chw);
  if (!eps || !eps_uncond || !partial) TSD_FAIL(TSD_E_ARG, "cfg rescale: eps, eps_uncond and the partials buffer are required");
  if (!ctx->launch()) return TSD_OK;
  const dim3 grid((unsigned)cfg_rescale_blocks(chw), (unsigned)B);
  {
    ProfScope prof(ctx, KC_ELEMENTWISE);
    hipLaunchKernelGGL(k_cfg_moments, grid, dim3(CFG_THREADS), 0, ctx->stream, eps, eps_uncond, tab, chw, partial);
    HIP_TRY(hipGetLastError());
  }
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_cfg_rescale, grid, dim3(CFG_THREADS), 0, ctx->stream, eps, eps_uncond, tab, chw, partial, g_out);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
