// kernels_vpred.hip - the sampler updates of a v-prediction session (tsd_session_set_prediction): the model output means
//   v = alpha_t e - sigma_t x0                        (Salimans & Ho 2022), hence x0 = alpha_t x - sigma_t v, e = sigma_t x + alpha_t v
// and DDPM, DDIM(eta) and DPM-Solver++(2M) are all
//   v     = (v_c - v_u) * s + v_u                     CFG combine; v = v_c without it
//   x_out = c_x x + c_v v + c_h h + c_n z             h = the data prediction of the previous step, z ~ N(0,1)
//   h_out = alpha_t x - sigma_t v                     the data prediction, without a division
// with per-step scalars from sampler.cpp (sampler_coeffs_v) that are finite where alpha_bar_t = 0, the first step of a zero-terminal-SNR
// schedule.  The four kernels are the linear-multistep halves of k_sampler_step, k_sampler_step_seeded (kernels_sampler.hip),
// k_slot_update and k_slot_update_blend (kernels_slots.hip) with sampler_step_v_element (update_element.h) as the element: the same
// grids, the same arguments, the same bytes read and written.  They live in a file of their own so that the listings of the eps kernels,
// which are pinned (isa_contract.json), are not touched.  Pure element-wise: one thread per element, no LDS, no cross-thread traffic;
// the only atomic is the non-finite report.
#include <algorithm>

#include "common.h"
#include "update_element.h"

#define GRID1D(n, bs) dim3((unsigned)std::min<int64_t>(((n) + (bs)-1) / (bs), 1 << 20))

__global__ void k_sampler_step_v(const float* x, const float* __restrict__ v, const float* __restrict__ v_u, float cfg_scale,
                                 const float* hist_in, const float* __restrict__ noise, int64_t n, SamplerCoeffs c, int eps_hw,
                                 float* x_out, float* hist_out, int* __restrict__ nonfinite) {
  int nbad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    nbad += sampler_step_v_element<false>(i, x, v, v_u, cfg_scale, hist_in, noise, NormalBases(), 0, c, eps_hw, x_out, hist_out);
  nonfinite_report(nonfinite, nbad);
}
__global__ void k_sampler_step_v_seeded(const float* x, const float* __restrict__ v, const float* __restrict__ v_u, float cfg_scale,
                                        const float* hist_in, NormalBases bases, int64_t chw, int64_t n, SamplerCoeffs c, int eps_hw,
                                        float* x_out, float* hist_out, int* __restrict__ nonfinite) {
  int nbad = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    nbad += sampler_step_v_element<true>(i, x, v, v_u, cfg_scale, hist_in, nullptr, bases, chw, c, eps_hw, x_out, hist_out);
  nonfinite_report(nonfinite, nbad);
}
int launch_sampler_step_v(tsd_ctx* ctx, const float* x, const float* v, const float* v_uncond, float cfg_scale, const float* hist_in,
                          const float* noise, int64_t n, const SamplerCoeffs& c, int eps_hw, float* x_out, float* hist_out) {
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_sampler_step_v, GRID1D(n, 256), dim3(256), 0, ctx->stream, x, v, v_uncond, cfg_scale, hist_in, noise, n, c,
                     eps_hw, x_out, hist_out, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
int launch_sampler_step_v_seeded(tsd_ctx* ctx, const float* x, const float* v, const float* v_uncond, float cfg_scale,
                                 const float* hist_in, const NormalBases& bases, int64_t chw, int64_t n, const SamplerCoeffs& c,
                                 int eps_hw, float* x_out, float* hist_out) {
  if (chw <= 0 || n > 16 * chw) TSD_FAIL(TSD_E_SHAPE, "seeded v sampler step: n=%lld is more than 16 samples of %lld", (long long)n, (long long)chw);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_sampler_step_v_seeded, GRID1D(n, 256), dim3(256), 0, ctx->stream, x, v, v_uncond, cfg_scale, hist_in, bases, chw,
                     n, c, eps_hw, x_out, hist_out, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// ---- slot sessions: k_slot_update / k_slot_update_blend for a v session ---------------------------------------------------------------
// Grid (x blocks over the chw elements of a sample, B); entry b of the by-value table is uniform for a block.  A SKIP entry returns before
// its first load.  Every other entry is SLOT_LMS - the launchers refuse a table with SLOT_DDPM - so the update is the two loops of
// k_sampler_step_v_seeded and k_sampler_step_v over one sample, with `post` between an element's update and its single store.
template <class Post>
__device__ __forceinline__ int slot_update_v_sample(int b, const SlotEntry& e, float* x, const float* __restrict__ v,
                                                    const float* __restrict__ v_u, float* hist, const NormalBases& bases, int64_t chw,
                                                    int eps_hw, const Post& post) {
  const int flags = e.flags;
  const float cfg_scale = e.cfg_scale;
  const int64_t first = b * chw, j0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const SamplerCoeffs c = {e.c[0], e.c[1], e.c[2], e.c[3], e.c[4], e.c[5]};
  const float* hist_in = (flags & SLOT_HIST_IN) ? hist : nullptr;
  float* hist_out = (flags & SLOT_HIST_OUT) ? hist : nullptr;
  int nbad = 0;
  if (flags & SLOT_NOISE) {
    for (int64_t j = j0; j < chw; j += stride)
      nbad += sampler_step_v_element<true>(first + j, x, v, v_u, cfg_scale, hist_in, nullptr, bases, chw, c, eps_hw, x, hist_out, post);
  } else {
    for (int64_t j = j0; j < chw; j += stride)
      nbad += sampler_step_v_element<false>(first + j, x, v, v_u, cfg_scale, hist_in, nullptr, NormalBases(), 0, c, eps_hw, x, hist_out, post);
  }
  return nbad;
}
__global__ void k_slot_update_v(float* x, const float* __restrict__ v, const float* __restrict__ v_u, float* hist, SlotTable tab,
                                int64_t chw, int eps_hw, int* __restrict__ nonfinite) {
  const int b = blockIdx.y;
  const SlotEntry& e = tab.e[b];
  if (e.mode == SLOT_SKIP) return;
  nonfinite_report(nonfinite, slot_update_v_sample(b, e, x, v, v_u, hist, tab.bases, chw, eps_hw, StoreAsIs()));
}
// mask [B][hw], known / noise [B][4][hw] CHW: the session's ip_* buffers, read for `on` entries only.  The history written is the data
// prediction of the latents the step READ: the blend does not touch it.
__global__ void k_slot_update_blend_v(float* x, const float* __restrict__ v, const float* __restrict__ v_u, float* hist, SlotTable tab,
                                      SlotBlendTable blend, const float* __restrict__ mask, const float* __restrict__ known,
                                      const float* __restrict__ noise, int64_t chw, int eps_hw, int* __restrict__ nonfinite) {
  const int b = blockIdx.y;
  const SlotEntry& e = tab.e[b];
  if (e.mode == SLOT_SKIP) return;
  const SlotBlend& bl = blend.e[b];
  int nbad;
  if (bl.on) {
    const int64_t hw = chw >> 2;
    const InpaintBlend post = {mask + b * hw, known, noise, b * chw, hw, bl.a_prev, bl.s_prev};
    nbad = slot_update_v_sample(b, e, x, v, v_u, hist, tab.bases, chw, eps_hw, post);
  } else {
    nbad = slot_update_v_sample(b, e, x, v, v_u, hist, tab.bases, chw, eps_hw, StoreAsIs());
  }
  nonfinite_report(nonfinite, nbad);
}
static int slot_table_is_lms(const SlotTable& tab, int B) {
  for (int b = 0; b < B; b++)
    if (tab.e[b].mode != SLOT_SKIP && tab.e[b].mode != SLOT_LMS)
      TSD_FAIL(TSD_E_ARG, "slot update (v): entry %d has mode %d; a v-prediction update is SLOT_LMS or SLOT_SKIP", b, tab.e[b].mode);
  return TSD_OK;
}
int launch_slot_update_v(tsd_ctx* ctx, float* x, const float* v, const float* v_uncond, float* hist, const SlotTable& tab, int B,
                         int64_t chw, int eps_hw) {
  if (B <= 0 || B > 16 || chw <= 0) TSD_FAIL(TSD_E_SHAPE, "slot update (v): B=%d (1..16) chw=%lld", B, (long long)chw);
  TSD_TRY(slot_table_is_lms(tab, B));
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  const unsigned gx = (unsigned)std::min<int64_t>((chw + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(k_slot_update_v, dim3(gx, (unsigned)B), dim3(256), 0, ctx->stream, x, v, v_uncond, hist, tab, chw, eps_hw,
                     ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
int launch_slot_update_blend_v(tsd_ctx* ctx, float* x, const float* v, const float* v_uncond, float* hist, const SlotTable& tab,
                               const SlotBlendTable& blend, const float* mask, const float* known, const float* noise, int B,
                               int64_t chw, int eps_hw) {
  if (B <= 0 || B > 16 || chw <= 0 || (chw & 3)) TSD_FAIL(TSD_E_SHAPE, "slot update + blend (v): B=%d (1..16) chw=%lld (4 hw)", B, (long long)chw);
  if (!mask || !known || !noise) TSD_FAIL(TSD_E_ARG, "slot update + blend (v): mask, known and noise are required");
  TSD_TRY(slot_table_is_lms(tab, B));
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  const unsigned gx = (unsigned)std::min<int64_t>((chw + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(k_slot_update_blend_v, dim3(gx, (unsigned)B), dim3(256), 0, ctx->stream, x, v, v_uncond, hist, tab, blend, mask,
                     known, noise, chw, eps_hw, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
