// kernels_slots.hip - the kernels of a slot session (tsd_session_slots_open / _slot_start / _advance, session.cpp): the samples of one
// batch sit at different indices of the schedule, so what the lockstep kernels take as scalars for the whole batch arrives here as a
// by-value table with one entry per sample.
//   k_slot_update      one launch updates every active sample with the coefficients, guidance scale, history flags and noise base of ITS
//                      step, through ddpm_step_element / sampler_step_element (update_element.h) - the functions the lockstep kernels
//                      inline, called with the same global element index and the same pointers, so the bits are the lockstep bits
//   k_slot_update_blend  the same with a second table { on, a_prev, s_prev }: a slot with inpainting on blends the updated value with its
//                      known region before the single store (the lockstep path's k_inpaint_blend, fused: the scalars differ per slot)
//   k_slot_time_rows   gathers row i_b of the hoisted time table for every sample into the [Bu][N] buffer the forward reads per sample
//   k_slot_timesteps   without the hoist: the per-sample timesteps for k_time_embedding's t pointer
// The tables are kernel arguments and read-only.  Grids put a sample on blockIdx.y, so the entry index is uniform for a block and the
// compiler reads the entry with scalar loads from the argument segment into SGPRs (no table in memory, no copy per advance).
#include <algorithm>

#include "common.h"
#include "update_element.h"

// Grid (x blocks over the chw elements of a sample, B).  A SKIP entry returns before its first load: an idle or finished slot's latents
// and history are neither read nor written, and its eps - computed by the forward like everyone's - is ignored and never counted.
// The four loops are the bodies of k_ddpm_step, k_ddpm_step_seeded, k_sampler_step and k_sampler_step_seeded over one sample.
__global__ void k_slot_update(float* x, const float* __restrict__ eps, const float* __restrict__ eps_u, float* hist, SlotTable tab,
                              int64_t chw, int eps_hw, int* __restrict__ nonfinite) {
  const int b = blockIdx.y;
  const SlotEntry& e = tab.e[b];
  const int mode = e.mode, flags = e.flags;
  if (mode == SLOT_SKIP) return;
  const float cfg_scale = e.cfg_scale;
  const int64_t first = b * chw, j0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  int nbad = 0;
  if (mode == SLOT_DDPM) {
    const float sa = e.c[0], sb = e.c[1], c_x0 = e.c[2], c_xt = e.c[3], sigma = e.c[4];
    if (flags & SLOT_NOISE) {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += ddpm_step_element<true>(first + j, x, eps, eps_u, cfg_scale, nullptr, tab.bases, chw, sa, sb, c_x0, c_xt, sigma, eps_hw);
    } else {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += ddpm_step_element<false>(first + j, x, eps, eps_u, cfg_scale, nullptr, NormalBases(), 0, sa, sb, c_x0, c_xt, sigma, eps_hw);
    }
  } else {
    const SamplerCoeffs c = {e.c[0], e.c[1], e.c[2], e.c[3], e.c[4], e.c[5]};
    const float* hist_in = (flags & SLOT_HIST_IN) ? hist : nullptr;
    float* hist_out = (flags & SLOT_HIST_OUT) ? hist : nullptr;
    if (flags & SLOT_NOISE) {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += sampler_step_element<true>(first + j, x, eps, eps_u, cfg_scale, hist_in, nullptr, tab.bases, chw, c, eps_hw, x, hist_out);
    } else {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += sampler_step_element<false>(first + j, x, eps, eps_u, cfg_scale, hist_in, nullptr, NormalBases(), 0, c, eps_hw, x, hist_out);
    }
  }
  nonfinite_report(nonfinite, nbad);
}
int launch_slot_update(tsd_ctx* ctx, float* x, const float* eps, const float* eps_uncond, float* hist, const SlotTable& tab, int B,
                       int64_t chw, int eps_hw) {
  if (B <= 0 || B > 16 || chw <= 0) TSD_FAIL(TSD_E_SHAPE, "slot update: B=%d (1..16) chw=%lld", B, (long long)chw);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  const unsigned gx = (unsigned)std::min<int64_t>((chw + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(k_slot_update, dim3(gx, (unsigned)B), dim3(256), 0, ctx->stream, x, eps, eps_uncond, hist, tab, chw, eps_hw,
                     ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// The update of k_slot_update over the sample of entry e - the same four loops, the same calls - with `post` between an element's update
// and its single store (update_element.h).  k_slot_update keeps its own copy of the loops: its code is pinned (isa_contract.json).
template <class Post>
__device__ __forceinline__ int slot_update_sample(int b, const SlotEntry& e, float* x, const float* __restrict__ eps,
                                                  const float* __restrict__ eps_u, float* hist, const NormalBases& bases, int64_t chw,
                                                  int eps_hw, const Post& post) {
  const int mode = e.mode, flags = e.flags;
  const float cfg_scale = e.cfg_scale;
  const int64_t first = b * chw, j0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  int nbad = 0;
  if (mode == SLOT_DDPM) {
    const float sa = e.c[0], sb = e.c[1], c_x0 = e.c[2], c_xt = e.c[3], sigma = e.c[4];
    if (flags & SLOT_NOISE) {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += ddpm_step_element<true>(first + j, x, eps, eps_u, cfg_scale, nullptr, bases, chw, sa, sb, c_x0, c_xt, sigma, eps_hw, post);
    } else {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += ddpm_step_element<false>(first + j, x, eps, eps_u, cfg_scale, nullptr, NormalBases(), 0, sa, sb, c_x0, c_xt, sigma, eps_hw, post);
    }
  } else {
    const SamplerCoeffs c = {e.c[0], e.c[1], e.c[2], e.c[3], e.c[4], e.c[5]};
    const float* hist_in = (flags & SLOT_HIST_IN) ? hist : nullptr;
    float* hist_out = (flags & SLOT_HIST_OUT) ? hist : nullptr;
    if (flags & SLOT_NOISE) {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += sampler_step_element<true>(first + j, x, eps, eps_u, cfg_scale, hist_in, nullptr, bases, chw, c, eps_hw, x, hist_out, post);
    } else {
      for (int64_t j = j0; j < chw; j += stride)
        nbad += sampler_step_element<false>(first + j, x, eps, eps_u, cfg_scale, hist_in, nullptr, NormalBases(), 0, c, eps_hw, x, hist_out, post);
    }
  }
  return nbad;
}

// k_slot_update for an advance with inpainting slots: the same grid, the same table and the same update; a sample whose SlotBlend entry is
// `on` blends the updated value with its known region (InpaintBlend, update_element.h) before the single store - no launch and no pass
// over the latents beyond the update's own.  mask [B][hw], known / noise [B][4][hw] CHW: the session's ip_* buffers.  The history written
// is the data prediction of the latents the step READ: the blend does not touch it.  Both tables are read through the argument segment.
__global__ void k_slot_update_blend(float* x, const float* __restrict__ eps, const float* __restrict__ eps_u, float* hist, SlotTable tab,
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
    nbad = slot_update_sample(b, e, x, eps, eps_u, hist, tab.bases, chw, eps_hw, post);
  } else {
    nbad = slot_update_sample(b, e, x, eps, eps_u, hist, tab.bases, chw, eps_hw, StoreAsIs());
  }
  nonfinite_report(nonfinite, nbad);
}
int launch_slot_update_blend(tsd_ctx* ctx, float* x, const float* eps, const float* eps_uncond, float* hist, const SlotTable& tab,
                             const SlotBlendTable& blend, const float* mask, const float* known, const float* noise, int B, int64_t chw,
                             int eps_hw) {
  if (B <= 0 || B > 16 || chw <= 0 || (chw & 3)) TSD_FAIL(TSD_E_SHAPE, "slot update + blend: B=%d (1..16) chw=%lld (4 hw)", B, (long long)chw);
  if (!mask || !known || !noise) TSD_FAIL(TSD_E_ARG, "slot update + blend: mask, known and noise are required");
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  const unsigned gx = (unsigned)std::min<int64_t>((chw + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(k_slot_update_blend, dim3(gx, (unsigned)B), dim3(256), 0, ctx->stream, x, eps, eps_uncond, hist, tab, blend, mask,
                     known, noise, chw, eps_hw, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

__global__ void k_slot_time_rows(const float* __restrict__ ttab, int N, SlotRows rows, float* __restrict__ out) {
  const int b = blockIdx.y;
  const float* src = ttab + (int64_t)rows.row[b] * N;
  float* dst = out + (int64_t)b * N;
  for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) dst[j] = src[j];
}
int launch_slot_time_rows(tsd_ctx* ctx, const float* ttab, int N, const SlotRows& rows, int Bu, float* out) {
  if (Bu <= 0 || Bu > 16 || N <= 0) TSD_FAIL(TSD_E_SHAPE, "slot time rows: Bu=%d (1..16) N=%d", Bu, N);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_slot_time_rows, dim3((unsigned)ceil_div(N, 256), (unsigned)Bu), dim3(256), 0, ctx->stream, ttab, N, rows, out);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

__global__ void k_slot_timesteps(SlotTimes t, int Bu, float* __restrict__ tdev) {
  const int b = threadIdx.x;
  if (b < Bu) tdev[b] = t.t[b];
}
int launch_slot_timesteps(tsd_ctx* ctx, const SlotTimes& t, int Bu, float* tdev) {
  if (Bu <= 0 || Bu > 16) TSD_FAIL(TSD_E_SHAPE, "slot timesteps: Bu=%d (1..16)", Bu);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_slot_timesteps, dim3(1), dim3(64), 0, ctx->stream, t, Bu, tdev);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
