// update_element.h - one element of a sampler update, shared by every kernel that applies one: k_ddpm_step / k_ddpm_step_seeded
// (kernels_elementwise.hip), k_sampler_step / k_sampler_step_seeded (kernels_sampler.hip) and k_slot_update / k_slot_update_blend
// (kernels_slots.hip), and by their v-prediction siblings (kernels_vpred.hip).  The lockstep kernels and the per-slot kernels inline the SAME function, so a slot's update gives the bits of the
// lockstep step it stands for.
// Include after common.h.
#pragma once
#include "common.h"

// What an element function does with the updated value o between computing and storing it: post(i, o, nbad) returns what is stored at
// x[i] and adds what it counts as non-finite to nbad.  StoreAsIs, the default, is the update as it always was (the lockstep kernels
// and k_slot_update).
struct StoreAsIs {
  __device__ __forceinline__ float operator()(int64_t, float o, int&) const { return o; }
};
// The masked-denoising blend of k_inpaint_blend (kernels_sampler.hip states the formula and why this form) on one sample, applied to the
// update's value before its single store: the same seven operations in the same order, ONE fp32 rounding each (no fma), so the stored
// value is bit for bit what the lockstep update launch followed by the lockstep blend launch leaves.  The blended value is counted like
// the blend launch counts it (the update's own value is counted by the element function, like the update launch does).
// first = b * chw, the sample's first global element; mask is the SAMPLE's [hw] plane (it serves the 4 channels), known / noise are the
// whole CHW [B][4][hw] tensors, indexed like x.
struct InpaintBlend {
  const float* __restrict__ mask;
  const float* __restrict__ known;
  const float* __restrict__ noise;
  int64_t first, hw;
  float a_prev, s_prev;
  __device__ __forceinline__ float operator()(int64_t i, float x, int& nbad) const {
#pragma clang fp contract(off)
    // The update's value is final here.  ddpm_step_element leaves contraction to the compiler, which decides per expression tree: without
    // this fence the blend's operations join the update's tree and the update rounds differently than in the lockstep kernels.
    asm volatile("" : "+v"(x));
    int64_t pix = i - first;  // < 4 hw: the channel is peeled off without a division
    if (pix >= 2 * hw) pix -= 2 * hw;
    if (pix >= hw) pix -= hw;
    const float m = mask[pix];
    const float ka = a_prev * known[i];
    const float kn = s_prev * noise[i];
    const float k = ka + kn;
    const float om = 1.f - m;
    const float tx = m * x;
    const float tk = om * k;
    const float o = tx + tk;
    nbad += nonfinite_f(o);
    return o;
  }
};

// ---- DDPM update + CFG combine (sampler.mojo:75-109, pipeline.mojo:117-119; App.D K9) ------------
// eps_hw > 0: eps / eps_u are the UNet output convolution's own layout [B][eps_hw][4] (x and noise stay CHW [B][4][eps_hw])
// One element of the update.  SEEDED: the noise is drawn where the other flavour reads noise[i] - normal_counter(bases.base[b], j) for element j of
// sample b (chw elements per sample, counter_rng.h) - and is always added; without it the instantiation is the kernel as it always was.
template <bool SEEDED, class Post = StoreAsIs>
__device__ __forceinline__ int ddpm_step_element(int64_t i, float* __restrict__ x, const float* __restrict__ eps,
                                                 const float* __restrict__ eps_u, float cfg_scale, const float* __restrict__ noise,
                                                 const NormalBases& bases, int64_t chw, float sa, float sb, float c_x0, float c_xt,
                                                 float sigma, int eps_hw, const Post& post = Post()) {
  int64_t ie = i;
  if (eps_hw > 0) {
    const int64_t bc = i / eps_hw, pix = i - bc * eps_hw, b = bc >> 2;
    ie = (b * eps_hw + pix) * 4 + (bc & 3);
  }
  float e = eps[ie];
  if (eps_u) {
    const float u = eps_u[ie];
    e = (e - u) * cfg_scale + u;
  }
  const float xv = x[i];
  const float x0 = (xv - e * sb) / sa;
  float o = x0 * c_x0 + xv * c_xt;
  if constexpr (SEEDED) {
    const int64_t b = i / chw;
    o += normal_counter(bases.base[b], (uint64_t)(i - b * chw)) * sigma;
  } else {
    if (noise) o += noise[i] * sigma;
  }
  int nbad = nonfinite_f(o);  // a non-finite UNet output (fp16 overflow upstream) lands here every step
  x[i] = post(i, o, nbad);
  return nbad;
}

// ---- linear-multistep update (DDIM, DPM-Solver++(2M); kernels_sampler.hip states the formula) ------------
// Every product and sum below is ONE fp32 rounding, in this order, whatever the eps layout and whichever optional pointers are set
// (contraction into fma is off: an absent term is skipped, the others round as before).  Roundings on the longest path
//   x_out: e (sub, mul, add) -> * c_e -> + c_x x -> + c_h h -> + c_n z = 7;   h_out: e (3) -> * sigma_t -> x - . -> / alpha_t = 6
// which is what tests/test_gpu_sampler.py bounds the kernel with.
// eps_hw > 0: eps / eps_u are the UNet output convolution's own layout [B][eps_hw][4] (x, hist and noise stay CHW [B][4][eps_hw]).
// x_out may be x and hist_out may be hist_in: element i is read and written by the same thread only.
// One element of the update.  SEEDED: z is drawn where the other flavour reads noise[i] - normal_counter(bases.base[b], j) for element j of sample b (chw
// elements per sample, counter_rng.h) - and its term is always added; without it the instantiation is the kernel as it always was.
template <bool SEEDED, class Post = StoreAsIs>
__device__ __forceinline__ int sampler_step_element(int64_t i, const float* x, const float* __restrict__ eps,
                                                    const float* __restrict__ eps_u, float cfg_scale, const float* hist_in,
                                                    const float* __restrict__ noise, const NormalBases& bases, int64_t chw,
                                                    const SamplerCoeffs& c, int eps_hw, float* x_out, float* hist_out,
                                                    const Post& post = Post()) {
#pragma clang fp contract(off)
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
  if constexpr (SEEDED) {
    const int64_t b = i / chw;
    const float tn = c.c_n * normal_counter(bases.base[b], (uint64_t)(i - b * chw));
    o = o + tn;
  } else {
    if (noise) {
      const float tn = c.c_n * noise[i];
      o = o + tn;
    }
  }
  if (hist_out) {
    const float se = c.sigma_t * e;
    const float xs = xv - se;
    hist_out[i] = xs / c.alpha_t;
  }
  int nbad = nonfinite_f(o);  // a non-finite UNet output (fp16 overflow upstream) lands here every step
  x_out[i] = post(i, o, nbad);
  return nbad;
}

// ---- the same update for a model output that means v = alpha e - sigma x0 (Salimans & Ho 2022; kernels_vpred.hip) ------------
// x0 = alpha_t x - sigma_t v and e = sigma_t x + alpha_t v, so the scalars fold into c_x and c.c_e (which multiplies v here) on the host
// and x_out is sampler_step_element's sequence with v in place of e: the same operations in the same order, ONE fp32 rounding each.
// What differs is the history store,
//   hx = alpha_t x ; hv = sigma_t v ; h_out = hx - hv
// which divides by nothing: at the terminal step of a zero-terminal-SNR table (alpha_t = 0, sigma_t = 1) it is 0 - v = -v exactly,
// where the eps form is 0 / 0.  Roundings on the longest path
//   x_out: v (sub, mul, add) -> * c_v -> + c_x x -> + c_h h -> + c_n z = 7;   h_out: v (3) -> * sigma_t -> hx - . = 5
// which is what tests/test_gpu_vpred.py bounds the kernels with.  A sibling of sampler_step_element, not a parameter of it: the eps
// instantiations keep the instruction streams they were blessed with (isa_contract.json).
template <bool SEEDED, class Post = StoreAsIs>
__device__ __forceinline__ int sampler_step_v_element(int64_t i, const float* x, const float* __restrict__ vp,
                                                      const float* __restrict__ vp_u, float cfg_scale, const float* hist_in,
                                                      const float* __restrict__ noise, const NormalBases& bases, int64_t chw,
                                                      const SamplerCoeffs& c, int eps_hw, float* x_out, float* hist_out,
                                                      const Post& post = Post()) {
#pragma clang fp contract(off)
  int64_t ie = i;
  if (eps_hw > 0) {
    const int64_t bc = i / eps_hw, pix = i - bc * eps_hw, b = bc >> 2;
    ie = (b * eps_hw + pix) * 4 + (bc & 3);
  }
  float v = vp[ie];
  if (vp_u) {
    const float u = vp_u[ie];
    const float d = v - u;
    const float ds = d * cfg_scale;
    v = ds + u;
  }
  const float xv = x[i];
  float o = c.c_x * xv;
  const float tv = c.c_e * v;
  o = o + tv;
  if (hist_in) {
    const float th = c.c_h * hist_in[i];
    o = o + th;
  }
  if constexpr (SEEDED) {
    const int64_t b = i / chw;
    const float tn = c.c_n * normal_counter(bases.base[b], (uint64_t)(i - b * chw));
    o = o + tn;
  } else {
    if (noise) {
      const float tn = c.c_n * noise[i];
      o = o + tn;
    }
  }
  if (hist_out) {
    const float hx = c.alpha_t * xv;
    const float hv = c.sigma_t * v;
    hist_out[i] = hx - hv;
  }
  int nbad = nonfinite_f(o);  // a non-finite UNet output (fp16 overflow upstream) lands here every step
  x_out[i] = post(i, o, nbad);
  return nbad;
}
