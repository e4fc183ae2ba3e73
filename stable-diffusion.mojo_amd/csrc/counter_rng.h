// counter_rng.h - the counter RNG of the device: value = f(seed, stream, element counter), no state.  Included by every kernel file that
// draws from it (kernels_elementwise.hip: k_fill_uniform, the seeded DDPM update; kernels_sampler.hip: k_fill_normal, the seeded
// linear-multistep update), so the inline draw of an update kernel and the fill kernel are ONE function and give the same bits.
// Host twins: tsd/rng.py (hash_u64 / uniform / normal_counter), oracle/rng.py.
#pragma once
#include <stdint.h>

// base of a (seed, stream) pair, on the host: the rule of launch_fill_uniform and rng.hash_u64 (uint64, wrapping)
inline uint64_t counter_rng_base(uint64_t seed, uint64_t stream) {
  return seed * 0x9E3779B97F4A7C15ull + stream * 0xBF58476D1CE4E5B9ull;
}
// up to 16 per-sample bases passed to a kernel by value (a session's UNet batch is <= 16): sample b of a launch draws from base[b]
struct NormalBases {
  uint64_t base[16];
};

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// N(0,1) value j of the stream `base` (Box-Muller, the cosine branch):
//   k1 = mix64(base + 2j) >> 40, k2 = mix64(base + 2j + 1) >> 40          24 bits each
//   u1 = (k1 + 1) 2^-24 in (0, 1], v = k2 2^-23 in [0, 2)                  both exact in fp32
//   z  = sqrt(-2 ln u1) * cos(pi v)                                        |z| <= sqrt(48 ln 2) = 5.77; k1 = 2^24 - 1 gives z = +-0
// Every operation is one fp32 rounding in this order (contraction into fma is off).  Against the float64 twin rng.normal_counter, which
// rounds to float32 once, the relative error is bounded by the library functions' own bounds (the device math library is built to
// OpenCL's: log <= 3 ulp, cospi <= 4 ulp; sqrtf is correctly rounded here):
//   ln u1        3 ulp       (relative to ln u1: u1 is exact, and so is the result 0 at u1 = 1)
//   * (-2)       exact
//   sqrt         halves what it is given (1.5 ulp) and adds 0.5 ulp
//   cospi(v)     4 ulp       (v is exact and the reduction of an exact argument is exact: the bound is relative down to cospi's zeros,
//                             which are exact zeros on both sides)
//   product      0.5 ulp
//   the twin's own rounding to float32: 0.5 ulp
// = 7 ulp, i.e. |z_dev - z_twin| <= 7 * 2^-23 |z_twin| = 14 * 2^-24 |z_twin|: the eps of tests/test_gpu_noise.py, under the 16 * 2^-24
// beyond which the device stream would not be the twin's.  Measured on an MI355X over that test's inputs: see the test's docstring.
__device__ __forceinline__ float normal_counter(uint64_t base, uint64_t j) {
#pragma clang fp contract(off)
  const uint64_t c = base + 2 * j;
  const uint32_t k1 = (uint32_t)(mix64(c) >> 40), k2 = (uint32_t)(mix64(c + 1) >> 40);
  const float u1 = (float)(k1 + 1u) * 5.9604644775390625e-08f;   // (k1 + 1) 2^-24: k1 + 1 <= 2^24, exact
  const float v = (float)k2 * 1.1920928955078125e-07f;           // k2 2^-23, exact
  const float l = logf(u1);
  const float m = -2.f * l;
  const float r = sqrtf(m);
  const float cs = cospif(v);
  return r * cs;
}
