// kernels_fp8.hip - the opt-in FP8 feed-forward: an OCP e4m3 row quantiser and a GEMM on v_mfma_f32_16x16x128_f8f6f4.
//
// k_quant_rows_e4m3: x [M][K] fp16 (pitch ld) -> q [M][Kp] e4m3 bytes, Kp = round_up(K, 128), and one fp32 scale per row.  Per row, in fp32:
//     amax = max |x|     scale = amax / 448 (1 where amax == 0)     inv = 448 / amax
//     q[k] = e4m3_rne(clamp(float(x[k]) * inv, -448, 448))          bytes K .. Kp - 1 are +0
// A row that holds an inf or a NaN gets scale = NaN and bytes of zero: whatever multiplies it comes out NaN, never silently finite.
// One wave owns one row and four waves share a workgroup (they never meet: no LDS, no barrier).  Lane l holds the 16-byte chunks
// l, l + 64, .. of the row in registers (NI chunks: K <= 512 NI, so 5120 columns are 80 halves per lane) between the amax reduction - a
// butterfly over the 64 lanes, exact in any order - and the conversion: ONE pass over HBM, 16-byte loads, 8-byte stores.  Packed LinW rows
// [N][Kpad] go through the same kernel; their scales are then per output channel.
//
// k_gemm_e4m3: out[m][n] = rn16(epi(sa[m] * sw[n] * sum_k A8[m][k] W8[n][k])) over Kp bytes per row, fp32 accumulation.
//   * 256 threads, a 128 x 128 output tile, K steps of 128 bytes.  The four waves own 64 x 64 each as 4 x 4 MFMA tiles: 64 accumulator
//     registers, 8 per operand fragment.
//   * The operands are SWAPPED into the instruction: the W rows go in as its A matrix and the activation rows as its B matrix, so
//     accumulator r of lane l is out[m = l % 16][n = 4 (l / 16) + r].  A lane then owns four CONSECUTIVE output columns of one row: bias is
//     one 16-byte load, the residual one 8-byte load, the store one 8-byte store, and GEGLU's interleaved (a, gate) pairs sit in one lane -
//     no cross-lane traffic in any epilogue.
//   * Fragment of a 16-row group: lane l supplies row l % 16, k-bytes 32 (l / 16) .. + 31 (two ds_read_b128).  Both operands use the same
//     k map, so the sum does not depend on how the instruction numbers k inside a lane.
//   * LDS: A and W tiles of 128 rows x 128 bytes, double-buffered: 4 x 16 KB = 64 KB.  Rows are 128 bytes, so the 16 lanes of a quarter
//     wave reading the same chunk of 16 consecutive rows would hit two bank groups 8 times each.  The 16-byte chunk index is XOR-swizzled
//     with (row >> 1) & 7 instead of padding the pitch (padding would leave the 64 KB): row parity picks the half of the banks, the
//     swizzle one of 8 chunks - 16 rows, 64 banks, no conflict, for the fragment reads and for the staging writes alike.
//   * Global -> LDS through registers: four 16-byte loads per operand and thread for tile t + 1 are issued before the MFMAs of tile t
//     and written to the other buffer after them; one barrier per K step.  The compiler's own waits; no counted s_waitcnt.
//   * Partial tiles: rows >= M / >= N are staged as zeros and never stored.  N is a multiple of 16, so a lane's four columns are all in
//     or all out.  No scratch, no atomics.
//
// MXFP4 weights (W4A8, tsd_model_set_ff_fp8(m, 2); OCP MX v1.0) - the second half of this file:
//
// k_quant_weights_mxfp4: w [N][K] fp16 (pitch ld, K a multiple of 32) -> e2m1 elements, two to a byte (low nibble first), and one e8m0 scale
//   byte per block of 32 consecutive k of a row, over Kp = round_up(K, 128) columns.  Per block, exact in fp32:
//     amax = max |w|     byte = floor(log2 amax) - 2 + 127     X = 2^(byte - 127)     nibble[k] = sign | e2m1_rne(min(|w[k]| / X, 6))
//   amax / X is in [4, 8): the largest element lands on 4 or 6 (7 X and above saturate to 6).  An all-zero block and the pad blocks are scale
//   byte 127 and zero nibbles.  A non-finite weight counts into the context's non-finite latch (there is no NaN in e2m1): the caller's
//   synchronisation point reports TSD_E_NONFINITE.  One lane owns one block: 64 bytes in, 16 bytes and one scale byte out; a wave owns the
//   16 rows x 4 blocks of one (n-block, k-step) with lane l on row l % 16, block l / 16 - the lane that will feed them to the matrix unit.
//   Output either plain row-major (elements [N][Kp / 2], scales [N][Kp / 32]: the op-level entry) or TILE-MAJOR for the GEMM: for n-block nb
//   and k-step kt, MX_TILE = 1088 bytes at ((nb nk) + kt) MX_TILE: the 64 lanes' 16-byte fragments (lane l at 16 l), then the 64 scale bytes
//   (lane l at 1024 + l).  Rows >= N of the last n-block are zero nibbles under byte 127.  k_tile_mxfp4 re-lays the plain form.
//
// k_gemm_e4m3_mxfp4: out[m][n] = rn16(epi(sa[m] * sum_k A8[m][k] * X[n][k / 32] * W4[n][k])), the same tile, wave and epilogue maps as
//   k_gemm_e4m3, the W rows again the instruction's A matrix - now with format selector 4 (e2m1) and the lane's own e8m0 byte as that
//   operand's block scale (byte 0 of the scale register, op_sel 0); the activation side stays e4m3 under the neutral byte 127.
//   * Lane l of a 16-row group supplies row l % 16 and, of the e2m1 operand, k 32 (l / 16) .. + 31 of the step: ONE MX block in ONE 16-byte
//     fragment, nibble i being k 32 (l / 16) + i, and the scale the instruction applies to a lane's 32 values is the byte that lane passes.
//     The e4m3 operand is numbered differently (g8_frag_mx below): the activation fragment is chunks l / 16 and l / 16 + 4 of the row.
//   * A goes through LDS exactly as above (swizzled chunks, two buffers: 32 KB).  W NEVER touches LDS: each wave loads the fragments and
//     scale bytes of its four n-blocks for step t + 1 straight from the tile-major stream - one coalesced 16-byte load and one byte load per
//     lane and n-block - before the MFMAs of step t.  The two waves that share an n-range read the same 4 KB; the second read is an L1 / L2 hit.
//   * Registers: 64 accumulators, 32 for the A fragments, 2 x 16 W fragments and 2 x 4 scales, 16 staging: two workgroups per CU
//     (__launch_bounds__(256, 2)).  A 128 x 256 tile would need 128 accumulators and 2 x 32 W registers on top of the same A side: one
//     workgroup per CU, and the feed-forward's N = C GEMM at M = 2048 already fills only 160 of 256 CUs with 128-wide tiles.
//   * No scratch, no atomics, the compiler's own waits.
#include <math.h>

#include "common.h"
#include "lds_dma.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int Q8_THREADS = 256, Q8_ROWS = Q8_THREADS / 64;
constexpr float E4M3_MAX = 448.f;

template <int NI>
__global__ void __launch_bounds__(Q8_THREADS) k_quant_rows_e4m3(const half_t* __restrict__ x, long long M, int K, int ld, int Kp, int vec,
                                                                uint8_t* __restrict__ q, float* __restrict__ scale) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * Q8_ROWS + wave;
  if (row >= M) return;  // uniform for the wave; the waves of a workgroup never meet
  const half_t* xr = x + row * ld;
  h8 v[NI];
  float amax = 0.f;
  bool bad = false;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int k0 = (lane + 64 * i) * 8;
    if (vec && k0 + 8 <= K) {
      v[i] = *(const h8*)(xr + k0);
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) v[i][j] = k0 + j < K ? xr[k0 + j] : (half_t)0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float a = fabsf((float)v[i][j]);
      bad |= !(a <= 65504.f);
      amax = fmaxf(amax, a);
    }
  }
#pragma unroll
  for (int o = 32; o; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
  bad = __builtin_amdgcn_ballot_w64(bad) != 0;
  const bool flat = bad || amax == 0.f;
  const float inv = flat ? 0.f : E4M3_MAX / amax;
  if (lane == 0) scale[row] = bad ? __builtin_nanf("") : (amax == 0.f ? 1.f : amax / E4M3_MAX);
  uint8_t* qr = q + row * Kp;
#pragma unroll
  for (int i = 0; i < NI; i++) {
    const int k0 = (lane + 64 * i) * 8;
    if (k0 >= Kp) continue;
    int w[2] = {0, 0};
    if (!bad) {
#pragma unroll
      for (int j = 0; j < 8; j += 2) {
        const float f0 = fminf(fmaxf((float)v[i][j] * inv, -E4M3_MAX), E4M3_MAX);
        const float f1 = fminf(fmaxf((float)v[i][j + 1] * inv, -E4M3_MAX), E4M3_MAX);
        w[j >> 2] = (j & 2) ? __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, w[j >> 2], true) : __builtin_amdgcn_cvt_pk_fp8_f32(f0, f1, w[j >> 2], false);
      }
    }
    *(int2*)(qr + k0) = make_int2(w[0], w[1]);
  }
}

int launch_quant_rows_e4m3(tsd_ctx* ctx, const half_t* x, int64_t M, int K, int ld, uint8_t* q, float* scale) {
  if (M <= 0 || M > ((int64_t)1 << 31) - 1 || K <= 0 || K > FP8_MAX_K || ld < K)
    TSD_FAIL(TSD_E_SHAPE, "quant_rows_e4m3: M=%lld K=%d (1..%d) pitch %d", (long long)M, K, FP8_MAX_K, ld);
  if (!ctx->launch()) return TSD_OK;
  if (((uintptr_t)q & 15) || ((uintptr_t)scale & 3)) TSD_FAIL(TSD_E_ARG, "quant_rows_e4m3: the byte rows are not 16-byte aligned");
  const int Kp = round_up(K, 128);
  const int vec = !((uintptr_t)x & 15) && ld % 8 == 0;
  const dim3 grid((unsigned)((M + Q8_ROWS - 1) / Q8_ROWS)), block(Q8_THREADS);
  ProfScope prof(ctx, KC_ELEMENTWISE);
  if (Kp <= 1024) hipLaunchKernelGGL(k_quant_rows_e4m3<2>, grid, block, 0, ctx->stream, x, (long long)M, K, ld, Kp, vec, q, scale);
  else if (Kp <= 2560) hipLaunchKernelGGL(k_quant_rows_e4m3<5>, grid, block, 0, ctx->stream, x, (long long)M, K, ld, Kp, vec, q, scale);
  else hipLaunchKernelGGL(k_quant_rows_e4m3<10>, grid, block, 0, ctx->stream, x, (long long)M, K, ld, Kp, vec, q, scale);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// ---- the GEMM ---------------------------------------------------------------------------------------------------------------------------
constexpr int G8_THREADS = 256, G8_BM = 128, G8_BN = 128, G8_BK = 128;
constexpr int G8_TILE = G8_BM * G8_BK;               // bytes of one operand tile (BM == BN)
constexpr int G8_CHUNKS = G8_TILE / 16 / G8_THREADS;  // 16-byte chunks a thread stages per operand and K step: 4

struct Fp8GemmK {
  const uint8_t* A8; const uint8_t* W8;
  const float* sa; const float* sw; const float* bias;
  const half_t* R; half_t* out;
  int M, N, Kp, ldr, ldo, epi;
};

// byte offset of 16-byte chunk c of row r in a swizzled tile
__device__ __forceinline__ int g8_off(int r, int c) { return r * G8_BK + ((c ^ ((r >> 1) & 7)) << 4); }

__device__ __forceinline__ v8i g8_frag(const uint8_t* tile, int r, int g) {
  const v4i lo = *(const v4i*)(tile + g8_off(r, 2 * g)), hi = *(const v4i*)(tile + g8_off(r, 2 * g + 1));
  v8i f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3]; f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

__global__ void __launch_bounds__(G8_THREADS) k_gemm_e4m3(Fp8GemmK p) {
  __shared__ __attribute__((aligned(16))) uint8_t sA[2][G8_TILE];
  __shared__ __attribute__((aligned(16))) uint8_t sW[2][G8_TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lg = lane >> 4;
  const int n0 = blockIdx.x * G8_BN, m0 = blockIdx.y * G8_BM;
  const int nk = p.Kp / G8_BK;

  // staging map: chunk id = tid + 256 i -> tile row id / 8, 16-byte chunk id % 8; rows beyond the operand are zeros
  const uint8_t* ga[G8_CHUNKS]; const uint8_t* gw[G8_CHUNKS];
  int so[G8_CHUNKS];
#pragma unroll
  for (int i = 0; i < G8_CHUNKS; i++) {
    const int id = tid + G8_THREADS * i, r = id >> 3, c = id & 7;
    so[i] = g8_off(r, c);
    ga[i] = m0 + r < p.M ? p.A8 + (int64_t)(m0 + r) * p.Kp + c * 16 : nullptr;
    gw[i] = n0 + r < p.N ? p.W8 + (int64_t)(n0 + r) * p.Kp + c * 16 : nullptr;
  }
  v4i ra[G8_CHUNKS], rw[G8_CHUNKS];
  auto fetch = [&](int kt) {
#pragma unroll
    for (int i = 0; i < G8_CHUNKS; i++) {
      ra[i] = ga[i] ? *(const v4i*)(ga[i] + (int64_t)kt * G8_BK) : v4i{0, 0, 0, 0};
      rw[i] = gw[i] ? *(const v4i*)(gw[i] + (int64_t)kt * G8_BK) : v4i{0, 0, 0, 0};
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < G8_CHUNKS; i++) {
      *(v4i*)(sA[buf] + so[i]) = ra[i];
      *(v4i*)(sW[buf] + so[i]) = rw[i];
    }
  };

  v4f acc[4][4];  // [jn][im]
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int i = 0; i < 4; i++) acc[j][i] = v4f{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const int buf = kt & 1;
    if (kt + 1 < nk) fetch(kt + 1);
    v8i fa[4];
#pragma unroll
    for (int i = 0; i < 4; i++) fa[i] = g8_frag(sA[buf], wm * 64 + i * 16 + lr, lg);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const v8i fw = g8_frag(sW[buf], wn * 64 + j * 16 + lr, lg);
#pragma unroll
      for (int i = 0; i < 4; i++)
        acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[i], acc[j][i], 0, 0, 0, 0, 0, 0);  // e4m3 x e4m3, neutral block scales
    }
    tsd_jitter();
    if (kt + 1 < nk) stage(buf ^ 1);  // the other buffer: every wave left it at the barrier that ended step kt - 1
    tsd_jitter();
    __syncthreads();
  }

  // epilogue: lane owns out[m][n .. n + 3], m = .. + lane % 16, n = .. + 4 (lane / 16)
  const bool geglu = p.epi & EPI_GEGLU;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int m = m0 + wm * 64 + i * 16 + lr;
    if (m >= p.M) continue;
    const float sam = p.sa[m];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = n0 + wn * 64 + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      const v4f swn = *(const v4f*)(p.sw + n);
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; r++) v[r] = acc[j][i][r] * (sam * swn[r]);
      if (p.epi & EPI_BIAS_N) {
        const v4f b = *(const v4f*)(p.bias + n);
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] += b[r];
      }
      if (p.epi & EPI_RESIDUAL) {
        const h4 rr = *(const h4*)(p.R + (int64_t)m * p.ldr + n);
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] += (float)rr[r];
      }
      if (geglu) {
        h2 o;
        o[0] = (half_t)(v[0] * gelu_tanh_f(v[1]));
        o[1] = (half_t)(v[2] * gelu_tanh_f(v[3]));
        *(h2*)(p.out + (int64_t)m * p.ldo + (n >> 1)) = o;
      } else {
        h4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = (half_t)v[r];
        *(h4*)(p.out + (int64_t)m * p.ldo + n) = o;
      }
    }
  }
}

int launch_gemm_e4m3(tsd_ctx* ctx, const Fp8GemmArgs& a) {
  if (a.M <= 0 || a.N <= 0 || a.N % 16 || a.K <= 0 || a.M > (1 << 30) / G8_BM || a.N > 65535 * G8_BN)
    TSD_FAIL(TSD_E_SHAPE, "gemm_e4m3: M=%lld N=%d (a multiple of 16) K=%d", (long long)a.M, a.N, a.K);
  if (a.epi & ~(EPI_BIAS_N | EPI_RESIDUAL | EPI_GEGLU)) TSD_FAIL(TSD_E_ARG, "gemm_e4m3: epilogue %d (bias, residual, GEGLU)", a.epi);
  if ((a.epi & EPI_GEGLU) && (a.epi & EPI_RESIDUAL)) TSD_FAIL(TSD_E_ARG, "gemm_e4m3: GEGLU takes no residual");
  const int width = (a.epi & EPI_GEGLU) ? a.N / 2 : a.N, lda = (a.epi & EPI_GEGLU) ? 2 : 4;
  if (a.ldo < width || a.ldo % lda) TSD_FAIL(TSD_E_SHAPE, "gemm_e4m3: output pitch %d (>= %d, a multiple of %d)", a.ldo, width, lda);
  if ((a.epi & EPI_RESIDUAL) && (a.ldr < a.N || a.ldr % 4)) TSD_FAIL(TSD_E_SHAPE, "gemm_e4m3: residual pitch %d (>= %d, a multiple of 4)", a.ldr, a.N);
  if (!ctx->launch()) return TSD_OK;
  if (!a.A8 || !a.W8 || !a.sa || !a.sw || !a.out || ((a.epi & EPI_BIAS_N) && !a.bias) || ((a.epi & EPI_RESIDUAL) && !a.R))
    TSD_FAIL(TSD_E_ARG, "gemm_e4m3: NULL operand");
  if (((uintptr_t)a.A8 & 15) || ((uintptr_t)a.W8 & 15) || ((uintptr_t)a.sw & 15) || ((uintptr_t)a.bias & 15) || ((uintptr_t)a.R & 7) ||
      ((uintptr_t)a.out & 7))
    TSD_FAIL(TSD_E_ARG, "gemm_e4m3: an operand is not aligned (16 bytes: byte rows, scales, bias; 8: residual, output)");
  Fp8GemmK k;
  k.A8 = a.A8; k.W8 = a.W8; k.sa = a.sa; k.sw = a.sw; k.bias = a.bias; k.R = a.R; k.out = a.out;
  k.M = (int)a.M; k.N = a.N; k.Kp = round_up(a.K, 128); k.ldr = a.ldr; k.ldo = a.ldo; k.epi = a.epi;
  ProfScope prof(ctx, KC_GEMM, (int)a.M, a.N, k.Kp, 1);
  hipLaunchKernelGGL(k_gemm_e4m3, dim3((unsigned)ceil_div(a.N, G8_BN), (unsigned)ceil_div((int)a.M, G8_BM)), dim3(G8_THREADS), 0, ctx->stream, k);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// ---- MXFP4 weights: the quantiser, the re-tiler -------------------------------------------------------------------------------------------
constexpr int MX_THREADS = 256, MX_WAVES = MX_THREADS / 64;
constexpr int MX_FRAG_BYTES = 1024, MX_TILE = MX_FRAG_BYTES + 64;  // one (16-row n-block, 128-wide k-step): 64 fragments, 64 scale bytes
constexpr int E8M0_ONE = 127;

size_t mxfp4_stream_bytes(int N, int K) { return (size_t)ceil_div(N, 16) * (round_up(K, 128) / 128) * MX_TILE; }

// where lane `lane` of tile (nb, kt) keeps its fragment; its scale byte is MX_FRAG_BYTES - 15 lane further on
__device__ __forceinline__ size_t mx_frag_off(int nb, int kt, int nk, int lane) { return ((size_t)nb * nk + kt) * MX_TILE + lane * 16; }
__device__ __forceinline__ size_t mx_scale_off(int nb, int kt, int nk, int lane) { return ((size_t)nb * nk + kt) * MX_TILE + MX_FRAG_BYTES + lane; }

// e2m1 code of a >= 0 (values 0, .5, 1, 1.5, 2, 3, 4, 6), nearest, ties to the even code, saturating
__device__ __forceinline__ int e2m1_rne(float a) {
  return (a > 0.25f) + (a >= 0.75f) + (a > 1.25f) + (a >= 1.75f) + (a > 2.5f) + (a >= 3.5f) + (a > 5.f);
}

template <bool TILED>
__global__ void __launch_bounds__(MX_THREADS) k_quant_weights_mxfp4(const half_t* __restrict__ w, int N, int K, int ld, int nk, int vec,
                                                                    uint8_t* __restrict__ elems, uint8_t* __restrict__ scales, int* status) {
  const int lane = threadIdx.x & 63;
  const long long tile = (long long)blockIdx.x * MX_WAVES + (threadIdx.x >> 6);
  const int nb = (int)(tile / nk), kt = (int)(tile % nk);
  if (nb >= (N + 15) / 16) return;
  const int row = nb * 16 + (lane & 15), kb = kt * 4 + (lane >> 4);
  const bool live = row < N && kb * 32 < K;  // K is a multiple of 32: a block is all weights or all pad
  h8 v[4];
  float amax = 0.f;
  int bad = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const half_t* src = w + (long long)row * ld + kb * 32 + i * 8;
    if (live && vec) {
      v[i] = *(const h8*)src;
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) v[i][j] = live ? src[j] : (half_t)0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float a = fabsf((float)v[i][j]);
      bad += !(a <= 65504.f);
      amax = fmaxf(amax, a);
    }
  }
  if (bad) nonfinite_report(status, bad);
  // every fp16 magnitude is a normal fp32: its exponent field E is floor(log2 amax) + 127.  X = 2^(E - 129), 1 / X = 2^(129 - E)
  const unsigned E = __float_as_uint(amax) >> 23;
  const bool flat = bad || amax == 0.f;
  const float inv = __uint_as_float((256u - E) << 23);
  v4i q = {0, 0, 0, 0};
  if (!flat) {
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float f = (float)v[i][j];
        q[i] |= (e2m1_rne(fabsf(f) * inv) | (__float_as_uint(f) >> 28 & 8)) << (4 * j);
      }
  }
  const uint8_t byte = flat ? E8M0_ONE : (uint8_t)(E - 2);
  if (TILED) {
    *(v4i*)(elems + mx_frag_off(nb, kt, nk, lane)) = q;
    elems[mx_scale_off(nb, kt, nk, lane)] = byte;
  } else if (row < N) {
    *(v4i*)(elems + (size_t)row * (nk * 64) + kb * 16) = q;
    scales[(size_t)row * (nk * 4) + kb] = byte;
  }
}

// plain elements [N][64 nk] and scales [N][4 nk] -> the tile-major stream
__global__ void __launch_bounds__(MX_THREADS) k_tile_mxfp4(const uint8_t* __restrict__ elems, const uint8_t* __restrict__ scales, int N, int nk,
                                                           uint8_t* __restrict__ stream) {
  const int lane = threadIdx.x & 63;
  const long long tile = (long long)blockIdx.x * MX_WAVES + (threadIdx.x >> 6);
  const int nb = (int)(tile / nk), kt = (int)(tile % nk);
  if (nb >= (N + 15) / 16) return;
  const int row = nb * 16 + (lane & 15), kb = kt * 4 + (lane >> 4);
  const bool live = row < N;
  *(v4i*)(stream + mx_frag_off(nb, kt, nk, lane)) = live ? *(const v4i*)(elems + (size_t)row * (nk * 64) + kb * 16) : v4i{0, 0, 0, 0};
  stream[mx_scale_off(nb, kt, nk, lane)] = live ? scales[(size_t)row * (nk * 4) + kb] : (uint8_t)E8M0_ONE;
}

// one wave per (n-block, k-step) tile
static unsigned mx_grid(int N, int nk) { return (unsigned)(((long long)ceil_div(N, 16) * nk + MX_WAVES - 1) / MX_WAVES); }
static int mx_shape_ok(const char* who, int N, int K, int ld) {
  if (N <= 0 || N > (1 << 20) || K <= 0 || K % 32 || K > (1 << 17) || ld < K)
    TSD_FAIL(TSD_E_SHAPE, "%s: N=%d K=%d (a multiple of 32) pitch %d", who, N, K, ld);
  return TSD_OK;
}

int launch_quant_weights_mxfp4(tsd_ctx* ctx, const half_t* w, int N, int K, int ld, uint8_t* elems, uint8_t* scales) {
  TSD_TRY(mx_shape_ok("quant_weights_mxfp4", N, K, ld));
  if (!ctx->launch()) return TSD_OK;
  if (((uintptr_t)elems & 15)) TSD_FAIL(TSD_E_ARG, "quant_weights_mxfp4: the element rows are not 16-byte aligned");
  const int nk = round_up(K, 128) / 128, vec = !((uintptr_t)w & 15) && ld % 8 == 0;
  const dim3 grid(mx_grid(N, nk)), block(MX_THREADS);
  ProfScope prof(ctx, KC_ELEMENTWISE);
  if (scales) hipLaunchKernelGGL(k_quant_weights_mxfp4<false>, grid, block, 0, ctx->stream, w, N, K, ld, nk, vec, elems, scales, ctx->status);
  else hipLaunchKernelGGL(k_quant_weights_mxfp4<true>, grid, block, 0, ctx->stream, w, N, K, ld, nk, vec, elems, scales, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

int launch_tile_mxfp4(tsd_ctx* ctx, const uint8_t* elems, const uint8_t* scales, int N, int K, uint8_t* stream) {
  TSD_TRY(mx_shape_ok("tile_mxfp4", N, K, K));
  if (!ctx->launch()) return TSD_OK;
  if (((uintptr_t)elems & 15) || ((uintptr_t)stream & 15)) TSD_FAIL(TSD_E_ARG, "tile_mxfp4: the element rows / the stream are not 16-byte aligned");
  const int nk = round_up(K, 128) / 128;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_tile_mxfp4, dim3(mx_grid(N, nk)), dim3(MX_THREADS), 0, ctx->stream,
                     elems, scales, N, nk, stream);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// ---- the W4A8 GEMM ------------------------------------------------------------------------------------------------------------------------
struct Mx4GemmK {
  const uint8_t* A8; const uint8_t* W4;
  const float* sa; const float* bias;
  const half_t* R; half_t* out;
  int M, N, Kp, ldr, ldo, epi;
};

// The instruction numbers k differently per format (measured with one-hot operands): lane group g = lane / 16 holds
// k 32 g .. 32 g + 31 of an e2m1 operand in its four registers, but of an e4m3 operand k 16 g .. + 15 in registers 0 - 3 and
// 64 + 16 g .. + 15 in registers 4 - 7.  So the activation fragment is the 16-byte chunks g and g + 4 of the row (k_gemm_e4m3 takes 2 g and
// 2 g + 1 for BOTH operands, which is the same sum); the swizzle spreads the sixteen rows of either chunk over all banks as before.
__device__ __forceinline__ v8i g8_frag_mx(const uint8_t* tile, int r, int g) {
  const v4i lo = *(const v4i*)(tile + g8_off(r, g)), hi = *(const v4i*)(tile + g8_off(r, g + 4));
  v8i f;
  f[0] = lo[0]; f[1] = lo[1]; f[2] = lo[2]; f[3] = lo[3]; f[4] = hi[0]; f[5] = hi[1]; f[6] = hi[2]; f[7] = hi[3];
  return f;
}

__global__ void __launch_bounds__(G8_THREADS, 2) k_gemm_e4m3_mxfp4(Mx4GemmK p) {
  __shared__ __attribute__((aligned(16))) uint8_t sA[2][G8_TILE];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int wm = wave >> 1, wn = wave & 1, lr = lane & 15, lg = lane >> 4;
  const int n0 = blockIdx.x * G8_BN, m0 = blockIdx.y * G8_BM;
  const int nk = p.Kp / G8_BK;

  // A: the staging map of k_gemm_e4m3
  const uint8_t* ga[G8_CHUNKS];
  int so[G8_CHUNKS];
#pragma unroll
  for (int i = 0; i < G8_CHUNKS; i++) {
    const int id = tid + G8_THREADS * i, r = id >> 3, c = id & 7;
    so[i] = g8_off(r, c);
    ga[i] = m0 + r < p.M ? p.A8 + (int64_t)(m0 + r) * p.Kp + c * 16 : nullptr;
  }
  v4i ra[G8_CHUNKS];
  auto fetch = [&](int kt) {
#pragma unroll
    for (int i = 0; i < G8_CHUNKS; i++) ra[i] = ga[i] ? *(const v4i*)(ga[i] + (int64_t)kt * G8_BK) : v4i{0, 0, 0, 0};
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < G8_CHUNKS; i++) *(v4i*)(sA[buf] + so[i]) = ra[i];
  };
  // W: this lane's fragment and scale byte in step 0 of the wave's four n-blocks; an n-block beyond N is zeros under the neutral scale
  const uint8_t* gf[4]; const uint8_t* gs[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int nb = (n0 + wn * 64 + j * 16) >> 4;
    const bool in = nb * 16 < p.N;
    gf[j] = in ? p.W4 + mx_frag_off(nb, 0, nk, lane) : nullptr;
    gs[j] = in ? p.W4 + mx_scale_off(nb, 0, nk, lane) : nullptr;
  }
  v4i wc[4], wx[4];
  int sc[4], sx[4];
  auto fetch_w = [&](int kt, v4i* f, int* s) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      f[j] = gf[j] ? *(const v4i*)(gf[j] + (size_t)kt * MX_TILE) : v4i{0, 0, 0, 0};
      s[j] = gs[j] ? (int)gs[j][(size_t)kt * MX_TILE] : E8M0_ONE;
    }
  };

  v4f acc[4][4];  // [jn][im]
#pragma unroll
  for (int j = 0; j < 4; j++)
#pragma unroll
    for (int i = 0; i < 4; i++) acc[j][i] = v4f{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  fetch_w(0, wc, sc);
  stage(0);
  __syncthreads();
  for (int kt = 0; kt < nk; kt++) {
    const int buf = kt & 1;
    const bool more = kt + 1 < nk;
    if (more) fetch(kt + 1);
    fetch_w(more ? kt + 1 : kt, wx, sx);  // (the last step re-reads its own tile: in bounds, never used)
    v8i fa[4];
#pragma unroll
    for (int i = 0; i < 4; i++) fa[i] = g8_frag_mx(sA[buf], wm * 64 + i * 16 + lr, lg);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const v8i fw = {wc[j][0], wc[j][1], wc[j][2], wc[j][3], 0, 0, 0, 0};  // e2m1: the instruction reads the first four registers
#pragma unroll
      for (int i = 0; i < 4; i++)
        acc[j][i] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw, fa[i], acc[j][i], 4, 0, 0, sc[j], 0, E8M0_ONE);  // e2m1 (block scale) x e4m3
    }
    tsd_jitter();
    if (more) stage(buf ^ 1);  // the other buffer: every wave left it at the barrier that ended step kt - 1
    tsd_jitter();
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; j++) { wc[j] = wx[j]; sc[j] = sx[j]; }
  }

  // epilogue: lane owns out[m][n .. n + 3], m = .. + lane % 16, n = .. + 4 (lane / 16)
  const bool geglu = p.epi & EPI_GEGLU;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int m = m0 + wm * 64 + i * 16 + lr;
    if (m >= p.M) continue;
    const float sam = p.sa[m];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int n = n0 + wn * 64 + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; r++) v[r] = acc[j][i][r] * sam;
      if (p.epi & EPI_BIAS_N) {
        const v4f b = *(const v4f*)(p.bias + n);
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] += b[r];
      }
      if (p.epi & EPI_RESIDUAL) {
        const h4 rr = *(const h4*)(p.R + (int64_t)m * p.ldr + n);
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] += (float)rr[r];
      }
      if (geglu) {
        h2 o;
        o[0] = (half_t)(v[0] * gelu_tanh_f(v[1]));
        o[1] = (half_t)(v[2] * gelu_tanh_f(v[3]));
        *(h2*)(p.out + (int64_t)m * p.ldo + (n >> 1)) = o;
      } else {
        h4 o;
#pragma unroll
        for (int r = 0; r < 4; r++) o[r] = (half_t)v[r];
        *(h4*)(p.out + (int64_t)m * p.ldo + n) = o;
      }
    }
  }
}

int launch_gemm_e4m3_mxfp4(tsd_ctx* ctx, const Fp8GemmArgs& a) {
  if (a.M <= 0 || a.N <= 0 || a.N % 16 || a.K <= 0 || a.M > (1 << 30) / G8_BM || a.N > 65535 * G8_BN)
    TSD_FAIL(TSD_E_SHAPE, "gemm_e4m3_mxfp4: M=%lld N=%d (a multiple of 16) K=%d", (long long)a.M, a.N, a.K);
  if (a.epi & ~(EPI_BIAS_N | EPI_RESIDUAL | EPI_GEGLU)) TSD_FAIL(TSD_E_ARG, "gemm_e4m3_mxfp4: epilogue %d (bias, residual, GEGLU)", a.epi);
  if ((a.epi & EPI_GEGLU) && (a.epi & EPI_RESIDUAL)) TSD_FAIL(TSD_E_ARG, "gemm_e4m3_mxfp4: GEGLU takes no residual");
  const int width = (a.epi & EPI_GEGLU) ? a.N / 2 : a.N, lda = (a.epi & EPI_GEGLU) ? 2 : 4;
  if (a.ldo < width || a.ldo % lda) TSD_FAIL(TSD_E_SHAPE, "gemm_e4m3_mxfp4: output pitch %d (>= %d, a multiple of %d)", a.ldo, width, lda);
  if ((a.epi & EPI_RESIDUAL) && (a.ldr < a.N || a.ldr % 4))
    TSD_FAIL(TSD_E_SHAPE, "gemm_e4m3_mxfp4: residual pitch %d (>= %d, a multiple of 4)", a.ldr, a.N);
  if (!ctx->launch()) return TSD_OK;
  if (!a.A8 || !a.W4 || !a.sa || !a.out || ((a.epi & EPI_BIAS_N) && !a.bias) || ((a.epi & EPI_RESIDUAL) && !a.R))
    TSD_FAIL(TSD_E_ARG, "gemm_e4m3_mxfp4: NULL operand");
  if (((uintptr_t)a.A8 & 15) || ((uintptr_t)a.W4 & 15) || ((uintptr_t)a.bias & 15) || ((uintptr_t)a.R & 7) || ((uintptr_t)a.out & 7))
    TSD_FAIL(TSD_E_ARG, "gemm_e4m3_mxfp4: an operand is not aligned (16 bytes: byte rows, weight stream, bias; 8: residual, output)");
  Mx4GemmK k;
  k.A8 = a.A8; k.W4 = a.W4; k.sa = a.sa; k.bias = a.bias; k.R = a.R; k.out = a.out;
  k.M = (int)a.M; k.N = a.N; k.Kp = round_up(a.K, 128); k.ldr = a.ldr; k.ldo = a.ldo; k.epi = a.epi;
  ProfScope prof(ctx, KC_GEMM, (int)a.M, a.N, k.Kp, 1);
  hipLaunchKernelGGL(k_gemm_e4m3_mxfp4, dim3((unsigned)ceil_div(a.N, G8_BN), (unsigned)ceil_div((int)a.M, G8_BM)), dim3(G8_THREADS), 0, ctx->stream, k);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
