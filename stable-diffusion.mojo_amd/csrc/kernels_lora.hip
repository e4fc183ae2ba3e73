// kernels_lora.hip - low-rank (LoRA) merge into ONE packed fp16 weight parameter, in place in its device layout:
//   W'[o][c] = rn16( (float)W[o][c] + s * sum_j up[o - row0][j] * down[j][c] )      for row0 <= o < row0 + rows, c < cols
// A load-time kernel: exactness first, no tuning.  The product runs on the exact-fp32 matrix instruction (v_mfma_f32_16x16x4_f32:
// fp32 operands, fp32 accumulate - numerically a k-ordered fmaf chain), never on the fp16 one, whose operands would be rounded.
// Callers speak reference coordinates only: o is a row of the reference tensor, c a column in the reference order (i for a linear
// layer, i * k * k + tap for a convolution); the GEGLU row interleave (k_pack_linear) and the tap-major K of the packed convolution
// (k_pack_conv) are resolved here.  Nothing but the addressed elements is written: no pad row, no pad channel, no other row.
#include "common.h"
#include "lds_dma.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int LORA_TM = 16;    // reference rows per workgroup
constexpr int LORA_TN = 128;   // reference columns per workgroup: 4 waves x 2 tiles of 16
constexpr int LORA_KC = 32;    // rank chunk staged in LDS (a multiple of the instruction's K = 4)

struct LoraArgs {
  half_t* W;          // packed parameter: linear [N][ld], convolution [Opad][kk][ld]
  const float* up;    // [rows][rank]
  const float* down;  // [rank][cols]
  int N, I, kk, ld, inter;  // reference rows, input channels, taps (1: linear), packed pitch (Kpad / Ipad), GEGLU row interleave
  int row0, rows, cols, rank;
  float scale;
};

// packed position of reference element (o, c)
__device__ __forceinline__ int64_t lora_packed_index(const LoraArgs& a, int o, int c) {
  const int prow = a.inter ? (o < a.N / 2 ? 2 * o : 2 * (o - a.N / 2) + 1) : o;
  const int i = c / a.kk, tap = c - i * a.kk;
  return ((int64_t)prow * a.kk + tap) * a.ld + i;
}

__global__ __launch_bounds__(256) void k_lora_merge(LoraArgs a, int* __restrict__ nonfinite) {
  // the rank is padded to the chunk with zeros HERE (rows past `rows` and columns past `cols` as well): a zero operand pair adds an exact 0
  __shared__ float s_up[LORA_TM][LORA_KC + 1];
  __shared__ float s_dn[LORA_KC][LORA_TN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r0 = blockIdx.y * LORA_TM, c0 = blockIdx.x * LORA_TN;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};  // two independent accumulators per wave: columns [0,16) and [16,32) of its slice
  const int ar = lane & 15, ak = lane >> 4, cw = wave * 32;
  for (int k0 = 0; k0 < a.rank; k0 += LORA_KC) {
    for (int e = tid; e < LORA_TM * LORA_KC; e += 256) {
      const int r = e / LORA_KC, k = e % LORA_KC;
      s_up[r][k] = (r0 + r < a.rows && k0 + k < a.rank) ? a.up[(int64_t)(r0 + r) * a.rank + k0 + k] : 0.f;
    }
    for (int e = tid; e < LORA_KC * LORA_TN; e += 256) {
      const int k = e / LORA_TN, c = e % LORA_TN;
      s_dn[k][c] = (k0 + k < a.rank && c0 + c < a.cols) ? a.down[(int64_t)(k0 + k) * a.cols + c0 + c] : 0.f;
    }
    tsd_jitter();
    __syncthreads();
#pragma unroll
    for (int kq = 0; kq < LORA_KC; kq += 4) {  // lane l: A[l & 15][l >> 4], B[l >> 4][l & 15]
      const float av = s_up[ar][kq + ak];
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_dn[kq + ak][cw + ar], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s_dn[kq + ak][cw + 16 + ar], acc1, 0, 0, 0);
    }
    tsd_jitter();  // the next rank chunk overwrites s_up / s_dn: a wave still in its MFMAs meets a wave that is early staging
    __syncthreads();
  }
  // C / D: column = lane & 15, row = 4 * (lane >> 4) + register
  int nbad = 0;
#pragma unroll
  for (int t = 0; t < 2; t++) {
    const int c = c0 + cw + 16 * t + (lane & 15);
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int lr = r0 + 4 * (lane >> 4) + j;
      if (lr < a.rows && c < a.cols) {
        const int64_t at = lora_packed_index(a, a.row0 + lr, c);
        const float d = t ? acc1[j] : acc0[j];
        const half_t h = (half_t)((float)a.W[at] + a.scale * d);  // ONE rounding to fp16, nearest-even
        a.W[at] = h;
        nbad += nonfinite_f((float)h);
      }
    }
  }
  nonfinite_report(nonfinite, nbad);
}

// W: packed linear [N][Kpad] (k = 0; `interleave`: GEGLU row interleave) or packed convolution [Opad][k * k][Ipad] (k = 1, 3); `ld` is
// Kpad / Ipad.  up [rows][rank], down [rank][I * max(k * k, 1)] are device fp32.  The caller has checked the row range against N.
int launch_lora_merge(tsd_ctx* ctx, half_t* W, int N, int I, int k, int ld, int interleave, int row0, int rows, const float* up,
                      const float* down, int rank, float scale) {
  if (!ctx->launch()) return TSD_OK;
  if (!W || !up || !down || N <= 0 || I <= 0 || I > ld || (k != 0 && k != 1 && k != 3) || row0 < 0 || rows <= 0 || row0 > N - rows ||
      rank < 1 || (interleave && (k != 0 || (N & 1))))
    TSD_FAIL(TSD_E_ARG, "lora merge: bad launch N=%d I=%d k=%d ld=%d rows [%d, +%d) rank=%d", N, I, k, ld, row0, rows, rank);
  LoraArgs a;
  a.W = W; a.up = up; a.down = down;
  a.N = N; a.I = I; a.kk = k ? k * k : 1; a.ld = ld; a.inter = interleave ? 1 : 0;
  a.row0 = row0; a.rows = rows; a.cols = I * a.kk; a.rank = rank; a.scale = scale;
  const dim3 grid(ceil_div(a.cols, LORA_TN), ceil_div(rows, LORA_TM));
  hipLaunchKernelGGL(k_lora_merge, grid, dim3(256), 0, ctx->stream, a, ctx->status);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
