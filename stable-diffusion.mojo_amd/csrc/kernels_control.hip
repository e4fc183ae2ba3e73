// kernels_control.hip - ControlNet injection (Zhang et al. 2023, "Adding Conditional Control to Text-to-Image Diffusion Models"): between
// the encoder and the decoder of the full-size UNet every skip tensor and the bottleneck output receive a residual of the control network,
// scaled per sample, in place:
//     y = rn16(fmaf(s_b, (float)r, (float)x))               fp32, ONE rounding to fp16, 16-byte NHWC loads and stores
// and the GroupNorm statistics their producers emitted for free (EPI_GNSTATS) are emitted again from the rounded y, so every consumer
// takes the branch it took before (the composite statistics over a concat included, which needs equal slab counts on both sources):
//     partial[(b * nslab + slab) * G + g] = (sum y, sum y^2)  fp32, into the tensor's own gn_buf, with its producer's G and nslab
// ONE launch serves all tensors: a by-value table (ControlTable, like SlotTable) of up to 16 entries with a block-range prefix.  A workgroup
// owns one (entry, sample, slab): grid (sum of the entries' slabs, B).  Slab `s` of an entry is pixels [s * sp, (s + 1) * sp) of the sample,
// sp = ceil(HW / nslab) - 32 rows where the producer emitted one slab per 32-row epilogue pass.  The thread map is k_gn_partial's (a thread
// keeps the same 8 channels and strides over the slab's pixels, per-channel sums in registers), and so is the reduction: through LDS in a
// fixed order, pixel lanes and then the channels of a group, no atomics.  A sample's y and partials are a function of its own x, r and s:
// the same bits in every batch position, run after run.
// The per-sample scale is a device fp32 [B] (CFG's cond-only control is scale 0 on the uncond half).  With `skip_zero` set (the graph sets
// it) a workgroup of a sample whose scale is exactly 0 returns before its first load: y == x, so the tensor and the statistics its producer
// emitted both stand as they are.
#include "common.h"
#include "lds_dma.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int CTL_THREADS = 256;
constexpr int CTL_MAX_PLC = 2048;  // pixel lanes x channels a workgroup reduces through LDS: 256 threads x 8 channels

__global__ void __launch_bounds__(CTL_THREADS) k_control_inject(ControlTable tab, const float* __restrict__ scale) {
  __shared__ float red[2 * CTL_MAX_PLC];  // [PL][2][C]
  const int b = blockIdx.y;
  // the entry of this block: the prefix is uniform, so this is a scalar loop over the argument segment
  int ei = 0;
  for (int i = 1; i < tab.n; i++)
    if ((int)blockIdx.x >= tab.e[i].blk0) ei = i;
  const ControlEntry& e = tab.e[ei];
  const float s = scale[b];
  if (tab.skip_zero && s == 0.f) return;
  const int slab = (int)blockIdx.x - e.blk0;
  const int C = e.C, nch = C >> 3;
  const int PL = CTL_THREADS / nch;
  const int tid = threadIdx.x;
  const int pl = tid / nch, ch = tid - pl * nch;
  const bool active = tid < PL * nch;
  const int sp = (e.HW + e.nslab - 1) / e.nslab;
  const int p_begin = slab * sp;
  const int p_end = min(e.HW, p_begin + sp);
  float a1[8], a2[8];
#pragma unroll
  for (int j = 0; j < 8; j++) a1[j] = a2[j] = 0.f;
  if (active) {
    for (int pix = p_begin + pl; pix < p_end; pix += PL) {
      const int64_t row = (int64_t)b * e.HW + pix;
      half_t* xp = e.x + row * e.ldx + ch * 8;
      const h8 xv = *(const h8*)xp;
      const h8 rv = *(const h8*)(e.r + row * e.ldr + ch * 8);
      h8 yv;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        yv[j] = (half_t)fmaf(s, (float)rv[j], (float)xv[j]);
        const float f = (float)yv[j];
        a1[j] += f;
        a2[j] = fmaf(f, f, a2[j]);
      }
      *(h8*)xp = yv;
    }
  }
  if (!e.part) return;  // the producer emitted no statistics: the consumer keeps its own pass (uniform for the block)
  if (active) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      red[(pl * 2 + 0) * C + ch * 8 + j] = a1[j];
      red[(pl * 2 + 1) * C + ch * 8 + j] = a2[j];
    }
  }
  tsd_jitter();
  __syncthreads();
  // fixed-order (deterministic) reduction: pixel lanes, then the channels of each group
  const int cpg = C / e.groups;
  for (int g = tid; g < e.groups; g += CTL_THREADS) {
    float t1 = 0.f, t2 = 0.f;
    for (int c = g * cpg; c < (g + 1) * cpg; c++)
      for (int l = 0; l < PL; l++) {
        t1 += red[(l * 2 + 0) * C + c];
        t2 += red[(l * 2 + 1) * C + c];
      }
    float* o = e.part + (((int64_t)b * e.nslab + slab) * e.groups + g) * 2;
    o[0] = t1;
    o[1] = t2;
  }
}

// Fills e.blk0 / tab.n from the entries' slab counts and launches.  Every entry: x and r 16-byte aligned with pitches that are multiples
// of 8, C a multiple of 8 up to 2048, 1 <= nslab <= HW; an entry with statistics (part != NULL): C a multiple of groups.
int launch_control_inject(tsd_ctx* ctx, ControlTable tab, int B, const float* scale) {
  if (tab.n <= 0 || tab.n > CONTROL_MAX_ENTRIES || B <= 0 || B > 16) TSD_FAIL(TSD_E_SHAPE, "control inject: %d entries (1..%d), B=%d (1..16)", tab.n, CONTROL_MAX_ENTRIES, B);
  if (!scale) TSD_FAIL(TSD_E_ARG, "control inject: the per-sample scales are required");
  int blocks = 0;
  for (int i = 0; i < tab.n; i++) {
    ControlEntry& e = tab.e[i];
    if (!e.x || !e.r) TSD_FAIL(TSD_E_ARG, "control inject: entry %d has no tensor / residual", i);
    if (e.C <= 0 || e.C % 8 || e.C > CTL_MAX_PLC || e.HW <= 0 || e.nslab <= 0 || e.nslab > e.HW || e.ldx < e.C || e.ldr < e.C || e.ldx % 8 || e.ldr % 8)
      TSD_FAIL(TSD_E_SHAPE, "control inject: entry %d: HW=%d C=%d pitches %d / %d nslab=%d", i, e.HW, e.C, e.ldx, e.ldr, e.nslab);
    if (ctx->launch() && (((uintptr_t)e.x | (uintptr_t)e.r) & 15)) TSD_FAIL(TSD_E_ARG, "control inject: entry %d is not 16-byte aligned", i);
    if (e.part && (e.groups <= 0 || e.C % e.groups)) TSD_FAIL(TSD_E_SHAPE, "control inject: entry %d: %d groups over %d channels", i, e.groups, e.C);
    if (!e.part) e.groups = 0;
    // the last slab must not be empty: ceil(HW / nslab) * (nslab - 1) < HW
    if ((int64_t)((e.HW + e.nslab - 1) / e.nslab) * (e.nslab - 1) >= e.HW) TSD_FAIL(TSD_E_SHAPE, "control inject: entry %d: %d slabs do not tile %d rows", i, e.nslab, e.HW);
    e.blk0 = blocks;
    blocks += e.nslab;
  }
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_control_inject, dim3((unsigned)blocks, (unsigned)B), dim3(CTL_THREADS), 0, ctx->stream, tab, scale);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
