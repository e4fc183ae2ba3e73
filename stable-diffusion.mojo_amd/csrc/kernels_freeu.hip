// kernels_freeu.hip - FreeU (Si et al. 2023, "FreeU: Free Lunch in Diffusion U-Net"): in front of every decoder concat of the full-size UNet
// the backbone half of the hidden tensor is scaled up and the lowest spatial frequencies of the popped skip are scaled down, both in place.
//
// Skip r [B][HW][Cr] (fp16 NHWC), s != 1.  diffusers' fourier_filter(x, threshold = 1, scale = s) multiplies exactly the four bins
// (fy, fx) in {0, -1}^2 of the plane's 2-D DFT by s.  For a real plane that is r + (s - 1) P(r) with P the projection on those bins, and
// P needs no transform: with cy[y] = cos(2 pi y / H), sy[y] = sin(2 pi y / H), cx / sx likewise over W, cxy = cy cx - sy sx and
// sxy = sy cx + cy sx, per (sample, channel) plane
//     S0 = sum r   Ay = sum r cy   By = sum r sy   Ax = sum r cx   Bx = sum r sx   Axy = sum r cxy   Bxy = sum r sxy
//     P[y,x] = (S0 + Ay cy + By sy + Ax cx + Bx sx + Axy cxy + Bxy sxy) / (H W)
//     r'[y,x] = rn16(r[y,x] + (s - 1) P[y,x])
// (H = 2 included: bin -1 is then the Nyquist bin, sy = 0 and the formula counts it once, as the mask does.)  The four 1-D tables are built
// on the host in double, rounded once to fp32 and kept on the context per (H, W) (freeu_tab), as the vision front end keeps its tables.
// Sums and P are fp32 in a fixed order, one rounding to fp16.
//
// Hidden h [B][HW][Ch], b != 1, channels c < Ch / 2 only (the other half is never written):
//     constant  (diffusers)               h' = rn16(b h)
//     modulated (the authors' "v2" form)  m[p] = (1 / Ch) sum_c h[p][c] over ALL Ch channels; lo / hi its minimum / maximum over the sample's
//                                         pixels; n[p] = (m[p] - lo) / (hi - lo), 0 where hi == lo; h' = rn16(((b - 1) n[p] + 1) h)
//
// ONE launch (k_freeu) serves both tensors: grid (hidden blocks + skip blocks, B), 256 threads.  The thread map is k_control_inject's: a
// thread keeps the same 8 channels (one 16-byte access) of a 64-channel chunk and strides over pixels in 32 pixel lanes.
//   * a skip block owns one (sample, 64-channel chunk): it loops over ALL pixels of the plane with the seven sums of its 8 channels in
//     registers, reduces the 32 pixel lanes through LDS in lane order, and loops over the pixels again to apply.  A channel's sums are a
//     function of its own plane: the same bits for every B, batch position and Cr.
//   * a hidden block owns one (sample, 64-channel chunk of the lower half, 256-pixel slab) - element-wise work, cut freely.  In modulated
//     mode it first finds lo / hi from the sample's row of means itself (minimum and maximum are exact in any order).
// The modulated mode has one short launch in front (k_freeu_mean): one wave per pixel, the lanes' partial sums combined in a fixed tree.
// No atomics, no scratch, no counted waits, no host round trip.
#include <math.h>

#include <algorithm>

#include "common.h"
#include "lds_dma.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int FU_THREADS = 256;
constexpr int FU_CHUNK = 64;               // channels per block: 8 threads of 8 channels
constexpr int FU_OCT = FU_CHUNK / 8;
constexpr int FU_PL = FU_THREADS / FU_OCT;  // 32 pixel lanes
constexpr int FU_SLAB = 8 * FU_PL;          // pixels per hidden block
constexpr int FU_SUMS = 7;

struct FreeuK {
  half_t* h;          // [B][HW][ldh] or nullptr: the hidden tensor stays as it is
  half_t* r;          // [B][HW][ldr] or nullptr: the skip stays as it is
  const float* tab;   // cy[H] sy[H] cx[W] sx[W]
  const float* mean;  // [B][HW]: modulated mode only
  int ldh, ldr, H, W, Ch, Cr;
  float b, b1;        // b and b - 1
  float g;            // (s - 1) / (H W)
  int hblocks, hslabs;
};

__global__ void __launch_bounds__(FU_THREADS) k_freeu_mean(const half_t* __restrict__ h, int ldh, int HW, int Ch, float* __restrict__ mean) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pix = blockIdx.x * (FU_THREADS / 64) + wave;
  if (pix >= HW) return;  // uniform for the wave
  const int b = blockIdx.y;
  const half_t* row = h + ((int64_t)b * HW + pix) * ldh;
  float a = 0.f;
  for (int o = lane; o < (Ch >> 3); o += 64) {
    const h8 v = *(const h8*)(row + o * 8);
#pragma unroll
    for (int j = 0; j < 8; j++) a += (float)v[j];
  }
  // fixed tree over the 64 lanes (lanes beyond the row's octets hold 0)
#pragma unroll
  for (int o = 32; o; o >>= 1) a += __shfl_down(a, o, 64);
  if (lane == 0) mean[(int64_t)b * HW + pix] = a / (float)Ch;
}

__global__ void __launch_bounds__(FU_THREADS) k_freeu(FreeuK k) {
  __shared__ float red[FU_SUMS * FU_PL * FU_CHUNK];  // [7][32 pixel lanes][64 channels]
  __shared__ float tot[FU_SUMS * FU_CHUNK];
  const int b = blockIdx.y;
  const int tid = threadIdx.x;
  const int oct = tid & (FU_OCT - 1), pl = tid >> 3;
  const int HW = k.H * k.W;
  if ((int)blockIdx.x < k.hblocks) {
    // ---- hidden: channels [c0, c0 + 64) of the lower half, pixels of one slab ----
    const int chunk = (int)blockIdx.x / k.hslabs, slab = (int)blockIdx.x - chunk * k.hslabs;
    const int c = chunk * FU_CHUNK + oct * 8;
    float lo = 0.f, hi = 0.f;
    const float* mrow = nullptr;
    if (k.mean) {
      mrow = k.mean + (int64_t)b * HW;
      lo = hi = mrow[0];
      for (int i = tid; i < HW; i += FU_THREADS) {
        const float v = mrow[i];
        lo = fminf(lo, v); hi = fmaxf(hi, v);
      }
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
      }
      if ((tid & 63) == 0) { tot[tid >> 6] = lo; tot[4 + (tid >> 6)] = hi; }
      tsd_jitter();
      __syncthreads();
      lo = fminf(fminf(tot[0], tot[1]), fminf(tot[2], tot[3]));
      hi = fmaxf(fmaxf(tot[4], tot[5]), fmaxf(tot[6], tot[7]));
    }
    if (c >= (k.Ch >> 1)) return;
    const float d = hi - lo;
    const int p_end = min(HW, (slab + 1) * FU_SLAB);
    for (int pix = slab * FU_SLAB + pl; pix < p_end; pix += FU_PL) {
      float f = k.b;
      if (mrow) {
        const float n = d > 0.f ? (mrow[pix] - lo) / d : 0.f;
        f = fmaf(k.b1, n, 1.f);
      }
      half_t* p = k.h + ((int64_t)b * HW + pix) * k.ldh + c;
      const h8 v = *(const h8*)p;
      h8 y;
#pragma unroll
      for (int j = 0; j < 8; j++) y[j] = (half_t)(f * (float)v[j]);
      *(h8*)p = y;
    }
    return;
  }
  // ---- skip: channels [c0, c0 + 64), the whole plane ----
  const int c = ((int)blockIdx.x - k.hblocks) * FU_CHUNK + oct * 8;
  const bool active = c < k.Cr;
  const float* cy = k.tab;
  const float* sy = cy + k.H;
  const float* cx = sy + k.H;
  const float* sx = cx + k.W;
  half_t* base = k.r + (int64_t)b * HW * k.ldr + c;
  float a[FU_SUMS][8];
#pragma unroll
  for (int q = 0; q < FU_SUMS; q++)
#pragma unroll
    for (int j = 0; j < 8; j++) a[q][j] = 0.f;
  if (active) {
    for (int pix = pl; pix < HW; pix += FU_PL) {
      const int y = pix / k.W, x = pix - y * k.W;
      const float vcy = cy[y], vsy = sy[y], vcx = cx[x], vsx = sx[x];
      const float vcxy = fmaf(vcy, vcx, -(vsy * vsx)), vsxy = fmaf(vsy, vcx, vcy * vsx);
      const h8 v = *(const h8*)(base + (int64_t)pix * k.ldr);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float f = (float)v[j];
        a[0][j] += f;
        a[1][j] = fmaf(f, vcy, a[1][j]);
        a[2][j] = fmaf(f, vsy, a[2][j]);
        a[3][j] = fmaf(f, vcx, a[3][j]);
        a[4][j] = fmaf(f, vsx, a[4][j]);
        a[5][j] = fmaf(f, vcxy, a[5][j]);
        a[6][j] = fmaf(f, vsxy, a[6][j]);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < FU_SUMS; q++)
#pragma unroll
    for (int j = 0; j < 8; j++) red[(q * FU_PL + pl) * FU_CHUNK + oct * 8 + j] = a[q][j];
  tsd_jitter();
  __syncthreads();
  // fixed-order reduction over the pixel lanes: one thread per (sum, channel)
  for (int t = tid; t < FU_SUMS * FU_CHUNK; t += FU_THREADS) {
    const int q = t / FU_CHUNK, ch = t - q * FU_CHUNK;
    float s = 0.f;
    for (int l = 0; l < FU_PL; l++) s += red[(q * FU_PL + l) * FU_CHUNK + ch];
    tot[t] = s;
  }
  tsd_jitter();
  __syncthreads();
  if (!active) return;
#pragma unroll
  for (int q = 0; q < FU_SUMS; q++)
#pragma unroll
    for (int j = 0; j < 8; j++) a[q][j] = tot[q * FU_CHUNK + oct * 8 + j];
  for (int pix = pl; pix < HW; pix += FU_PL) {
    const int y = pix / k.W, x = pix - y * k.W;
    const float vcy = cy[y], vsy = sy[y], vcx = cx[x], vsx = sx[x];
    const float vcxy = fmaf(vcy, vcx, -(vsy * vsx)), vsxy = fmaf(vsy, vcx, vcy * vsx);
    half_t* p = base + (int64_t)pix * k.ldr;
    const h8 v = *(const h8*)p;
    h8 o;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float P = a[0][j];
      P = fmaf(a[1][j], vcy, P);
      P = fmaf(a[2][j], vsy, P);
      P = fmaf(a[3][j], vcx, P);
      P = fmaf(a[4][j], vsx, P);
      P = fmaf(a[5][j], vcxy, P);
      P = fmaf(a[6][j], vsxy, P);
      o[j] = (half_t)fmaf(k.g, P, (float)v[j]);
    }
    *(h8*)p = o;
  }
}

// cy[H] sy[H] cx[W] sx[W] of one plane size: built in double, rounded once to fp32, kept on the context (released with it)
int freeu_tab(tsd_ctx* ctx, int H, int W, const float** out) {
  if (H < 2 || W < 2 || H > 4096 || W > 4096) TSD_FAIL(TSD_E_SHAPE, "freeu: plane %d x %d (sides 2 .. 4096)", H, W);
  for (const FreeuTab& t : ctx->freeu_tabs)
    if (t.H == H && t.W == W) { *out = t.dev; return TSD_OK; }
  std::vector<float> host((size_t)2 * (H + W));
  const double tau = 6.283185307179586476925286766559;
  for (int y = 0; y < H; y++) { host[y] = (float)cos(tau * y / H); host[H + y] = (float)sin(tau * y / H); }
  for (int x = 0; x < W; x++) { host[2 * H + x] = (float)cos(tau * x / W); host[2 * H + W + x] = (float)sin(tau * x / W); }
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->freeu_tabs.size() >= 32) {  // a bounded cache: the oldest table goes once nothing in flight can read it
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (void)dev_free(ctx->freeu_tabs.front().dev);
    ctx->freeu_tabs.erase(ctx->freeu_tabs.begin());
  }
  FreeuTab t;
  t.H = H; t.W = W;
  HIP_TRY(dev_malloc((void**)&t.dev, host.size() * sizeof(float)));
  hipError_t e = hipMemcpyAsync(t.dev, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `host` goes out of scope
  if (e != hipSuccess) { (void)dev_free(t.dev); TSD_FAIL(TSD_E_HIP, "freeu: table upload failed: %s", hipGetErrorString(e)); }
  ctx->freeu_tabs.push_back(t);
  *out = t.dev;
  return TSD_OK;
}

int launch_freeu(tsd_ctx* ctx, const FreeuOp& op) {
  const int H = op.H, W = op.W, B = op.B;
  if (B <= 0 || B > 65535 || H < 2 || W < 2 || H > 4096 || W > 4096 || (int64_t)H * W > (1 << 22))
    TSD_FAIL(TSD_E_SHAPE, "freeu: B=%d plane %d x %d", B, H, W);
  if (op.mode != TSD_FREEU_CONSTANT && op.mode != TSD_FREEU_MODULATED) TSD_FAIL(TSD_E_ARG, "freeu: mode %d (0 constant, 1 modulated)", op.mode);
  if (!isfinite(op.b) || !isfinite(op.s)) TSD_FAIL(TSD_E_ARG, "freeu: b = %g, s = %g must be finite", (double)op.b, (double)op.s);
  const bool do_h = op.b != 1.f, do_r = op.s != 1.f;
  if (!do_h && !do_r) return TSD_OK;
  if (do_h) {
    if (!op.h) TSD_FAIL(TSD_E_ARG, "freeu: no hidden tensor");
    if (op.Ch <= 0 || op.Ch % 16 || op.ldh < op.Ch || op.ldh % 8) TSD_FAIL(TSD_E_SHAPE, "freeu: hidden Ch=%d (a multiple of 16) pitch %d", op.Ch, op.ldh);
    if (ctx->launch() && ((uintptr_t)op.h & 15)) TSD_FAIL(TSD_E_ARG, "freeu: the hidden tensor is not 16-byte aligned");
    if (op.mode == TSD_FREEU_MODULATED && !op.mean) TSD_FAIL(TSD_E_ARG, "freeu: the modulated mode needs the [B][HW] buffer of means");
  }
  if (do_r) {
    if (!op.r) TSD_FAIL(TSD_E_ARG, "freeu: no skip tensor");
    if (op.Cr <= 0 || op.Cr % 8 || op.ldr < op.Cr || op.ldr % 8) TSD_FAIL(TSD_E_SHAPE, "freeu: skip Cr=%d (a multiple of 8) pitch %d", op.Cr, op.ldr);
    if (ctx->launch() && ((uintptr_t)op.r & 15)) TSD_FAIL(TSD_E_ARG, "freeu: the skip tensor is not 16-byte aligned");
  }
  // the table of a new plane size is built here, in the planning pass too: a session that sized its workspace with FreeU on allocates
  // nothing in its steps
  const float* tab = nullptr;
  if (do_r) TSD_TRY(freeu_tab(ctx, H, W, &tab));
  if (!ctx->launch()) return TSD_OK;
  const int HW = H * W;
  FreeuK k = {};
  if (do_r) {
    k.tab = tab;
    k.r = op.r; k.ldr = op.ldr; k.Cr = op.Cr;
    k.g = (float)(((double)op.s - 1.0) / (double)HW);
  }
  const bool modulated = do_h && op.mode == TSD_FREEU_MODULATED;
  if (do_h) {
    k.h = op.h; k.ldh = op.ldh; k.Ch = op.Ch; k.b = op.b; k.b1 = op.b - 1.f;
    k.mean = modulated ? op.mean : nullptr;
    k.hslabs = ceil_div(HW, FU_SLAB);
    k.hblocks = ceil_div(op.Ch / 2, FU_CHUNK) * k.hslabs;
  }
  k.H = H; k.W = W;
  const int rblocks = do_r ? ceil_div(op.Cr, FU_CHUNK) : 0;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  if (modulated) {
    prof.kernels = 2;
    hipLaunchKernelGGL(k_freeu_mean, dim3((unsigned)ceil_div(HW, FU_THREADS / 64), (unsigned)B), dim3(FU_THREADS), 0, ctx->stream,
                       (const half_t*)op.h, op.ldh, HW, op.Ch, op.mean);
    HIP_TRY(hipGetLastError());
  }
  hipLaunchKernelGGL(k_freeu, dim3((unsigned)(k.hblocks + rblocks), (unsigned)B), dim3(FU_THREADS), 0, ctx->stream, k);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
