// kernels_vision.hip - the image front end of the CLIP vision encoder (model kind TSD_MODEL_CLIP_VISION_H): pixels to the A operand of the
// patch-embedding GEMM in ONE launch.  It is the float-valued form of Hugging Face's CLIPImageProcessor:
//   images fp32 [B][3][H][W] on 0 .. 255
//   -> resize, shortest edge to 224 and the other edge to int(224 * long / short): PIL's separable antialiased bicubic, horizontal pass
//      first.  Per axis  scale = n_in / n_out, fs = max(scale, 1), support = 2 fs;  output xx has  center = (xx + 0.5) scale,
//      lo = max(int(center - support + 0.5), 0), hi = min(int(center + support + 0.5), n_in)  and the weights
//      w((x - center + 0.5) / fs), x in [lo, hi), Keys' cubic at a = -0.5, divided by their sum
//   -> centre crop to 224 x 224: top = (RH - 224) / 2, left = (RW - 224) / 2
//   -> normalise (v / 255 - mean_c) / std_c, as ONE fma  v * 1 / (255 std_c) + (-mean_c / std_c)  with the two constants rounded to fp32
//   -> rounded once to fp16 into patch rows [B * 256][ld]: row b * 256 + py * 16 + px, column c * 196 + kh * 14 + kw (the flattening of the
//      HF conv weight [1280][3][14][14]); columns 588 .. ld - 1 are zeros.
// Not reproduced: the rounding to uint8 that PIL applies after resizing an 8-bit image - at most 0.5 / 255 / std = 7.5e-3 after the
// normalisation.  At 224 x 224 every coefficient row is (0, 1, 0, 0): the resize is the identity, exactly.
//
// The host builds the two coefficient tables in double (vision_tab), rounds every weight to fp32 once and keeps them on the context per
// (H, W): the 224 CROPPED outputs of each axis with their first source index, tap count and weights.
//
// One workgroup of 256 threads per (sample, patch); grid (256, B).  The horizontal pass over the R source rows the patch's 14 output rows
// read goes to LDS as fp32 [3][R][14] (R <= ~160 at the 2048 limit: under 32 KB), then 588 vertical sums out of LDS, the fma, one 2-byte
// store per element.  Sums run in tap order with fmaf: fp32, the same order for every sample.  No atomics; a sample's bits depend on its own
// pixels and the tables only - not on B, not on its batch position.
// Error against the exact formula, coefficients rounded to fp32 and fp32 sums (T_h, T_v the two tap counts of an element):
//   |v^ - v| <= 1.01 (T_h + T_v + 2) 2^-24 sum |w_v| |w_h| |x|,  then the fma adds 2 * 2^-24 (|v| / (255 std) + mean / std) and the store the
//   fp16 half-ulp (tests/clipvision_ref.py spells it out).
#include <math.h>

#include <algorithm>

#include "common.h"
#include "lds_dma.h"

struct ImgPatchK {
  const float* img; half_t* out;
  const int* xs; const int* xn; const int* ys; const int* yn;
  const float* wx; const float* wy;
  int H, W, tx, ty, ld;
  float a[3], b[3];  // y = fma(v, a[c], b[c])
};

__global__ void __launch_bounds__(256) k_clip_image_patches(ImgPatchK k) {
  extern __shared__ float hb[];  // [3][R][14]
  const int p = blockIdx.x, b = blockIdx.y;
  const int oy0 = (p >> 4) * CV_PATCH, ox0 = (p & 15) * CV_PATCH;
  // first source indices and ends do not decrease along an axis: the patch's rows are [ys[first], ys[last] + yn[last])
  const int y0 = k.ys[oy0];
  const int R = k.ys[oy0 + CV_PATCH - 1] + k.yn[oy0 + CV_PATCH - 1] - y0;
  const float* img = k.img + (size_t)b * 3 * k.H * k.W;
  for (int i = threadIdx.x; i < 3 * R * CV_PATCH; i += 256) {
    const int j = i % CV_PATCH, cr = i / CV_PATCH, r = cr % R, c = cr / R;
    const int ox = ox0 + j, n = k.xn[ox];
    const float* src = img + ((size_t)c * k.H + (y0 + r)) * k.W + k.xs[ox];
    const float* w = k.wx + ox * k.tx;
    float acc = 0.f;
    for (int t = 0; t < n; t++) acc = fmaf(w[t], src[t], acc);
    hb[i] = acc;
  }
  tsd_jitter();
  __syncthreads();
  half_t* out = k.out + ((size_t)b * CV_PATCHES + p) * k.ld;
  for (int e = threadIdx.x; e < k.ld; e += 256) {
    half_t y = (half_t)0;
    if (e < CV_PATCH_K) {
      const int c = e / (CV_PATCH * CV_PATCH), rem = e % (CV_PATCH * CV_PATCH), kh = rem / CV_PATCH, kw = rem % CV_PATCH;
      const int oy = oy0 + kh, n = k.yn[oy];
      const float* w = k.wy + oy * k.ty;
      const float* col = hb + (c * R + (k.ys[oy] - y0)) * CV_PATCH + kw;
      float acc = 0.f;
      for (int t = 0; t < n; t++) acc = fmaf(w[t], col[t * CV_PATCH], acc);
      y = (half_t)fmaf(acc, k.a[c], k.b[c]);
    }
    out[e] = y;
  }
}

__global__ void __launch_bounds__(256) k_vision_class_rows(const float* cls, const half_t* pos, int C, half_t* x, long long sx) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n < C) x[(long long)blockIdx.y * sx + n] = (half_t)(cls[n] + (float)pos[n]);
}

// ---- the coefficient tables (host, double) ------------------------------------------------------------------------------------------------
namespace {
double keys_cubic(double x) {  // a = -0.5
  const double a = -0.5;
  x = fabs(x);
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}
struct AxisTab {
  int start[CV_SIDE], count[CV_SIDE], taps = 0;
  std::vector<double> w[CV_SIDE];
};
// outputs [off, off + 224) of the resize of n_in samples to n_out
void build_axis(int n_in, int n_out, int off, AxisTab& t) {
  const double scale = (double)n_in / n_out, fs = scale < 1.0 ? 1.0 : scale, support = 2.0 * fs, ss = 1.0 / fs;
  t.taps = 0;
  for (int o = 0; o < CV_SIDE; o++) {
    const double center = (off + o + 0.5) * scale;
    int lo = (int)(center - support + 0.5), hi = (int)(center + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
    t.start[o] = lo; t.count[o] = hi - lo;
    t.w[o].resize((size_t)(hi - lo));
    double ww = 0.0;
    for (int x = lo; x < hi; x++) { t.w[o][x - lo] = keys_cubic((x - center + 0.5) * ss); ww += t.w[o][x - lo]; }
    if (ww != 0.0) for (double& v : t.w[o]) v /= ww;
    t.taps = std::max(t.taps, hi - lo);
  }
}
}  // namespace

int vision_tab(tsd_ctx* ctx, int H, int W, VisionTab* out) {
  if (H < 8 || W < 8 || H > 2048 || W > 2048) TSD_FAIL(TSD_E_SHAPE, "clip image: sides %d x %d outside 8 .. 2048", H, W);
  for (const VisionTab& t : ctx->vision_tabs)
    if (t.H == H && t.W == W) { *out = t; return TSD_OK; }
  const int RH = H <= W ? CV_SIDE : (int)((long long)CV_SIDE * H / W), RW = H <= W ? (int)((long long)CV_SIDE * W / H) : CV_SIDE;
  AxisTab ax, ay;
  build_axis(W, RW, (RW - CV_SIDE) / 2, ax);
  build_axis(H, RH, (RH - CV_SIDE) / 2, ay);
  VisionTab t;
  t.H = H; t.W = W; t.tx = ax.taps; t.ty = ay.taps;
  for (int o = 0; o < CV_SIDE; o++) {  // what the kernel relies on: every tap inside the image, starts and ends in order
    if (ax.count[o] < 1 || ay.count[o] < 1 || ax.start[o] < 0 || ay.start[o] < 0 || ax.start[o] + ax.count[o] > W || ay.start[o] + ay.count[o] > H ||
        (o && (ax.start[o] < ax.start[o - 1] || ay.start[o] < ay.start[o - 1] || ay.start[o] + ay.count[o] < ay.start[o - 1] + ay.count[o - 1])))
      TSD_FAIL(TSD_E_STATE, "clip image: coefficient table of %d x %d is not monotone / inside the image at output %d", H, W, o);
  }
  for (int py = 0; py < CV_GRID; py++)
    t.rows = std::max(t.rows, ay.start[py * CV_PATCH + CV_PATCH - 1] + ay.count[py * CV_PATCH + CV_PATCH - 1] - ay.start[py * CV_PATCH]);
  if ((size_t)3 * t.rows * CV_PATCH * sizeof(float) > 48 * 1024) TSD_FAIL(TSD_E_SHAPE, "clip image: %d source rows per patch do not fit the LDS", t.rows);
  const size_t ni = 4 * CV_SIDE, nf = (size_t)CV_SIDE * (t.tx + t.ty);
  std::vector<char> host(ni * 4 + nf * 4, 0);
  int* hi = (int*)host.data();
  float* hw = (float*)(host.data() + ni * 4);
  for (int o = 0; o < CV_SIDE; o++) {
    hi[o] = ax.start[o]; hi[CV_SIDE + o] = ax.count[o]; hi[2 * CV_SIDE + o] = ay.start[o]; hi[3 * CV_SIDE + o] = ay.count[o];
    for (int j = 0; j < ax.count[o]; j++) hw[(size_t)o * t.tx + j] = (float)ax.w[o][j];
    for (int j = 0; j < ay.count[o]; j++) hw[(size_t)CV_SIDE * t.tx + (size_t)o * t.ty + j] = (float)ay.w[o][j];
  }
  HIP_TRY(hipSetDevice(ctx->device));
  if (ctx->vision_tabs.size() >= 32) {  // a bounded cache: the oldest table goes once nothing in flight can read it
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    (void)dev_free(ctx->vision_tabs.front().dev);
    ctx->vision_tabs.erase(ctx->vision_tabs.begin());
  }
  HIP_TRY(dev_malloc(&t.dev, host.size()));
  hipError_t e = hipMemcpyAsync(t.dev, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // `host` goes out of scope
  if (e != hipSuccess) { (void)dev_free(t.dev); TSD_FAIL(TSD_E_HIP, "clip image: table upload failed: %s", hipGetErrorString(e)); }
  ctx->vision_tabs.push_back(t);
  *out = t;
  return TSD_OK;
}

int launch_clip_image_patches(tsd_ctx* ctx, const float* img, int B, int H, int W, half_t* out, int ld) {
  if (B <= 0 || B > 65535) TSD_FAIL(TSD_E_SHAPE, "clip image: B=%d", B);
  if (ld < CV_PATCH_LD || ld % 8 || ld > 4096) TSD_FAIL(TSD_E_SHAPE, "clip image: patch row pitch %d (>= %d, a multiple of 8)", ld, CV_PATCH_LD);
  if (!img || !out) TSD_FAIL(TSD_E_ARG, "clip image: NULL operand");
  VisionTab t;
  TSD_TRY(vision_tab(ctx, H, W, &t));
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  ImgPatchK k;
  k.img = img; k.out = out;
  k.xs = (const int*)t.dev; k.xn = k.xs + CV_SIDE; k.ys = k.xs + 2 * CV_SIDE; k.yn = k.xs + 3 * CV_SIDE;
  k.wx = (const float*)(k.xs + 4 * CV_SIDE); k.wy = k.wx + (size_t)CV_SIDE * t.tx;
  k.H = H; k.W = W; k.tx = t.tx; k.ty = t.ty; k.ld = ld;
  const double mean[3] = {0.48145466, 0.4578275, 0.40821073}, sd[3] = {0.26862954, 0.26130258, 0.27577711};
  for (int c = 0; c < 3; c++) { k.a[c] = (float)(1.0 / (255.0 * sd[c])); k.b[c] = (float)(-mean[c] / sd[c]); }
  const size_t lds = (size_t)3 * t.rows * CV_PATCH * sizeof(float);
  hipLaunchKernelGGL(k_clip_image_patches, dim3(CV_PATCHES, (unsigned)B), dim3(256), lds, ctx->stream, k);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

int launch_vision_class_rows(tsd_ctx* ctx, const float* cls, const half_t* pos, int B, int C, half_t* x, int64_t sx) {
  if (B <= 0 || B > 65535 || C <= 0) TSD_FAIL(TSD_E_SHAPE, "vision class rows: B=%d C=%d", B, C);
  if (!ctx->launch()) return TSD_OK;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_vision_class_rows, dim3((unsigned)ceil_div(C, 256), (unsigned)B), dim3(256), 0, ctx->stream, cls, pos, C, x, (long long)sx);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
