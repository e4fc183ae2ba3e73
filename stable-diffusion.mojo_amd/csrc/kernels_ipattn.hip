// kernels_ipattn.hip - IP-Adapter's decoupled cross attention (Ye et al. 2023, "IP-Adapter: Text Compatible Image Prompt Adapter for
// Text-to-Image Diffusion Models"): in every cross-attention block a second key / value pair reads N <= 16 image tokens and its attention
// result is added to the text result before the shared output projection.  ONE launch per block, between the cross-attention flash call
// and `ca_out`, on the block's live q and ao:
//     O <- rn16( f32(O) + s_b * ( sum_j p_j V_ip[j] ) / sum_j p_j ),   p_j = rn16( exp( scale * (q . K_ip[j]) - max_j ) ),  j < N
// fp32 products and sums on the matrix unit, the TRUE row maximum (all N scores of a row are in registers: no optimistic pass), keys
// j >= N masked to p = 0, the denominator the sum of the ROUNDED p_j, one division, one fma with s_b, one rounding to fp16.
//
// A wave owns 16 queries of one (sample, head); a workgroup is four such waves on consecutive query tiles; grid (ceil(S / 64), H, B).  A
// tile never crosses a sample boundary (S need not be a multiple of 16: rows >= S load zeros and store nothing).  No LDS, no barrier, no
// atomics; a sample's bits depend on its own q, K_ip, V_ip^T, O and s_b only - the same in every batch position and at every B.
//
// Register layout (v_mfma_f32_16x16x16_f16: A[row l&15][k 4(l>>4)+j], B[k 4(l>>4)+j][col l&15], D[row 4(l>>4)+r][col l&15]); i = l & 15,
// g = l >> 4:
//   S^T = K_ip . Q^T   A = keys (row i), B = queries (col i).  The head's dims are walked in 32-wide pairs of k steps: lane (i, g) holds
//                      dims 32m + 8g + [0, 8) of key i and of query i - ONE 16-byte load each - and feeds the low / high half to the two
//                      steps of pair m.  Both operands use the same permutation of the dims, so the dot product is the plain one; dims >= d
//                      of the last pair (d = 40: 40 .. 63, d = 80: 80 .. 95) are exact zeros.
//   The accumulator holds score[key 4g + r][query i], r = 0 .. 3: already the B-operand layout of the second product.  Maximum and sum
//   are an in-lane step over r and two cross-lane steps over the four 16-lane groups (the same bits in all four lanes of a query).
//   O^T = V_ip^T . P^T A = channels (row i), B = p.  V_ip^T [C][ldvt] gives a lane its 4 keys 4g .. 4g + 3 of a channel in one 8-byte load.
//                      Channel tiles come in pairs as well: row i of tile t of pair m is channel 32m + 8(i >> 2) + 4t + (i & 3), so result
//                      row 4g + r of tile t is channel 32m + 8g + 4t + r and the lane ends with the 8 ADJACENT channels 32m + 8g + [0, 8)
//                      of its query: one 16-byte load and one 16-byte store of O.
// Keys >= N are never loaded from K_ip and are replaced by zeros in the V_ip^T fragment: whatever rows N .. 15 of the two operands hold
// (they must exist: ldvt >= 16) changes no bit.  A sample whose scale is exactly 0 is neither read nor written: its workgroups return
// before their first load.
// Traffic: q once, O once in and once out = 3 M C 2 bytes; K_ip / V_ip^T are 2 x 16 x C fp16 per sample and stay in cache.
#include "common.h"
#include "lds_dma.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int IPA_WAVES = 4;

struct IpAttnK {
  const half_t* Q; const half_t* K; const half_t* Vt; half_t* O; const float* s;
  long long sQ, sK, sVt, sO;
  int ldq, ldk, ldvt, ldo;
  int S, N;
  float scale;
};

template <int D>
__global__ void __launch_bounds__(64 * IPA_WAVES) k_ip_attn_add(IpAttnK a) {
  constexpr int NP = (D + 31) / 32;  // 32-wide pairs of k steps / of channel tiles: 2 (d = 40), 3 (80), 5 (160)
  const int b = blockIdx.z, h = blockIdx.y;
  const float sb = a.s[b];
  if (sb == 0.f) return;
  const int lane = threadIdx.x & 63;
  const int q0 = ((int)blockIdx.x * IPA_WAVES + ((int)threadIdx.x >> 6)) * 16;
  if (q0 >= a.S) return;  // wave-uniform; the kernel has no barrier
  const int i = lane & 15, g = lane >> 4;
  const int q = q0 + i;
  const bool q_ok = q < a.S, k_ok = i < a.N;
  const half_t* qp = a.Q + (long long)b * a.sQ + (long long)q * a.ldq + h * D + 8 * g;
  const half_t* kp = a.K + (long long)b * a.sK + (long long)i * a.ldk + h * D + 8 * g;
  half_t* op = a.O + (long long)b * a.sO + (long long)q * a.ldo + h * D + 8 * g;
  const half_t* vp = a.Vt + (long long)b * a.sVt + ((long long)h * D + 8 * (i >> 2) + (i & 3)) * a.ldvt + 4 * g;
  h8 qf[NP], kf[NP], of[NP];
#pragma unroll
  for (int m = 0; m < NP; m++) {
    const bool c_ok = 32 * m + 8 * g < D;  // D is a multiple of 8: a lane's 8 dims are all inside the head or all outside
    qf[m] = (q_ok && c_ok) ? *(const h8*)(qp + 32 * m) : (h8)(half_t)0;
    kf[m] = (k_ok && c_ok) ? *(const h8*)(kp + 32 * m) : (h8)(half_t)0;
    of[m] = (q_ok && c_ok) ? *(const h8*)(op + 32 * m) : (h8)(half_t)0;
  }
  f4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int m = 0; m < NP; m++) {
    tsd_jitter();
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(kf[m].lo, qf[m].lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(kf[m].hi, qf[m].hi, acc, 0, 0, 0);
  }
  // exact softmax over the N keys of every query: acc[r] = score[key 4g + r][query i]
  float sc[4];
  float mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    sc[r] = 4 * g + r < a.N ? acc[r] * a.scale : -INFINITY;
    mx = fmaxf(mx, sc[r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  h4 p;
  float pf[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    p[r] = 4 * g + r < a.N ? (half_t)expf(sc[r] - mx) : (half_t)0;
    pf[r] = (float)p[r];
  }
  float den = (pf[0] + pf[1]) + (pf[2] + pf[3]);
  den += __shfl_xor(den, 16);
  den += __shfl_xor(den, 32);
#pragma unroll
  for (int m = 0; m < NP; m++) {
    tsd_jitter();
    f4 o2[2];
#pragma unroll
    for (int t = 0; t < 2; t++) {
      const int c = 32 * m + 8 * (i >> 2) + 4 * t + (i & 3);  // the channel of A row i in tile t of pair m
      h4 v = (h4)(half_t)0;
      if (c < D) v = *(const h4*)(vp + (long long)(32 * m + 4 * t) * a.ldvt);
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (4 * g + j >= a.N) v[j] = (half_t)0;
      const f4 z = {0.f, 0.f, 0.f, 0.f};
      o2[t] = __builtin_amdgcn_mfma_f32_16x16x16f16(v, p, z, 0, 0, 0);
    }
    if (q_ok && 32 * m + 8 * g < D) {
      h8 y;
#pragma unroll
      for (int j = 0; j < 8; j++) y[j] = (half_t)fmaf(sb, o2[j >> 2][j & 3] / den, (float)of[m][j]);
      *(h8*)(op + 32 * m) = y;
    }
  }
}

template <int D>
static int launch_ipa(tsd_ctx* ctx, const IpAttnK& k, int B, int H) {
  const dim3 grid((unsigned)ceil_div(ceil_div(k.S, 16), IPA_WAVES), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL(k_ip_attn_add<D>, grid, dim3(64 * IPA_WAVES), 0, ctx->stream, k);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

// O [B][S][ldo] += s_b * Attn(Q [B][S][ldq], K_ip [B][>= N rows][ldk], V_ip^T [B][H d][ldvt >= 16]) in place; s: device fp32 [B].
// d in {40, 80, 160}, 1 <= N <= 16, S a multiple of 4, pitches and per-sample strides multiples of 8 (16-byte rows), ldvt a multiple of 4.
int launch_ip_attn_add(tsd_ctx* ctx, const IpAttnArgs& a) {
  if (a.d != 40 && a.d != 80 && a.d != 160) TSD_FAIL(TSD_E_SHAPE, "ip attention: head dim %d unsupported (40 / 80 / 160)", a.d);
  if (a.N < 1 || a.N > IP_MAX_TOKENS) TSD_FAIL(TSD_E_SHAPE, "ip attention: %d image tokens (1..%d)", a.N, IP_MAX_TOKENS);
  if (a.B <= 0 || a.B > 65535 || a.H <= 0 || a.H > 65535 || a.S <= 0 || a.S % 4) TSD_FAIL(TSD_E_SHAPE, "ip attention: B=%d H=%d S=%d (S a multiple of 4)", a.B, a.H, a.S);
  const int C = a.H * a.d;
  if (a.ldq < C || a.ldk < C || a.ldo < C || a.ldvt < IP_MAX_TOKENS || a.ldq % 8 || a.ldk % 8 || a.ldo % 8 || a.ldvt % 4 || a.sQ % 8 || a.sK % 8 ||
      a.sO % 8 || a.sVt % 4)
    TSD_FAIL(TSD_E_SHAPE, "ip attention: misaligned or short pitches (q %d k %d o %d for C = %d, v^T %d for 16 keys)", a.ldq, a.ldk, a.ldo, C, a.ldvt);
  if (!a.Q || !a.K || !a.Vt || !a.O || !a.s) TSD_FAIL(TSD_E_ARG, "ip attention: NULL operand");
  if (!ctx->launch()) return TSD_OK;
  if ((((uintptr_t)a.Q | (uintptr_t)a.K | (uintptr_t)a.O) & 15) || ((uintptr_t)a.Vt & 7)) TSD_FAIL(TSD_E_ARG, "ip attention: operands are not 16-byte aligned");
  ProfScope prof(ctx, KC_ATTN, a.S, a.N, a.d, a.B * a.H);
  IpAttnK k;
  k.Q = a.Q; k.K = a.K; k.Vt = a.Vt; k.O = a.O; k.s = a.s;
  k.sQ = a.sQ; k.sK = a.sK; k.sVt = a.sVt; k.sO = a.sO;
  k.ldq = a.ldq; k.ldk = a.ldk; k.ldvt = a.ldvt; k.ldo = a.ldo;
  k.S = a.S; k.N = a.N; k.scale = a.scale;
  switch (a.d) {
    case 40: return launch_ipa<40>(ctx, k, a.B, a.H);
    case 80: return launch_ipa<80>(ctx, k, a.B, a.H);
    default: return launch_ipa<160>(ctx, k, a.B, a.H);
  }
}

// Debug / bench entry: time `iters` launches on synthetic device data (every sample's scale is 1); S queries, N image tokens.
extern "C" int tsd_debug_ip_attn_bench(tsd_ctx* ctx, int B, int H, int d, int S, int N, int iters, float* ms) {
  if (!ctx || !ms || iters <= 0 || B <= 0 || B > 16 || H <= 0 || d <= 0 || S <= 0) TSD_FAIL(TSD_E_ARG, "ip_attn_bench: bad argument");
  HIP_TRY(hipSetDevice(ctx->device));
  const int C = H * d;
  const int64_t nq = (int64_t)B * S * C, nk = (int64_t)B * IP_MAX_TOKENS * C;
  TSD_TRY(ctx_reserve_arena(ctx, (size_t)(2 * nq + 2 * nk) * 2 + (size_t)std::max(nq, nk) * 4 + 8192));
  ctx->arena.top = 0;
  half_t* Q = arena_alloc<half_t>(ctx, nq);
  half_t* K = arena_alloc<half_t>(ctx, nk);
  half_t* Vt = arena_alloc<half_t>(ctx, nk);
  half_t* O = arena_alloc<half_t>(ctx, nq);
  float* sc = arena_alloc<float>(ctx, 16);
  float* tmp = arena_alloc<float>(ctx, std::max(nq, nk));
  if (!Q || !K || !Vt || !O || !sc || !tmp) TSD_FAIL(TSD_E_ALLOC, "ip_attn_bench: arena");
  TSD_TRY(launch_fill_uniform(ctx, tmp, nq, 1, 11, 2.f));
  TSD_TRY(launch_f32_to_f16_rows(ctx, tmp, 1, (int)nq, Q, (int)nq, 1));
  HIP_TRY(hipMemsetAsync(O, 0, (size_t)nq * 2, ctx->stream));
  TSD_TRY(launch_fill_uniform(ctx, tmp, nk, 1, 12, 2.f));
  TSD_TRY(launch_f32_to_f16_rows(ctx, tmp, 1, (int)nk, K, (int)nk, 1));
  TSD_TRY(launch_fill_uniform(ctx, tmp, nk, 1, 13, 1.f));
  TSD_TRY(launch_f32_to_f16_rows(ctx, tmp, 1, (int)nk, Vt, (int)nk, 1));
  float ones[16];
  for (float& v : ones) v = 1.f;
  HIP_TRY(hipMemcpyAsync(sc, ones, sizeof(ones), hipMemcpyHostToDevice, ctx->stream));
  IpAttnArgs a;
  a.Q = Q; a.ldq = C; a.sQ = (int64_t)S * C; a.K = K; a.ldk = C; a.sK = (int64_t)IP_MAX_TOKENS * C;
  a.Vt = Vt; a.ldvt = IP_MAX_TOKENS; a.sVt = (int64_t)C * IP_MAX_TOKENS; a.O = O; a.ldo = C; a.sO = (int64_t)S * C;
  a.s = sc; a.B = B; a.H = H; a.d = d; a.S = S; a.N = N; a.scale = 1.f / sqrtf((float)d);
  int r = launch_ip_attn_add(ctx, a);
  if (r != TSD_OK) { ctx->arena.top = 0; return r; }
  HIP_TRY(hipEventRecord(ctx->ev0, ctx->stream));
  for (int it = 0; it < iters && r == TSD_OK; it++) r = launch_ip_attn_add(ctx, a);
  HIP_TRY(hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(hipEventSynchronize(ctx->ev1));
  float t = 0.f;
  HIP_TRY(hipEventElapsedTime(&t, ctx->ev0, ctx->ev1));
  *ms = t / iters;
  ctx->arena.top = 0;
  return r;
}
