// kernels_tome.hip - token merging for self attention (Bolya & Hoffman 2023, "Token Merging for Stable Diffusion"; tomesd's
// bipartite_soft_matching_random2d with sx = sy = 2, merge_attn only).  include/tsd.h "Token merging" states the semantics; in short, per
// sample over an H x W token grid (N = H W, Nd = N / 4 destinations - one per 2 x 2 cell -, Ns = 3 N / 4 sources):
//     score(i, j) = a_i . b_j / (|a_i| |b_j|)    node_idx[i] = argmax_j (smallest j on ties)    node_max[i] = that score
//     the r sources of largest node_max (smaller index first on ties) join their destination's row; a merged row is the mean of its members
// Four kernels, no scratch memory, no global atomics, no host round trip:
//
//   k_tome_match    grid (ceil(Ns / 128), B), 4 waves.  A workgroup owns 128 source rows and walks the sample's destination rows in 64-row
//                   tiles, 64 channels at a time, through double-buffered LDS (row pitch 72 halves: conflict-free 16-byte fragment reads).
//                   Both operands are gathered by cell arithmetic.  The product is taken swapped, S^T = B A^T on v_mfma_f32_32x32x16_f16:
//                   A = 32 destination rows from LDS, B = the wave's 32 source rows from registers, so a lane holds 32 scores of ONE source
//                   row per tile and the running maximum / arg-max is in-lane, with one lane ^ 32 exchange at the very end.  The four
//                   threads that stage a destination row square what they stage; |b_j|^-1 reaches the consumers through LDS with the tile
//                   and scales the accumulator rows, |a_i|^-1 (from the B fragments themselves) scales the winner once.  At C = 320 the
//                   source fragments (80 registers) stay resident for the whole walk (<1>); wider rows re-read them per 64-channel step (<0>).
//   k_tome_select   grid (B), 16 waves, the sample's Ns <= 24576 scores in LDS as order-preserving uint32.  A 4 x 8-bit radix select
//                   (LDS integer counters: a histogram does not depend on arrival order) finds the r-th largest key; a block scan in source
//                   order settles which of the keys EQUAL to it merge, a second one gives the unmerged sources their rows.  Members of a
//                   destination's row are collected in any order in LDS (the key array is dead by then) and placed by RANK - the number of
//                   smaller tokens in the segment - so what is written does not depend on the order: row_of, start, members are the same
//                   bits on every run.
//   k_tome_merge    rows of [B S'][C] through the member lists: 16-byte loads, fp32 sums in list order, one division, one rounding; a
//                   single-member row is a copy.
//   k_tome_unmerge  out[t] = y[row_of[t]], 16 bytes per thread.
// Every table index a kernel reads is clamped to its range before it addresses memory.
#include <math.h>

#include <algorithm>
#include <atomic>

#include "common.h"
#include "lds_dma.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f16v __attribute__((ext_vector_type(16)));

struct TomeGrid {
  int W, cw;        // token grid width, cells per row (W / 2)
  int N, Nd, Ns;
  uint32_t seed;
};

// the hash of include/tsd.h (murmur3's 32-bit finaliser over seed ^ cell * golden ratio)
__host__ __device__ static inline uint32_t tome_hash(uint32_t seed, uint32_t cell) {
  uint32_t x = seed ^ (cell * 0x9E3779B9u);
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}
__device__ __forceinline__ int tome_dst_pos(const TomeGrid& g, int c) { return g.seed ? (int)(tome_hash(g.seed, (uint32_t)c) & 3u) : 0; }
__device__ __forceinline__ int tome_cell_token(const TomeGrid& g, int c, int q) {
  const int cy = c / g.cw, cx = c - cy * g.cw;
  return (2 * cy + (q >> 1)) * g.W + 2 * cx + (q & 1);
}
__device__ __forceinline__ int tome_dst_token(const TomeGrid& g, int c) { return tome_cell_token(g, c, tome_dst_pos(g, c)); }
__device__ __forceinline__ int tome_src_token(const TomeGrid& g, int i) {
  const int c = i / 3, k = i - 3 * c;
  return tome_cell_token(g, c, k + (k >= tome_dst_pos(g, c) ? 1 : 0));
}

// ------------------------------------------------------------------------------------------------------------------- match
constexpr int TM_THREADS = 256;
constexpr int TM_SRC = 128;            // source rows per workgroup: 32 per wave
constexpr int TM_DT = 64;              // destination rows per tile
constexpr int TM_KB = 64;              // channels per step
constexpr int TM_PITCH = TM_KB + 8;    // LDS row pitch in halves (144 bytes)
constexpr int TM_HOLD_KB = 5;          // C = 320: the source fragments of all five steps stay in registers

struct TomeMatchK {
  const half_t* x;   // [B][N][ldx]
  int64_t sx;
  int ldx, C;
  TomeGrid g;
  float* node_max;   // [B][Ns]
  int* node_idx;     // [B][Ns]
};

__device__ __forceinline__ float tome_sumsq(const h8& v, float s) {
#pragma unroll
  for (int e = 0; e < 8; e++) s = fmaf((float)v[e], (float)v[e], s);
  return s;
}

template <int HOLD>
__global__ void __launch_bounds__(TM_THREADS) k_tome_match(TomeMatchK k) {
  __shared__ __attribute__((aligned(16))) half_t tile[2][TM_DT * TM_PITCH];
  __shared__ float dinv[2][TM_DT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, hi = lane >> 5;
  const TomeGrid g = k.g;
  const half_t* xb = k.x + (int64_t)blockIdx.y * k.sx;
  const int nkb = k.C / TM_KB, ntile = (g.Nd + TM_DT - 1) / TM_DT, nstep = ntile * nkb;

  // consumer role: this lane's source row is column l31 of the wave's score blocks
  const int si = blockIdx.x * TM_SRC + wave * 32 + l31;
  const half_t* srow = xb + (int64_t)tome_src_token(g, si < g.Ns ? si : g.Ns - 1) * k.ldx + 8 * hi;
  // loader role: destination row lr of the tile, halves [16 lp, 16 lp + 16) of the step's 64 channels
  const int lr = tid >> 2, lp = tid & 3;

  h8 sf[HOLD ? TM_HOLD_KB : 1][4];
  float ass = 0.f;   // this lane's half of |a_i|^2
  if (HOLD) {
#pragma unroll
    for (int kb = 0; kb < TM_HOLD_KB; kb++)
#pragma unroll
      for (int ks = 0; ks < 4; ks++) {
        sf[kb][ks] = *(const h8*)(srow + kb * TM_KB + ks * 16);
        ass = tome_sumsq(sf[kb][ks], ass);
      }
  }

  h8 pd[2];          // the staged 16 halves of the NEXT step's destination row
  h8 ps[4];          // <0>: the source fragments of the next step
  float dss = 0.f;   // running |b_j|^2 of the row being staged (this thread's quarter)
  const half_t* drow = nullptr;
  auto fetch = [&](int s) {   // global -> registers for step s
    const int t = s / nkb, kb = s - t * nkb;
    if (kb == 0) {
      const int j = t * TM_DT + lr;
      drow = j < g.Nd ? xb + (int64_t)tome_dst_token(g, j) * k.ldx + 16 * lp : nullptr;
      dss = 0.f;
    }
    if (drow) {
      pd[0] = *(const h8*)(drow + kb * TM_KB);
      pd[1] = *(const h8*)(drow + kb * TM_KB + 8);
    } else {
      pd[0] = h8{0, 0, 0, 0, 0, 0, 0, 0};
      pd[1] = pd[0];
    }
    if (!HOLD) {
#pragma unroll
      for (int ks = 0; ks < 4; ks++) ps[ks] = *(const h8*)(srow + kb * TM_KB + ks * 16);
    }
  };
  auto stage = [&](int s) {   // registers -> LDS buffer s & 1; the last step of a tile publishes the row's inverse norm with it
    const int t = s / nkb, kb = s - t * nkb;
    half_t* dst = &tile[s & 1][lr * TM_PITCH + 16 * lp];
    *(h8*)dst = pd[0];
    *(h8*)(dst + 8) = pd[1];
    dss = tome_sumsq(pd[1], tome_sumsq(pd[0], dss));
    if (kb == nkb - 1) {
      float ss = dss + __shfl_xor(dss, 1);
      ss += __shfl_xor(ss, 2);
      if (lp == 0) dinv[t & 1][lr] = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
    }
  };

  float best = -INFINITY;
  int bj = 0x7fffffff;
  f16v acc[2];
  h8 cur[4];

  fetch(0);
  stage(0);
  if (!HOLD) {
#pragma unroll
    for (int ks = 0; ks < 4; ks++) cur[ks] = ps[ks];
  }
  tsd_jitter();
  __syncthreads();

  auto mma = [&](int buf, const h8 (&bf)[4]) {
#pragma unroll
    for (int ks = 0; ks < 4; ks++)
#pragma unroll
      for (int blk = 0; blk < 2; blk++) {
        const h8 af = *(const h8*)&tile[buf][(blk * 32 + l31) * TM_PITCH + ks * 16 + 8 * hi];
        acc[blk] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf[ks], acc[blk], 0, 0, 0);
      }
  };
  auto finish_tile = [&](int t) {   // scale the 32 scores by |b_j|^-1 and fold them into the running arg-max
#pragma unroll
    for (int blk = 0; blk < 2; blk++)
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const int row = blk * 32 + (i >> 2) * 8 + hi * 4 + (i & 3), j = t * TM_DT + row;
        const float v = acc[blk][i] * dinv[t & 1][row];
        if (j < g.Nd && (v > best || (v == best && j < bj))) { best = v; bj = j; }
      }
  };

  for (int t = 0; t < ntile; t++) {
#pragma unroll
    for (int blk = 0; blk < 2; blk++)
#pragma unroll
      for (int i = 0; i < 16; i++) acc[blk][i] = 0.f;
    if (HOLD) {
#pragma unroll
      for (int kb = 0; kb < TM_HOLD_KB; kb++) {
        const int s = t * TM_HOLD_KB + kb;
        if (s + 1 < nstep) fetch(s + 1);
        mma(s & 1, sf[kb]);
        if (kb == TM_HOLD_KB - 1) finish_tile(t);
        if (s + 1 < nstep) stage(s + 1);
        tsd_jitter();
        __syncthreads();
      }
    } else {
      for (int kb = 0; kb < nkb; kb++) {
        const int s = t * nkb + kb;
        if (s + 1 < nstep) fetch(s + 1);
        if (t == 0) {
#pragma unroll
          for (int ks = 0; ks < 4; ks++) ass = tome_sumsq(cur[ks], ass);
        }
        mma(s & 1, cur);
        if (kb == nkb - 1) finish_tile(t);
        if (s + 1 < nstep) {
          stage(s + 1);
#pragma unroll
          for (int ks = 0; ks < 4; ks++) cur[ks] = ps[ks];
        }
        tsd_jitter();
        __syncthreads();
      }
    }
  }

  // the other half of the column (destination rows hi ^ 1) and of |a_i|^2 live in lane ^ 32
  const float ob = __shfl_xor(best, 32);
  const int oj = __shfl_xor(bj, 32);
  ass += __shfl_xor(ass, 32);
  if (ob > best || (ob == best && oj < bj)) { best = ob; bj = oj; }
  if (hi == 0 && si < g.Ns) {
    const float ainv = ass > 0.f ? 1.f / sqrtf(ass) : 0.f;
    const bool ok = bj >= 0 && bj < g.Nd;   // (a row of NaNs wins nothing)
    k.node_max[(int64_t)blockIdx.y * g.Ns + si] = ok ? best * ainv : 0.f;
    k.node_idx[(int64_t)blockIdx.y * g.Ns + si] = ok ? bj : 0;
  }
}

// ------------------------------------------------------------------------------------------------------------------ select
constexpr int TS_THREADS = 1024;
constexpr int TS_WAVES = TS_THREADS / 64;
constexpr int TS_MAX_PER = TOME_MAX_TOKENS * 3 / 4 / TS_THREADS;   // 24 sources per thread: their merged flags are one 32-bit mask

struct TomeSelectK {
  const float* node_max;  // [B][Ns]
  const int* node_idx;    // [B][Ns]
  TomeGrid g;
  int r;
  int* row_of;            // [B][N]
  int* start;             // [B][N - r + 1]
  int* members;           // [B][N]
};

// Exclusive scan of one int per thread in thread order; *total = the sum.  ws: TS_WAVES ints of LDS.  Ends with a barrier.
__device__ __forceinline__ int tome_block_scan(int v, int* ws, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  if (lane == 63) ws[wave] = inc;
  tsd_jitter();
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < TS_WAVES; w++) {
    const int s = ws[w];
    if (w < wave) base += s;
    tot += s;
  }
  *total = tot;
  tsd_jitter();
  __syncthreads();
  return base + inc - v;
}

__device__ __forceinline__ uint32_t tome_key(float f) {   // larger float <=> larger key (-0 below +0: both are score 0 of a zero row)
  uint32_t u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(TS_THREADS) k_tome_select(TomeSelectK k) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ts_smem[];
  const TomeGrid g = k.g;
  uint32_t* keys = ts_smem;                 // [Ns]; once the flags are settled: stage[r], (destination << 15 | token) of merged sources
  int* cnt = (int*)(ts_smem + g.Ns);        // [Nd]: sources merged into a destination, then the segment cursors
  int* hist = cnt + g.Nd;                   // [256]
  int* ws = hist + 256;                     // [TS_WAVES]
  int* sel = ws + TS_WAVES;                 // [2]
  const int tid = threadIdx.x, b = blockIdx.x, r = k.r, keep = g.Ns - r;
  const float* nmax = k.node_max + (int64_t)b * g.Ns;
  const int* nidx = k.node_idx + (int64_t)b * g.Ns;
  int* row_of = k.row_of + (int64_t)b * g.N;
  int* start = k.start + (int64_t)b * (g.N - r + 1);
  int* members = k.members + (int64_t)b * g.N;

  for (int i = tid; i < g.Ns; i += TS_THREADS) keys[i] = tome_key(nmax[i]);
  for (int c = tid; c < g.Nd; c += TS_THREADS) cnt[c] = 0;
  tsd_jitter();
  __syncthreads();

  // ---- the r-th largest key: 8 bits per pass from the top; `want` counts down to the place inside the keys that share the prefix
  uint32_t prefix = 0, mask = 0;
  int want = r;
  for (int shift = 24; shift >= 0 && r > 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    tsd_jitter();
    __syncthreads();
    for (int i = tid; i < g.Ns; i += TS_THREADS) {
      const uint32_t key = keys[i];
      if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1);
    }
    tsd_jitter();
    __syncthreads();
    const int v = tid < 256 ? hist[255 - tid] : 0;   // thread t looks at digit 255 - t: the scan counts the keys with a LARGER digit
    int total;
    const int above = tome_block_scan(v, ws, &total);
    if (tid < 256 && above < want && want <= above + v) { sel[0] = 255 - tid; sel[1] = above; }
    tsd_jitter();
    __syncthreads();
    prefix |= (uint32_t)sel[0] << shift;
    mask |= 255u << shift;
    want -= sel[1];
    __syncthreads();
  }
  // now: keys > prefix merge, and the first `want` keys == prefix in source order (r == 0: none)

  // ---- flags and rows, in source order: thread t owns sources [t per, t per + per)
  const int per = (g.Ns + TS_THREADS - 1) / TS_THREADS, i0 = tid * per, i1 = min(i0 + per, g.Ns);
  int neq = 0;
  for (int i = i0; i < i1; i++) neq += keys[i] == prefix;
  int total;
  int eq_rank = tome_block_scan(neq, ws, &total);
  uint32_t mmask = 0;
  int nun = 0;
  for (int i = i0; i < i1; i++) {
    const uint32_t key = keys[i];
    bool m = false;
    if (r > 0) {
      if (key > prefix) m = true;
      else if (key == prefix) m = eq_rank++ < want;
    }
    if (m) mmask |= 1u << (i - i0);
    else nun++;
  }
  int row = tome_block_scan(nun, ws, &total);
  for (int i = i0; i < i1; i++) {
    const int tok = tome_src_token(g, i);
    if ((mmask >> (i - i0)) & 1u) {
      const int c = min(max(nidx[i], 0), g.Nd - 1);
      row_of[tok] = keep + c;
      atomicAdd(&cnt[c], 1);
    } else if (row < keep) {   // (always, when the counts add up)
      row_of[tok] = row;
      start[row] = row;
      members[row] = tok;
      row++;
    }
  }
  tsd_jitter();
  __syncthreads();

  // ---- destination rows: row keep + c starts at keep + c + (sources merged into destinations < c)
  const int perd = (g.Nd + TS_THREADS - 1) / TS_THREADS, c0 = min(tid * perd, g.Nd), c1 = min(c0 + perd, g.Nd);
  int nloc = 0;
  for (int c = c0; c < c1; c++) nloc += cnt[c];
  int off = tome_block_scan(nloc, ws, &total);
  for (int c = c0; c < c1; c++) {
    const int n = cnt[c];
    cnt[c] = off;          // the cursor of segment c in stage[]; after the fill below it is the segment's end
    start[keep + c] = keep + c + off;
    row_of[tome_dst_token(g, c)] = keep + c;
    off += n;
  }
  if (tid == 0) start[keep + g.Nd] = g.N;
  tsd_jitter();
  __syncthreads();   // every key has been read (the flags are in mmask): the array becomes stage[]
  uint32_t* stage = keys;
  for (int i = i0; i < i1; i++)
    if ((mmask >> (i - i0)) & 1u) {
      const int c = min(max(nidx[i], 0), g.Nd - 1);
      const int p = atomicAdd(&cnt[c], 1);
      if (p < r) stage[p] = ((uint32_t)c << 15) | (uint32_t)tome_src_token(g, i);
    }
  tsd_jitter();
  __syncthreads();
  // placement by rank: the position of a member is the number of smaller tokens in its row - whatever order the segment was filled in
  const int nst = min(total, r);
  for (int p = tid; p < nst; p += TS_THREADS) {
    const uint32_t e = stage[p];
    const int c = (int)(e >> 15), tok = (int)(e & 32767u);
    const int s0 = c ? cnt[c - 1] : 0, s1 = min(cnt[c], nst);
    int rank = 0;
    for (int q = s0; q < s1; q++) rank += stage[q] < e;
    const int pos = keep + c + s0 + rank + (tome_dst_token(g, c) < tok ? 1 : 0);
    if (pos < g.N) members[pos] = tok;
  }
  for (int c = tid; c < g.Nd; c += TS_THREADS) {
    const int s0 = c ? cnt[c - 1] : 0, s1 = min(cnt[c], nst), td = tome_dst_token(g, c);
    int rank = 0;
    for (int q = s0; q < s1; q++) rank += (int)(stage[q] & 32767u) < td;
    const int pos = keep + c + s0 + rank;
    if (pos < g.N) members[pos] = td;
  }
}

// --------------------------------------------------------------------------------------------------------- merge / unmerge
constexpr int TG_THREADS = 256;

// y[b][row] = rn16(sum over the row's members of x[b][member] / count), the sum in fp32 in list order; one member: a copy
__global__ void __launch_bounds__(TG_THREADS) k_tome_merge(const half_t* __restrict__ x, int ldx, int N, int C8, int Sm, int tpr, int rpb,
                                                           const int* __restrict__ start, const int* __restrict__ members,
                                                           half_t* __restrict__ y, int ldy) {
  const int rl = threadIdx.x / tpr, cl = threadIdx.x - rl * tpr, b = blockIdx.y;
  const int row = blockIdx.x * rpb + rl;
  if (rl >= rpb || row >= Sm) return;
  const int* st = start + (int64_t)b * (Sm + 1);
  const int* mem = members + (int64_t)b * N;
  const int s0 = min(max(st[row], 0), N - 1), s1 = min(max(st[row + 1], s0 + 1), N);
  const half_t* xb = x + (int64_t)b * N * ldx;
  half_t* yr = y + ((int64_t)b * Sm + row) * ldy;
  for (int c8 = cl; c8 < C8; c8 += tpr) {
    const h8 first = *(const h8*)(xb + (int64_t)min(max(mem[s0], 0), N - 1) * ldx + c8 * 8);
    if (s1 - s0 == 1) { *(h8*)(yr + c8 * 8) = first; continue; }
    float s[8];
#pragma unroll
    for (int e = 0; e < 8; e++) s[e] = (float)first[e];
    for (int q = s0 + 1; q < s1; q++) {
      const h8 v = *(const h8*)(xb + (int64_t)min(max(mem[q], 0), N - 1) * ldx + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; e++) s[e] += (float)v[e];
    }
    const float cntf = (float)(s1 - s0);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = (_Float16)(s[e] / cntf);
    *(h8*)(yr + c8 * 8) = o;
  }
}

// out[b][t] = y[b][row_of[b][t]]
__global__ void __launch_bounds__(TG_THREADS) k_tome_unmerge(const half_t* __restrict__ y, int ldy, int N, int C8, int Sm, int tpr, int rpb,
                                                             const int* __restrict__ row_of, half_t* __restrict__ out, int ldo) {
  const int rl = threadIdx.x / tpr, cl = threadIdx.x - rl * tpr, b = blockIdx.y;
  const int t = blockIdx.x * rpb + rl;
  if (rl >= rpb || t >= N) return;
  const int row = min(max(row_of[(int64_t)b * N + t], 0), Sm - 1);
  const half_t* yr = y + ((int64_t)b * Sm + row) * ldy;
  half_t* orow = out + ((int64_t)b * N + t) * ldo;
  for (int c8 = cl; c8 < C8; c8 += tpr) *(h8*)(orow + c8 * 8) = *(const h8*)(yr + c8 * 8);
}

// ---------------------------------------------------------------------------------------------------------------- launchers
int tome_r(float ratio, int N) { return 8 * (int)floor((double)ratio * (double)N / 8.0); }

static int tome_grid(const TomeOp& op, TomeGrid* g) {
  if (op.B <= 0 || op.B > 65535) TSD_FAIL(TSD_E_SHAPE, "token merge: B=%d (1..65535)", op.B);
  if (op.H < 2 || op.W < 2 || (op.H | op.W) & 1 || (int64_t)op.H * op.W < 64)
    TSD_FAIL(TSD_E_SHAPE, "token merge: a %d x %d token grid (even sides, at least 64 tokens)", op.H, op.W);
  if ((int64_t)op.H * op.W > TOME_MAX_TOKENS) TSD_FAIL(TSD_E_SHAPE, "token merge: %d x %d tokens, more than %d", op.H, op.W, TOME_MAX_TOKENS);
  g->W = op.W; g->cw = op.W / 2; g->N = op.H * op.W; g->Nd = g->N / 4; g->Ns = g->N - g->Nd; g->seed = op.seed;
  if (op.r < 0 || op.r % 8 || op.r > g->Ns) TSD_FAIL(TSD_E_ARG, "token merge: r=%d (a multiple of 8 in 0..%d)", op.r, g->Ns);
  return TSD_OK;
}

int launch_tome_plan(tsd_ctx* ctx, const TomeOp& op) {
  TomeGrid g;
  TSD_TRY(tome_grid(op, &g));
  if (op.C <= 0 || op.C % 64 || op.C > 8192 || op.ldx < op.C || op.ldx % 8)
    TSD_FAIL(TSD_E_SHAPE, "token merge: C=%d (a multiple of 64 up to 8192) pitch %d", op.C, op.ldx);
  if (!ctx->launch()) return TSD_OK;
  if (!op.x || !op.node_max || !op.node_idx || !op.row_of || !op.start || !op.members) TSD_FAIL(TSD_E_ARG, "token merge: a NULL tensor");
  if ((uintptr_t)op.x & 15) TSD_FAIL(TSD_E_ARG, "token merge: the metric is not 16-byte aligned");
  TomeMatchK mk;
  mk.x = op.x; mk.sx = (int64_t)g.N * op.ldx; mk.ldx = op.ldx; mk.C = op.C; mk.g = g; mk.node_max = op.node_max; mk.node_idx = op.node_idx;
  TomeSelectK sk;
  sk.node_max = op.node_max; sk.node_idx = op.node_idx; sk.g = g; sk.r = op.r; sk.row_of = op.row_of; sk.start = op.start; sk.members = op.members;
  const size_t lds = ((size_t)g.Ns + g.Nd + 256 + TS_WAVES + 2) * 4;   // <= 132168 bytes at 32768 tokens
  static std::atomic<unsigned long long> attr{0};  // one bit per device
  if (!((attr.load(std::memory_order_relaxed) >> (ctx->device & 63)) & 1)) {
    HIP_TRY(hipFuncSetAttribute((const void*)k_tome_select, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr.fetch_or(1ull << (ctx->device & 63), std::memory_order_relaxed);
  }
  ProfScope prof(ctx, KC_ELEMENTWISE);
  prof.kernels = 2;
  const dim3 mg((unsigned)ceil_div(g.Ns, TM_SRC), (unsigned)op.B);
  if (op.C == TM_HOLD_KB * TM_KB) hipLaunchKernelGGL(k_tome_match<1>, mg, dim3(TM_THREADS), 0, ctx->stream, mk);
  else hipLaunchKernelGGL(k_tome_match<0>, mg, dim3(TM_THREADS), 0, ctx->stream, mk);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_tome_select, dim3((unsigned)op.B), dim3(TS_THREADS), lds, ctx->stream, sk);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

static int tome_rows_check(tsd_ctx* ctx, const char* what, int B, int N, int C, int Sm, int ldx, int ldy, const void* a, const void* b) {
  if (B <= 0 || B > 65535 || N < 1 || N > TOME_MAX_TOKENS || Sm < 1 || Sm > N) TSD_FAIL(TSD_E_SHAPE, "%s: B=%d N=%d rows %d", what, B, N, Sm);
  if (C <= 0 || C % 8 || C > 8192 || ldx < C || ldy < C || ldx % 8 || ldy % 8) TSD_FAIL(TSD_E_SHAPE, "%s: C=%d (a multiple of 8) pitches %d / %d", what, C, ldx, ldy);
  if (ctx->launch() && (((uintptr_t)a | (uintptr_t)b) & 15)) TSD_FAIL(TSD_E_ARG, "%s: a tensor is not 16-byte aligned", what);
  return TSD_OK;
}

int launch_tome_merge(tsd_ctx* ctx, const half_t* x, int ldx, int B, int N, int C, int Sm, const int* start, const int* members, half_t* y, int ldy) {
  TSD_TRY(tome_rows_check(ctx, "token merge rows", B, N, C, Sm, ldx, ldy, x, y));
  if (!ctx->launch()) return TSD_OK;
  const int tpr = std::min(C / 8, TG_THREADS), rpb = TG_THREADS / tpr;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_tome_merge, dim3((unsigned)ceil_div(Sm, rpb), (unsigned)B), dim3(TG_THREADS), 0, ctx->stream, x, ldx, N, C / 8, Sm, tpr, rpb,
                     start, members, y, ldy);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}

int launch_tome_unmerge(tsd_ctx* ctx, const half_t* y, int ldy, int B, int N, int C, int Sm, const int* row_of, half_t* out, int ldo) {
  TSD_TRY(tome_rows_check(ctx, "token unmerge rows", B, N, C, Sm, ldy, ldo, y, out));
  if (!ctx->launch()) return TSD_OK;
  const int tpr = std::min(C / 8, TG_THREADS), rpb = TG_THREADS / tpr;
  ProfScope prof(ctx, KC_ELEMENTWISE);
  hipLaunchKernelGGL(k_tome_unmerge, dim3((unsigned)ceil_div(N, rpb), (unsigned)B), dim3(TG_THREADS), 0, ctx->stream, y, ldy, N, C / 8, Sm, tpr, rpb,
                     row_of, out, ldo);
  HIP_TRY(hipGetLastError());
  return TSD_OK;
}
