// gemm_plan.cpp - the host decision of one GEMM / conv3x3 launch: which tile configuration runs, in how many split-K slices, as which
// conv variant.  Pure host code - no context, no HIP call, no allocation - and the ONLY place that takes the decision: launch_gemm
// (kernels_gemm.hip) acts on the plan and leaves it in tsd_ctx::gemm_last, the graph asks it for the statistics geometry and the
// upsample-fold eligibility, tsd_debug_gemm_plan reports it without a device.  The decision fixes the fp32 summation tree, so the bitwise
// batch invariance of the product rests on it: everything here keys on the LAYER (rows per sample, N, K) - tests/test_gemm_plan_cpu.py
// holds the one place where it does not.
#include <string.h>

#include "common.h"
#include "gemm_tiles.h"

// Split-K by 2 pays when a 128-row tiling leaves about half the CUs idle and K is long: the M = 2048 level of the UNet
// (16 x 8 tiles of 128x160, K = 5120..23040).  64-row tiles fill the chip there but move 46 flop per LDS-DMA byte and
// are bound by the per-CU DMA rate; two 128-row half-K blocks move 71 flop/B.
// Split-K plan: number of K slices (1 = none) and the tile configuration the split launch runs with.
static int splitk_plan(const TsdOptions& o, int M, int N, int K, int batch, int rps, int* cfg) {
  const int on = o.splitk;
  // The decision must not depend on the batch size (bitwise batch invariance: a split changes the fp32 summation
  // tree), so it keys on the layer: rows per sample, N and K.
  //  * rps <= 256 (the 16x16 level of a 64x64 latent): 2 slices of 128-row tiles once K >= 4096;
  //  * rps <= 64 (an 8x8 level: the full-size UNet's deepest at a 64x64 latent, the 23-layer graph's at 32x32): M is
  //    a few hundred rows, so 64-row tiles and up to 8 slices - 32 tiles x 8 fill the chip where 16 tiles x 2 left
  //    7/8 of it idle.
  const int min_k = o.splitk_mink, max_tiles = o.splitk_tiles, small_ways = o.splitk_small;
  // Round 3 (late): two more layer classes that left half the chip idle at batch 8 -
  //  * rps <= 256 with at most 4 tile columns (the 32x32 -> 16x16 downsampling conv, N = 640, K = 5760: 64 tiles): 4 slices;
  //  * rps <= 1024 with N * rps <= 320 * 1024 (the 64x64 -> 32x32 downsampling conv, N = 320, K = 2880: 128 tiles): 2 slices.
  const int wide = o.splitk_wide;
  const bool mid = wide && rps > 256 && rps <= 1024 && (long long)N * rps <= 320LL * 1024 && K >= 2880;
  // Round 4 (TSD_GEMM_SK256): 256x160 tiles (the staggered loader-wave configuration 51) for split launches, with twice the slices so
  // that the grid stays the same: a K tile then pulls 52 KB from the L2 for twice the products of a 128x160 tile's 36 KB (98 instead of
  // 71 flop per L2 byte; the K loops of these layers run on the L2 -> CU path).  Bit 0: the 16x16-level layers that split
  // already; bit 1: the 32x32-level 640-wide convolutions (K >= 5760: 256 tiles of 128x160 today, no split).  Keyed on the layer only.
  const bool mid256 = (o.sk256 & 2) && rps == 1024 && N == 640 && K >= 5760;
  if (!on || batch != 1 || N <= 16 || rps <= 0 || (rps > 256 && !mid && !mid256)) return 1;
  const bool n160 = (N % 160 == 0);
  const int BN = n160 ? 160 : 128;
  int ways = 1, BM = 128;
  if (rps <= 64 && small_ways > 1) {
    ways = K >= 8192 ? 8 : (K >= 2048 ? 4 : (K >= 1024 ? 2 : 1));
    if (ways > small_ways) ways = small_ways;
    BM = 64;
    const int deep = o.splitk_ring4;
    if (cfg) *cfg = deep ? (n160 ? 6 : 9) : (n160 ? 7 : 10);
  } else {
    const int big_env = o.splitk_big;
    // 2 slices for the 23-layer UNet at batch 8; the full-size UNet's graph asks for 4 (gemm_set_splitk_big: +4.3 % at its batch of 4,
    // -0.8 % on the headline).  A per-GRAPH choice, so every batch size of a model sums in the same tree.
    const int big_ways = big_env ? big_env : (o.sk_big_graph ? o.sk_big_graph : 2);
    ways = K >= 8192 ? big_ways : (K >= min_k ? 2 : 1);
    if (wide && ways == 2 && ceil_div(N, BN) <= 4) ways = 4;
    if (mid) ways = 2;
    const int sk128 = o.sk_cfg;  // 45: the same tile with loader waves
    if (cfg) *cfg = n160 ? sk128 : 8;
    const int tn = ceil_div(N, BN);
    const bool xcd256 = tn % 8 == 0 || (wide && rps % 256 == 0 && (tn * (rps / 256)) % 8 == 0);  // a tile's slices stay on one XCD
    if (n160 && xcd256 && ((mid256 && !mid) || ((o.sk256 & 1) && rps == 256 && ways >= 2 && ways <= 4))) {
      ways = mid256 ? 2 : ways * 2;
      BM = 256;
      if (cfg) *cfg = 51;
    }
  }
  // Eligibility looks at N only (8 | N-tiles keeps a tile's slices on one XCD for any M): a condition on the tile
  // count would make the split - and with it the fp32 summation tree - depend on the batch.
  // (round 3: 8 | tiles of one sample does the same for the layers with fewer tile columns)
  // The two M-dependent guards below are meant never to trigger inside the API's limits (B <= 16), and with rps > 64 they do not
  // (at most 16 x 2 x 8 = 256 tiles of 128 rows).  With 64-row tiles one of them DOES: the first GEGLU linear of a C = 1280 attention
  // block at an 8x8 level (rps 64, N = 10240, K = 1280) has 64 tile columns, and from B = 9 on its 9+ tile rows exceed
  // 2 * splitk_tiles - it splits K in two for B = 1..8 and not at all for B = 9..16, so a sample computed alone is not bitwise its row of
  // such a batch.  The 23-layer UNet is there at a 32x32 latent, the full-size one at 64x64.  Known and pinned
  // (tests/test_gemm_plan_cpu.py, the strict xfail); not fixed here because the fix changes bits for some batch sizes.
  const int tiles_n = ceil_div(N, BN), tiles = ceil_div(M, BM) * tiles_n;
  const bool xcd_ok = tiles_n % 8 == 0 || (wide && rps % BM == 0 && (tiles_n * (rps / BM)) % 8 == 0);
  if (ways == 1 || !xcd_ok || tiles > 2 * max_tiles || (ways - 1) * tiles > 4095) return 1;
  return ways;
}

// the tile configuration of an unsplit launch
static int choose_cfg(const TsdOptions& o, int M, int N, int K, int batch, bool conv) {
  {  // tuning aid: TSD_GEMM_CFG_OVERRIDE="M,N,K:cfg[;M,N,K:cfg...]" forces a tile configuration for exact shapes inside a real step
    const char* ov = o.cfg_override;
    if (ov[0]) {
      for (const char* q = ov; q && *q;) {
        int m = 0, n = 0, k = 0, c = 0;
        if (sscanf(q, "%d,%d,%d:%d", &m, &n, &k, &c) == 4 && m == M && n == N && k == K) return c;
        q = strchr(q, ';');
        if (q) q++;
      }
    }
  }
  if (N <= 16) {
    // the UNet's 320 -> 4 output convolution is one 128-row block per CU walking 45 K tiles behind a 2-slot ring: 64-row tiles with
    // a 4-slot ring (two blocks per CU, three tiles in flight) take 20 us where it took 33 in the step; with thousands of tiles
    // (the decoder's 128 -> 3 at 512 x 512) the 128-row tile stays ahead (277 vs 329 us).  Bitwise the same results either way.
    const int thin = o.thin_cfg;
    if (thin) return thin;
    return (long long)ceil_div(M, 128) * batch <= 1024 ? 24 : 4;
  }
  const bool n160 = (N % 160 == 0);
  const int BN = n160 ? 160 : 128;
  // measured on MI355X (scripts/bench_gemm.py with REAL_EPI=1, pinned issue order):
  //  * >= 2 tiles of 128 rows per CU: two 4-wave blocks per CU (cfg 0/2);
  //  * dense GEMMs whose 256x160 tiling is exactly one or two full rounds of the 256 CUs: the 8-wave tile (cfg 11)
  //    halves the operand traffic per flop and its prologue/epilogue count;
  //  * around one 128-row tile per CU: long K -> one 128-row block with a 3-slot DMA ring (one wave per SIMD, the
  //    pinned schedule keeps its MFMA pipe fed), short K -> 64-row tiles, two blocks per CU (fixed costs overlap);
  //  * fewer tiles than that: 64-row tiles with 3 ring slots, 4 when K is long.
  const long long t128 = (long long)ceil_div(M, 128) * ceil_div(N, BN) * batch;
  const long long t256 = (long long)ceil_div(M, 256) * ceil_div(N, BN) * batch;
  const int tune = o.tune;  // A/B switch for the rules below
  // Round 3: the staggered wave-specialised 256-row tiles (51 / 53: 8 compute waves in two groups + 4 loader waves) where a
  // 256-row tiling gives every CU whole tiles - measured -5...-10 % against configurations 0 / 2 / 11 on these shapes
  // (profiles/r03_loader_waves_ab.txt); TSD_GEMM_TUNE bit 2 turns them off.  Results are bitwise those of every other tile.
  if ((tune & 4) && M % 256 == 0) {
    if (n160 && conv && t256 >= 256 && t256 % 256 == 0) return 51;
    if (n160 && !conv && K >= 256 && (t256 == 256 || t256 == 384 || t256 == 512 || (t256 >= 192 && t256 < 256))) return 51;  // K < 256 (the im2col input conv, one K tile): nothing for loaders to do, 128x160 is 15 us against 20  // 192: the 16x16 level's fused q/k/v projection (23 us against 26-33 for the other tiles)
    if (!n160 && conv && N % 128 == 0 && N >= 256 && t256 >= 512 && K >= 2304) return 53;  // K = 1152 (128 -> 256 at 256 x 256): 128x128 tiles, 0.42 vs 0.45 ms in-step
  }
  if ((tune & 1) && !conv && n160 && K >= 256 && (t256 == 256 || t256 == 512) && M % 256 == 0) return 11;
  if (t128 >= 512) return n160 ? 0 : 2;
  // Round 3 (late), measured INSIDE the step (TSD_GEMM_CFG_OVERRIDE + experiments/drivers/instep_sweep.sh; the repeated-launch microbenchmark
  // keeps the operands in the L2 and ranks these the other way round): dense GEMMs with exactly one 128-row tile per CU run the
  // staggered 128x160 tile with loader waves (54: 8192x640x640 19.4 -> 17.7 us, 8192x640x2560 42 -> 39.7 us), and the 256-tile
  // 64-row problems of the 16x16 level the 64x160 tile with loader waves (47: 2048x1280x1280 20.2 -> 19.2 us); TSD_GEMM_TUNE bit 3
  if ((tune & 8) && !conv && n160 && t128 == 256 && M % 128 == 0 && K < 5760) return 54;
  if ((tune & 8) && !conv && n160 && N >= 8192 && t128 >= 384) return 0;  // few rows, very wide (context K | V^T: 34 -> 29 us)
  if (t128 >= 192) return (K >= 2560 || !(tune & 2)) ? (n160 ? 5 : 8) : (n160 ? 1 : 3);
  if (K >= 5760) return n160 ? 6 : 9;
  {  // 256 tiles: measured on 2048x1280x1280; 128 tiles: the full-size UNet's 1024x1280x1280 at batch 4 (0.483 -> 0.463 ms for its 25 launches)
    const long long t64 = (long long)ceil_div(M, 64) * ceil_div(N, BN) * batch;
    if ((tune & 8) && !conv && n160 && (t64 == 256 || t64 == 128) && M % 64 == 0 && N >= 1280) return 47;
  }
  return n160 ? 7 : 10;
}

// conv3x3 problems the halo-x K order can run: stride 1 on the source grid, whole 128-pixel tiles made of 64- or 128-pixel
// image-row segments, no split-K, row-major weights (the halo-x K order addresses W row-major: a launch that reads the K-tile-major
// weight copy keeps its plain tile)
// OFF by default: the halo-x order sums K in a different order than every other tile configuration, and which
// configuration runs depends on M - a sample computed alone would no longer equal its row of a batch bit for bit.  Measured
// with it on (TSD_CONV_HALO=1: the 128x128-tile convs, 2: the 128x160 ones too): decoder 26.1 -> 25.7 ms, encoder 13.95 ->
// 13.70 ms, UNet step unchanged.  tests/test_gpu_ops.py keeps the path correct against the plain configurations.
static bool hx_shape_ok(const GemmArgs& a, int ways) {
  return a.conv && a.stride == 1 && !a.ups && a.pad == 1 && ways <= 1 && !a.Cin1 && a.Hs == a.Ho && a.Ws == a.Wo && a.Cin % 64 == 0 &&
         (a.Wo == 64 || a.Wo % 128 == 0) && ((long long)a.Ho * a.Wo) % 128 == 0 && a.M % 128 == 0 && a.Ho < 2040 && a.Wo < 2040 &&
         (a.w_kts == 0 || a.w_kts == 128);
}
static bool hx_eligible(const TsdOptions& o, const GemmArgs& a, int ways) { return o.conv_halo > 0 && hx_shape_ok(a, ways); }

// Upsample fold (GemmArgs::ups == 2): may this conv3x3 over a nearest-2x upsampled source run as four parity-planar 2x2 convolutions?
// Decided on the LAYER (source plane, channels, width, epilogue) and never on M: which kernel runs must not change with the batch.
//  * stride 1, pad 1, no fused skip, no residual / statistics / fp32 epilogue (a one-parity tile holds no 32-raster-row slab);
//  * Cin % 64 == 0 (whole K tiles per folded tap) and N % 160 == 0 (the tile family the variant is built for);
//  * Hs * Ws % 256 == 0: every tile height the dispatcher can choose divides a parity plane;
//  * no split-K for the executed problem (rows per sample, N, 4 * Cin).
bool gemm_ups_fold_ok(const TsdOptions& o, const GemmArgs& a) {
  if (!a.conv || a.stride != 1 || a.pad != 1 || a.Cin1 || a.Cin2 || a.batch != 1 || a.Vt) return false;
  if (a.epi & (EPI_RESIDUAL | EPI_RES_UPS | EPI_GNSTATS | EPI_OUT_F32)) return false;
  if (a.Cin <= 0 || a.Cin % 64 || a.N % 160 || a.K != 9 * a.Cin) return false;
  const long long S = (long long)a.Hs * a.Ws;
  if (a.Hs <= 0 || a.Ws <= 0 || a.Hs >= 2040 || a.Ws >= 2040 || S % 256 || a.Ho != 2 * a.Hs || a.Wo != 2 * a.Ws || a.M <= 0 || a.M % (4 * S)) return false;
  return splitk_plan(o, a.M, a.N, 4 * a.Cin, a.batch, a.Ho * a.Wo, nullptr) == 1;
}

int GemmPlan::gn_slabs(int rows_per_sample, int groups) const {
  if (refused || !gn_stats || groups <= 0 || N % groups || (N & 7) || batch != 1 || rows_per_sample <= 0) return 0;
  const int cpg = N / groups;  // a tile whose wave columns split a group would write that group's slot from two waves
  if (BNw % cpg || rows_per_sample % BMw || M % rows_per_sample) return 0;
  return rows_per_sample / 32;  // one slab per 32-row epilogue pass, independent of the tile shape
}

GemmPlan gemm_plan(const TsdOptions& o, const GemmArgs& a) {
  GemmPlan p;
  p.M = a.M; p.N = a.N; p.batch = a.batch;
  const bool conv = a.conv != 0, uf = conv && a.ups == 2, forced = o.force_cfg >= 0;
  if (uf && !gemm_ups_fold_ok(o, a)) { p.refused = "this launch cannot run the upsample fold (ups = 2)"; return p; }
  p.K = uf ? 4 * a.Cin : a.K;  // the fold runs on the folded copies; the launch stays DESCRIBED (record, profile) as the 3x3 it computes
  int id = o.force_cfg;        // a forced configuration (the bench / check / replay entries) runs unsplit
  if (!forced) {
    if (!uf) p.ways = splitk_plan(o, a.M, a.N, a.K, a.batch, a.rows_per_sample_hint, &id);
    if (p.ways <= 1) id = choose_cfg(o, a.M, a.N, p.K, a.batch, conv);
    // halo-x measured: -3...5 % on the 128x128-tile convs of the VAE (N = 128 / 256 / 512), nothing on the 128x160 ones (TSD_CONV_HALO=2 turns those on too)
    if (hx_eligible(o, a, p.ways) && (id == 2 || (id == 0 && o.conv_halo >= 2))) id += GEMM_HX_ID;
    // rounds 3-4: the fused-skip variant of the 128x128 two-blocks-per-CU tile kept its offset tables in scratch (48 B per lane) and the
    // decoder's 256 -> 128 residual block at 512 x 512 (K = 1152 + 256) ran its 64-row sibling instead (1.18 ms against 1.35).  Round 5:
    // the scratch is gone (conv_tap_ptrs); TSD_GEMM_SKIP128=0 restores the detour for A/B runs
    if (conv && a.Cin1 > 0 && id == 2 && !o.skip128) id = 3;
  }
  p.cfg = id;
  bool hx = false;
  const GemmTile* t = gemm_tile(id, &hx);
  if (!t) { p.refused = "unknown tile configuration"; return p; }
  if (hx && !hx_shape_ok(a, p.ways)) { p.refused = "halo-x tile configuration on an ineligible problem"; return p; }
  if (uf && !t->ups_fold) { p.refused = "tile configuration has no upsample-fold variant"; return p; }
  p.variant = uf ? 3 : hx ? 1 : (conv && a.Cin1 > 0) ? 2 : 0;
  p.BM = t->BM(); p.BN = t->BN(); p.BMw = t->BMw(); p.BNw = t->BNw();
  p.lds_bytes = t->lds_bytes(hx);
  p.gn_stats = t->emits_gn_stats();
  if (p.ways > 1) p.ws_floats = (int64_t)(p.ways - 1) * ceil_div(a.M, p.BM) * ceil_div(a.N, p.BN) * p.BM * p.BN;
  return p;
}
