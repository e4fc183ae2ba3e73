// gemm_tiles.h - THE table of GEMM / conv3x3 tile configurations: the launch switches of kernels_gemm.hip and the geometry the host
// planner (gemm_plan.cpp) reasons with are both generated from it.
//
//   X(id, WGM, WGN, FM, FN, NS, PP, LW, UF, HX)
//     WGM x WGN  wave grid            FM x FN  16x16 fragments per wave      NS  LDS ring slots
//     PP         ping-pong schedule   LW       loader waves (0 / 4)
//     UF_Y       the tile also has the upsample-fold variant (GemmArgs::ups == 2): the configurations the dispatcher can return for a
//                non-thin, unsplit conv3x3 with N % 160 == 0
//     HX_Y       ... and the halo-x variant, launched as id + GEMM_HX_ID
//   Every tile has the plain variant (dense and conv3x3) and the conv3x3 one with a fused 1x1 skip source.  The tile is
//   BM x BN = WGM*FM*16 x WGN*FN*16, a wave's sub-tile FM*16 x FN*16, the ring NS * (BM + BN) * 128 bytes of LDS.
// The order of the rows is the order the kernels are instantiated in, and with it the order of the functions in the code object.
#pragma once

#define GEMM_TILES_MAIN(X)                                                                                                          \
  X(0, 2, 2, 4, 5, 2, false, 0, UF_Y, HX_Y)  /* 128x160  72 KiB  big-M UNet widths (N % 160 == 0), 2 blocks/CU */                    \
  X(1, 2, 2, 2, 5, 2, false, 0, UF_Y, HX_N)  /*  64x160  56 KiB  mid-M */                                                            \
  X(2, 2, 2, 4, 4, 2, false, 0, UF_N, HX_Y)  /* 128x128  64 KiB  VAE widths */                                                       \
  X(3, 2, 2, 2, 4, 2, false, 0, UF_N, HX_N)  /*  64x128  48 KiB */                                                                   \
  X(4, 4, 1, 2, 1, 2, false, 0, UF_N, HX_N)  /* 128x16   36 KiB  N <= 16, many tiles (decoder 128 -> 3) */                           \
  X(5, 2, 2, 4, 5, 3, false, 0, UF_Y, HX_N)  /* 128x160 108 KiB  deep ring, 1 block/CU */                                            \
  X(6, 2, 2, 2, 5, 4, false, 0, UF_Y, HX_N)  /*  64x160 112 KiB  few-tile problems (M = 2048 level) */                               \
  X(7, 2, 2, 2, 5, 3, false, 0, UF_Y, HX_N)  /*  64x160  84 KiB */                                                                   \
  X(8, 2, 2, 4, 4, 3, false, 0, UF_N, HX_N)  /* 128x128  96 KiB */                                                                   \
  X(9, 2, 2, 2, 4, 4, false, 0, UF_N, HX_N)  /*  64x128  96 KiB */                                                                   \
  X(10, 2, 2, 2, 4, 3, false, 0, UF_N, HX_N) /*  64x128  72 KiB */                                                                   \
  X(11, 4, 2, 4, 5, 3, false, 0, UF_N, HX_N) /* 256x160 156 KiB  8 waves, 1 block/CU, two K-tiles of DMA in flight */                \
  X(13, 4, 2, 4, 4, 3, false, 0, UF_N, HX_N) /* 256x128 144 KiB  8 waves */                                                          \
  X(24, 4, 1, 1, 1, 4, false, 0, UF_N, HX_N) /*  64x16   40 KiB  N <= 16, few tiles (the UNet's 320 -> 4 output convolution) */      \
  /* loader-wave variants (LW = 4): 40 + the id of the 4-wave one-block-per-CU configuration they extend, 51 = 11 + loaders */       \
  X(45, 2, 2, 4, 5, 3, false, 4, UF_N, HX_N)                                                                                         \
  X(46, 2, 2, 2, 5, 4, false, 4, UF_N, HX_N)                                                                                         \
  X(47, 2, 2, 2, 5, 3, false, 4, UF_N, HX_N)                                                                                         \
  X(48, 2, 2, 4, 4, 3, false, 4, UF_N, HX_N)                                                                                         \
  X(49, 2, 2, 2, 4, 4, false, 4, UF_N, HX_N)                                                                                         \
  X(50, 2, 2, 2, 4, 3, false, 4, UF_N, HX_N)                                                                                         \
  X(51, 4, 2, 4, 5, 3, false, 4, UF_Y, HX_N) /* 256x160, staggered: 8 compute waves in two groups */                                 \
  X(53, 4, 2, 4, 4, 3, false, 4, UF_N, HX_N) /* 256x128 */                                                                           \
  X(54, 4, 2, 2, 5, 3, false, 4, UF_N, HX_N) /* 128x160, staggered: 8 compute waves of 32x80 */                                      \
  X(55, 4, 2, 2, 4, 3, false, 4, UF_N, HX_N) /* 128x128 */

#ifdef TSD_GEMM_EXPERIMENTAL  // measured, not faster: built only to reproduce those numbers
#define GEMM_TILES_EXPERIMENTAL(X)                                                                                                  \
  X(12, 4, 2, 4, 5, 2, false, 0, UF_N, HX_N) /* 256x160 104 KiB  8 waves */                                                          \
  X(14, 2, 2, 8, 5, 3, false, 0, UF_N, HX_N)                                                                                         \
  X(15, 2, 2, 8, 5, 2, false, 0, UF_N, HX_N)                                                                                         \
  X(16, 4, 2, 4, 5, 3, true, 0, UF_N, HX_N)  /* 256x160 ping-pong */                                                                 \
  X(17, 4, 2, 2, 5, 3, true, 0, UF_N, HX_N)  /* 128x160 ping-pong */                                                                 \
  X(18, 4, 2, 4, 4, 3, true, 0, UF_N, HX_N)  /* 256x128 ping-pong */                                                                 \
  X(19, 4, 2, 2, 4, 3, true, 0, UF_N, HX_N)  /* 128x128 ping-pong */                                                                 \
  X(20, 2, 2, 2, 5, 5, false, 0, UF_N, HX_N) /*  64x160, 5-slot ring: slower than 4 slots (667 vs 821 TF) */                         \
  X(21, 2, 2, 2, 4, 6, false, 0, UF_N, HX_N) /*  64x128, 6-slot ring */
#else
#define GEMM_TILES_EXPERIMENTAL(X)
#endif

constexpr int GEMM_HX_ID = 30;  // id of the halo-x variant = id of its plain tile + 30 (30 / 32)

struct GemmTile {
  int id, wgm, wgn, fm, fn, ns, lw;
  bool ups_fold, halo, experimental;
  constexpr int BM() const { return wgm * fm * 16; }
  constexpr int BN() const { return wgn * fn * 16; }
  constexpr int BMw() const { return fm * 16; }
  constexpr int BNw() const { return fn * 16; }
  // the halo-x variant keeps the W ring and stages its A tiles in two buffers of their own
  constexpr int lds_bytes(bool hx) const { return hx ? ns * BN() * 128 + 2 * (BM() / 8 + 1) * 1024 : ns * (BM() + BN()) * 128; }
  // GroupNorm statistics come out of the coalesced epilogue (FN >= 4, whole 32-row passes); never measured on the experimental tiles
  constexpr bool emits_gn_stats() const { return fn >= 4 && fm % 2 == 0 && !experimental; }
};

// the row of tile configuration `id` - of its plain tile for a halo-x id, *hx set - or nullptr for an id the build does not have
inline const GemmTile* gemm_tile(int id, bool* hx = nullptr) {
#define UF_Y true
#define UF_N false
#define HX_Y true
#define HX_N false
#define TSD_TILE_ROW(id, wgm, wgn, fm, fn, ns, pp, lw, uf, hx) {id, wgm, wgn, fm, fn, ns, lw, uf, hx, false},
#define TSD_TILE_ROW_X(id, wgm, wgn, fm, fn, ns, pp, lw, uf, hx) {id, wgm, wgn, fm, fn, ns, lw, uf, hx, true},
  static constexpr GemmTile tiles[] = {GEMM_TILES_MAIN(TSD_TILE_ROW) GEMM_TILES_EXPERIMENTAL(TSD_TILE_ROW_X)};
#undef TSD_TILE_ROW
#undef TSD_TILE_ROW_X
#undef UF_Y
#undef UF_N
#undef HX_Y
#undef HX_N
  if (hx) *hx = false;
  for (const GemmTile& t : tiles) {
    if (t.id == id) return &t;
    if (t.halo && t.id + GEMM_HX_ID == id) { if (hx) *hx = true; return &t; }
  }
  return nullptr;
}
