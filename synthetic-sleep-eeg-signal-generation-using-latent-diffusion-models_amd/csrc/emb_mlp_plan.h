// Host-side tile and split-K arithmetic of the time-embedding MLP kernels (emb_mlp.hip).  Plain C++, no HIP: tests/test_emb_mlp_plan.py
// reads it through eegldm_debug_emb_mlp_plan without a device.
#pragma once
#ifdef __HIPCC__
#define EMB_HD __host__ __device__
#else
#define EMB_HD
#endif

constexpr int EMB_TILE = 64;        // output tile edge (rows and columns) of one workgroup; 32 for small products (emb_pick_tile)
constexpr int EMB_KC = 64;          // reduction chunk staged in LDS per iteration; split-K ranges are whole chunks
constexpr int EMB_MAX_SPLIT = 32;   // upper bound of the split-K partial count (the fold reads them in order 0, 1, ...)
constexpr int EMB_SPLIT_TARGET = 512;   // workgroups aimed at by the split (two per CU of a 256-CU chip)

static inline int emb_tiles(int n, int tile = EMB_TILE) { return (n + tile - 1) / tile; }
// A product that 64 x 64 tiles would spread over fewer than EMB_SMALL_GRID workgroups (half the CUs of the chip) runs on 32 x 32 tiles:
// four times the workgroups, a quarter of the multiply per reduction chunk of each.  The k order of an output does not depend on the tile.
constexpr int EMB_SMALL_GRID = 128;
static inline int emb_pick_tile(long tiles64) { return tiles64 < EMB_SMALL_GRID ? 32 : 64; }

// Partition of a reduction of length K over `splits` workgroups per output tile: split z owns [z * kper, min(K, (z + 1) * kper)), kper a
// whole number of chunks, no split empty.  `tiles` = output tiles of the product.
static inline void emb_splitk_plan(int tiles, int K, int* splits, int* kper) {
  const int chunks = (K + EMB_KC - 1) / EMB_KC;
  int want = tiles > 0 ? (EMB_SPLIT_TARGET + tiles - 1) / tiles : 1;
  if (want > EMB_MAX_SPLIT) want = EMB_MAX_SPLIT;
  if (want > chunks) want = chunks;
  if (want < 1) want = 1;
  const int per = (chunks + want - 1) / want;      // chunks per split
  *kper = per * EMB_KC;
  *splits = (chunks + per - 1) / per;              // drops the splits that the rounding of `per` left empty
}
// how many of the 4 consecutive elements starting at `i` lie below `end`
EMB_HD static inline int emb_valid4(int i, int end) { const int v = end - i; return v < 0 ? 0 : (v > 4 ? 4 : v); }
