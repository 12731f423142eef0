// What forest_predict.hip and bagged_forest_predict.hip have in common on
// the host's side: the limits of the row tile, the rows a workgroup owns and
// the launch numbers that follow from them. Read by the host compiler too
// (tabular_ops.cpp), so no device code here: that is forest_device.h.
// docs/kernels.md "The forests' row tile".
#pragma once

constexpr int FOREST_BLOCK = 256;
constexpr int FOREST_MAX_CLASSES = 32;
constexpr int FOREST_MAX_FEATURES = 2048;
constexpr int FOREST_MIN_ROWS = 4;          // rows per workgroup: a power of two, at least this
// a kernel's whole LDS carve stays within this, so that two workgroups
// share a CU's 160 KiB
constexpr int FOREST_LDS_BUDGET = 80 * 1024;
static_assert(2 * FOREST_LDS_BUDGET <= 160 * 1024, "two workgroups share a CU");

// row stride of the tile in dwords: odd, so that lanes reading different
// features of different rows spread over the banks
constexpr int forest_row_stride(int F) { return F | 1; }

// Rows per workgroup for F features and K values a row: the largest power of
// two in FOREST_MIN_ROWS..max_rows whose fp32 tile fits tile_bytes and whose
// R * K items fit max_items. 0: none (F or K out of range).
constexpr int forest_tile_rows(int F, int K, int max_rows, int tile_bytes, int max_items) {
  if (F < 1 || F > FOREST_MAX_FEATURES || K < 1 || K > FOREST_MAX_CLASSES) return 0;
  int R = max_rows;
  while (R > FOREST_MIN_ROWS &&
         ((long long)R * forest_row_stride(F) * 4 > tile_bytes || R * K > max_items))
    R >>= 1;
  return R;
}

// What a launch of B rows, R = forest_tile_rows(...) of them a workgroup,
// passes to the kernel for its grid and its row-tile stage.
struct ForestTileLaunch {
  int rshift;                 // R == 1 << rshift
  unsigned blocks;            // ceil(B / R)
  int tile_bytes;             // the tile [R][forest_row_stride(F)] fp32
  int f_magic;                // ceil(2^20 / F): t / F == (t * f_magic) >> 20, t < 256
  int step_rows, step_cols;   // 256 / F, 256 % F
};
inline ForestTileLaunch forest_tile_launch(int B, int F, int R) {
  ForestTileLaunch g{};
  while ((1 << g.rshift) < R) ++g.rshift;
  g.blocks = (unsigned)(((long long)B + R - 1) >> g.rshift);
  g.tile_bytes = R * forest_row_stride(F) * 4;
  g.f_magic = ((1 << 20) + F - 1) / F;
  g.step_rows = FOREST_BLOCK / F;
  g.step_cols = FOREST_BLOCK % F;
  return g;
}
