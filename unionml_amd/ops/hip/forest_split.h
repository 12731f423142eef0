// Split walk of a gradient-boosted forest (forest_split_predict.hip): the
// LDS carve, the launcher rule and the launcher's declaration. ops/forest.py
// is the Python copy of the constants and of the two functions (the extension
// exports them; a GPU test holds the two equal). docs/kernels.md "Split walk".
//
// The forest is packed with the bagged node (bagged_forest.h), a leaf's `thr`
// holding its row of leaf_values, and tree t = it * K + k adds to score
// column k:
//
//   nodes       [N]     BaggedNode, 8 bytes, trees back to back, breadth-first
//   tree_first  [T + 1] int32: first node of tree t, tree_first[T] == N
//   leaf_values [L]     fp64, one value a leaf
//   baseline    [K]     fp64
//
// Only the fp64 SUM needs the tree order; the walks do not. Two stream-ordered
// launches: forest_split_walk_kernel spreads (row, tree) walks over the whole
// device and leaves every walk's leaf row in leaf_rows [T][B] (int32, global
// memory); forest_split_sum_kernel adds the leaves of a (row, class) in
// iteration order, one fp64 rounding each.
#pragma once

#include <hip/hip_runtime_api.h>

#include "bagged_forest.h"
#include "forest_limits.h"

// The walk kernel's LDS carve, bytes from the base of dynamic LDS:
//   [0, 32768)       the slice's tree prefixes: SPLIT_PREFIX_SLOTS nodes, tree
//                    s of the slice owning slots [s * PS, (s + 1) * PS), PS
//                    the power of two at or above P, the nodes of a tree kept
//                    here: P = min(pow2floor(SPLIT_PREFIX_SLOTS / S), the
//                    largest tree, the caller's cap)
//   [32768, 34816)   the slice's tree table: SPLIT_SLICE_TREES first nodes and
//                    as many node counts
//   [34816, ...)     the row tile [R][F | 1] fp32, within FOREST_LDS_BUDGET
constexpr int SPLIT_PREFIX_SLOTS = 4096;
constexpr int SPLIT_SLICE_TREES = 256;     // the most trees of a slice: one table entry a thread
constexpr int SPLIT_WALK_ITEMS = 1024;     // RP * S aims at this: four walks a thread
constexpr int SPLIT_WG_MAX_ROWS = 256;     // the most rows per workgroup
constexpr int SPLIT_LDS_TAB_OFF = SPLIT_PREFIX_SLOTS * 8;
constexpr int SPLIT_LDS_TILE_OFF = SPLIT_LDS_TAB_OFF + 2 * SPLIT_SLICE_TREES * 4;
constexpr int SPLIT_TILE_BYTES = FOREST_LDS_BUDGET - SPLIT_LDS_TILE_OFF;
constexpr int SPLIT_SUM_AHEAD = 8;         // sum kernel: index and value loads in flight
// the leaf_rows scratch of one call: ops/forest.py scores larger calls in
// row blocks below this
constexpr long long SPLIT_SCRATCH_BYTES = 64ll << 20;

static_assert(SPLIT_LDS_TAB_OFF == 32768 && SPLIT_LDS_TILE_OFF == 34816 &&
                  SPLIT_TILE_BYTES == 47104,
              "the carve above");
static_assert(SPLIT_PREFIX_SLOTS % FOREST_BLOCK == 0 && SPLIT_SLICE_TREES == FOREST_BLOCK,
              "a thread loads PREFIX_SLOTS / BLOCK nodes and one table entry");
static_assert(SPLIT_WG_MAX_ROWS <= SPLIT_WALK_ITEMS && SPLIT_WG_MAX_ROWS <= FOREST_BLOCK,
              "a slice holds at least one tree; a row tile at most a row a thread");
static_assert(FOREST_MIN_ROWS * (forest_row_stride(FOREST_MAX_FEATURES) * 4) <= SPLIT_TILE_BYTES,
              "the widest row fits at the smallest R");

// Rows per workgroup that the tile budget allows for F features: up to
// SPLIT_WG_MAX_ROWS (the walk carries no per-class state, so K plays no part).
// The launcher takes fewer when the batch is smaller.
constexpr int forest_split_rows_per_wg(int F) {
  return forest_tile_rows(F, 1, SPLIT_WG_MAX_ROWS, SPLIT_TILE_BYTES, SPLIT_WG_MAX_ROWS);
}
static_assert(forest_split_rows_per_wg(64) == 128 && forest_split_rows_per_wg(5) == 256 &&
                  forest_split_rows_per_wg(45) == 256 && forest_split_rows_per_wg(300) == 32 &&
                  forest_split_rows_per_wg(2048) == 4 && forest_split_rows_per_wg(2049) == 0,
              "forest_split_rows_per_wg and ops/forest.py split_rows_per_wg disagree");

// Trees per slice of a launch whose workgroups hold `rows` rows (rounded up
// to a power of two, RP): SPLIT_WALK_ITEMS / RP, at least 1, at most
// SPLIT_SLICE_TREES, at most T, and at most `cap` when cap > 0. A lone row
// becomes ceil(T / 256) workgroups of one-lane walks.
constexpr int forest_split_trees_per_slice(int rows, int T, int cap) {
  int rp = 1;
  while (rp < rows) rp <<= 1;
  int n = SPLIT_WALK_ITEMS / rp;
  if (n > SPLIT_SLICE_TREES) n = SPLIT_SLICE_TREES;
  if (n > T) n = T;
  if (n < 1) n = 1;
  if (cap > 0 && cap < n) n = cap;
  return n;
}
static_assert(forest_split_trees_per_slice(1, 1000, 0) == 256 &&
                  forest_split_trees_per_slice(1, 100, 0) == 100 &&
                  forest_split_trees_per_slice(3, 1000, 0) == 256 &&
                  forest_split_trees_per_slice(64, 1000, 0) == 16 &&
                  forest_split_trees_per_slice(128, 1000, 0) == 8 &&
                  forest_split_trees_per_slice(256, 3, 0) == 3 &&
                  forest_split_trees_per_slice(256, 1000, 0) == 4 &&
                  forest_split_trees_per_slice(65, 100, 5) == 5,
              "forest_split_trees_per_slice and ops/forest.py split_trees_per_slice disagree");

// Rows per workgroup of the sum kernel: one (row, class) item a thread.
constexpr int forest_split_sum_rows(int K) {
  int r = 1;
  while (2 * r * K <= FOREST_BLOCK) r <<= 1;
  return r;
}
static_assert(forest_split_sum_rows(1) == 256 && forest_split_sum_rows(10) == 16 &&
                  forest_split_sum_rows(32) == 8 && forest_split_sum_rows(3) == 64,
              "pow2floor(256 / K)");

extern "C" {

// scores[b][k] = (((0 + baseline[k]) + leaf(tree k, b)) + leaf(tree K + k, b)) + ...
// for b < B, one fp64 rounding per addition; labels[b] = the first column
// with the largest score, or score > 0 when K == 1. X [B][F] fp32; nodes
// [n_nodes]; tree_first [T + 1], T a multiple of K; leaf_values [n_leaves];
// baseline [K]; max_tree_nodes the largest tree's node count (it only trims
// the LDS prefix); leaf_rows at least T * B int32 of scratch, overwritten.
// prefix_nodes < 0: as many nodes of each tree in LDS as fit, otherwise at
// most that many (0: every visit reads global memory); trees_per_slice 0: by
// the rule above, otherwise at most that many. Two launches on `stream`. 0
// launched, -2 the dynamic-LDS attribute failed, -3 arguments outside the
// kernels' range (tabular_launch.h's convention).
int launch_forest_split_predict(const float* X, int B, int F, int K,
                                const BaggedNode* nodes, int n_nodes,
                                const int* tree_first, int T, int max_tree_nodes,
                                const double* leaf_values, int n_leaves,
                                const double* baseline, int prefix_nodes,
                                int trees_per_slice, int* leaf_rows,
                                double* scores, int* labels, hipStream_t stream);

}  // extern "C"
