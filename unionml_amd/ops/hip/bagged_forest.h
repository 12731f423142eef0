// Bagged-forest inference (bagged_forest_predict.hip): the packed node, the
// LDS carve and the launcher's declaration. ops/forest.py is the Python copy
// of the node layout and of the constants (the extension exports them; a GPU
// test holds the two equal). docs/kernels.md "Bagged-forest inference".
//
// A packed bagged forest is T trees that each add a whole K-vector (class
// fractions, or one regression value) to the row's sum; the result is the
// sum over the trees in order, divided by T. Every tree is renumbered
// breadth-first, so a node's children are adjacent and a tree's top levels
// are a prefix of its nodes:
//
//   nodes       [N]     BaggedNode, 8 bytes, trees back to back
//   tree_first  [T + 1] int32: first node of tree t, tree_first[T] == N
//   leaf_values [L][K]  fp64, one row per leaf of the forest
//
// A visit at node i (counted from the tree's root) reads one BaggedNode and
// the row's feature x = X[row][meta & 0x7FF]:
//
//   dist = meta >> 12                      (0: a leaf)
//   next = i + dist + ((x != x ? (meta >> 11) & 1 : x <= thr) ? 0 : 1)
//
// A LEAF has dist == 0 and the bits of its `thr` are the row of leaf_values
// that the tree adds.
#pragma once

#include <hip/hip_runtime_api.h>

#include "forest_limits.h"

struct BaggedNode {
  float thr;       // rd32(threshold): x <= t in fp64  <=>  x <= thr in fp32;
                   // a leaf: the bits of its leaf_values row (uint32)
  unsigned meta;   // feature 0..10 | missing-left 11 | distance to the left child 12..31
};
static_assert(sizeof(BaggedNode) == 8, "one 8-byte load per visit");

static_assert(FOREST_MAX_FEATURES <= 1 << 11, "a node's feature has 11 bits of meta");
constexpr int BAGGED_MAX_TREE_NODES = 1 << 20;     // 20 bits of distance
constexpr int BAGGED_MAX_ROWS = 256;               // the most rows per workgroup
constexpr int BAGGED_META_MISSING_LEFT = 1 << 11;
constexpr int BAGGED_META_DIST_SHIFT = 12;

// The LDS carve, bytes from the base of dynamic LDS:
//   [0, 16384)       the chunk's tree prefixes: BAGGED_PREFIX_SLOTS nodes,
//                    tree c of the chunk owning slots [c * PS, (c + 1) * PS)
//   [16384, 32768)   the running sums [rows][K] fp64, BAGGED_MAX_ITEMS of them
//   [32768, 40960)   leaf_idx [C][RP] int32: the leaf_values row that tree c
//                    of the chunk gives row r, BAGGED_WALK_ITEMS of them
//   [40960, 45056)   two tree tables (this chunk's and the next one's), each
//                    BAGGED_CHUNK_TREES first nodes and as many node counts
//   [45056, ...)     the row tile [R][F | 1] fp32, within FOREST_LDS_BUDGET
constexpr int BAGGED_PREFIX_SLOTS = 2048;
constexpr int BAGGED_MAX_ITEMS = 2048;     // R * K <= this: (row, class) sums
constexpr int BAGGED_WALK_ITEMS = 2048;    // RP * C <= this: (row, tree) walks of a chunk
constexpr int BAGGED_CHUNK_TREES = 256;    // the most trees of a chunk: one table entry a thread
constexpr int BAGGED_LDS_ACC_OFF = BAGGED_PREFIX_SLOTS * 8;
constexpr int BAGGED_LDS_LEAF_OFF = BAGGED_LDS_ACC_OFF + BAGGED_MAX_ITEMS * 8;
constexpr int BAGGED_LDS_TAB_OFF = BAGGED_LDS_LEAF_OFF + BAGGED_WALK_ITEMS * 4;
constexpr int BAGGED_LDS_TILE_OFF = BAGGED_LDS_TAB_OFF + 2 * 2 * BAGGED_CHUNK_TREES * 4;
constexpr int BAGGED_TILE_BYTES = FOREST_LDS_BUDGET - BAGGED_LDS_TILE_OFF;

static_assert(BAGGED_LDS_TILE_OFF == 45056 && BAGGED_TILE_BYTES == 36864, "the carve above");
static_assert(BAGGED_PREFIX_SLOTS % FOREST_BLOCK == 0 && BAGGED_CHUNK_TREES == FOREST_BLOCK,
              "a thread prefetches PREFIX_SLOTS / BLOCK nodes and one table entry");
static_assert(BAGGED_MAX_ROWS * FOREST_MAX_CLASSES >= BAGGED_MAX_ITEMS &&
                  FOREST_MIN_ROWS * FOREST_MAX_CLASSES <= BAGGED_MAX_ITEMS,
              "the widest K fits at the smallest R");
static_assert(BAGGED_MAX_ROWS <= BAGGED_WALK_ITEMS, "a chunk holds at least one tree");
static_assert(FOREST_MIN_ROWS * (forest_row_stride(FOREST_MAX_FEATURES) * 4) <= BAGGED_TILE_BYTES,
              "the widest row fits at the smallest R");
static_assert(BAGGED_MAX_ITEMS * FOREST_MAX_CLASSES < (1 << 20),
              "i / K by a 20-bit multiplier is exact for i < BAGGED_MAX_ITEMS");

// Rows per workgroup for F features and K values a leaf (forest_tile_rows):
// up to BAGGED_MAX_ROWS, the tile within BAGGED_TILE_BYTES and the R * K
// sums within BAGGED_MAX_ITEMS.
constexpr int bagged_rows_per_wg(int F, int K) {
  return forest_tile_rows(F, K, BAGGED_MAX_ROWS, BAGGED_TILE_BYTES, BAGGED_MAX_ITEMS);
}
static_assert(bagged_rows_per_wg(64, 10) == 128 && bagged_rows_per_wg(64, 32) == 64 &&
                  bagged_rows_per_wg(5, 2) == 256 && bagged_rows_per_wg(300, 3) == 16 &&
                  bagged_rows_per_wg(2048, 1) == 4 && bagged_rows_per_wg(2049, 1) == 0 &&
                  bagged_rows_per_wg(4, 33) == 0,
              "bagged_rows_per_wg and ops/forest.py bagged_rows_per_wg disagree");

// Trees per chunk of a workgroup that holds `rows` rows (1..R; the last
// workgroup of a launch may hold fewer than R): as many as BAGGED_WALK_ITEMS
// (row, tree) walks allow with the rows rounded up to a power of two, at
// most BAGGED_CHUNK_TREES, at most T, and at most `cap` when cap > 0. A lone
// row is walked through 256 trees at once.
constexpr int bagged_trees_per_chunk(int rows, int T, int cap) {
  int rp = 1;
  while (rp < rows) rp <<= 1;
  int n = BAGGED_WALK_ITEMS / rp;
  if (n > BAGGED_CHUNK_TREES) n = BAGGED_CHUNK_TREES;
  if (n > T) n = T;
  if (cap > 0 && cap < n) n = cap;
  return n;
}
static_assert(bagged_trees_per_chunk(1, 100, 0) == 100 && bagged_trees_per_chunk(1, 1000, 0) == 256 &&
                  bagged_trees_per_chunk(128, 100, 0) == 16 && bagged_trees_per_chunk(65, 100, 5) == 5 &&
                  bagged_trees_per_chunk(256, 100, 0) == 8,
              "bagged_trees_per_chunk");

extern "C" {

// probs[b][k] = (((0 + v(tree 0, b)[k]) + v(tree 1, b)[k]) + ...) / T for
// b < B, v(t, b) the leaf_values row of the leaf that row b reaches in tree
// t; one fp64 rounding per addition and one for the division. labels[b] =
// the first k with the largest probs[b][k]. X [B][F] fp32; nodes [n_nodes];
// tree_first [T + 1]; leaf_values [n_leaves][K]; max_tree_nodes the largest
// tree's node count (it only trims the LDS prefix). prefix_nodes < 0: as many
// nodes of each tree in LDS as fit, otherwise at most that many (0: every
// visit reads global memory); trees_per_chunk 0: as many as fit, otherwise
// at most that many. 0 launched, -2 the dynamic-LDS attribute failed, -3
// arguments outside the kernel's range (tabular_launch.h's convention).
int launch_bagged_forest_predict(const float* X, int B, int F, int K,
                                 const BaggedNode* nodes, int n_nodes,
                                 const int* tree_first, int T, int max_tree_nodes,
                                 const double* leaf_values, int n_leaves,
                                 int prefix_nodes, int trees_per_chunk,
                                 double* probs, int* labels, hipStream_t stream);

}  // extern "C"
