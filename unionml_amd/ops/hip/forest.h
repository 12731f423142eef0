// Forest inference (forest_predict.hip): the packed node, the LDS carve and
// the launcher's declaration. ops/forest.py is the Python copy of the node
// layout and of the constants (the extension exports them; a GPU test holds
// the two equal). docs/kernels.md "Forest inference".
//
// A packed forest is T trees, tree t = it * K + k adding to score column k,
// each renumbered breadth-first so that a node's children are adjacent:
//
//   nodes      [N]     ForestNode, 16 bytes, trees back to back
//   tree_first [T + 1] int32: first node of tree t, tree_first[T] == N
//   baseline   [K]     fp64
//
// A visit at node i of a tree whose root sits at `base` reads one
// ForestNode and the row's feature x = X[row][meta & 0xFFFF]:
//
//   left = base + ((meta >> 16) & 0x7FFF)
//   next = (x != x ? meta >> 31 : x <= thr) ? left : left + 1
//
// A LEAF points at itself: its left offset is its own index in the tree,
// thr = +inf and the missing-goes-left bit is set, so every x, NaN
// included, stays on it (next == i is the leaf test); `value` is the fp64
// the tree adds. An inner node's `value` is unused (0).
#pragma once

#include <hip/hip_runtime_api.h>

#include "forest_limits.h"

struct ForestNode {
  float thr;       // rd32(threshold): x <= t in fp64  <=>  x <= thr in fp32
  unsigned meta;   // feature 0..15 | left offset in the tree 16..30 | missing-left 31
  double value;
};
static_assert(sizeof(ForestNode) == 16, "one ds_read_b128 per visit");

// items (row, class) a thread may carry; a workgroup's R rows satisfy
// R * K <= FOREST_BLOCK * FOREST_MAX_ITEMS
constexpr int FOREST_MAX_ITEMS = 8;
constexpr int FOREST_MAX_ROWS = 2048;       // the most rows per workgroup

// The LDS carve, bytes from the base of dynamic LDS:
//   [0, 32768)        the chunk's nodes, FOREST_CHUNK_NODES of them; after
//                     the last chunk the workgroup's scores [R][K] fp64
//   [32768, 33792)    the chunk's tree table: FOREST_CHUNK_TREES root offsets
//   [33792, 34048)    the baseline, FOREST_MAX_CLASSES fp64
//   [34048, ...)      the row tile [R][F | 1] fp32, within FOREST_LDS_BUDGET
constexpr int FOREST_CHUNK_NODES = 2048;    // also the most nodes ONE tree may have
constexpr int FOREST_CHUNK_TREES = 256;     // one table entry per thread
constexpr int FOREST_LDS_TILE_OFF =
    FOREST_CHUNK_NODES * 16 + FOREST_CHUNK_TREES * 4 + FOREST_MAX_CLASSES * 8;
constexpr int FOREST_TILE_BYTES = FOREST_LDS_BUDGET - FOREST_LDS_TILE_OFF;

static_assert(FOREST_CHUNK_NODES % FOREST_BLOCK == 0 &&
                  FOREST_CHUNK_TREES == FOREST_BLOCK,
              "a thread prefetches CHUNK_NODES / BLOCK nodes and one table entry");
static_assert(FOREST_BLOCK * FOREST_MAX_ITEMS * 8 <= FOREST_CHUNK_NODES * 16,
              "the final scores reuse the node area");
static_assert(FOREST_CHUNK_NODES <= 1 << 15, "left offsets have 15 bits");
static_assert(FOREST_MIN_ROWS * (forest_row_stride(FOREST_MAX_FEATURES) * 4) <= FOREST_TILE_BYTES,
              "the widest row fits at the smallest R");
static_assert(FOREST_MAX_FEATURES <= 1 << 16, "a node's feature has 16 bits");

// Rows per workgroup for F features and K classes (forest_tile_rows): up to
// FOREST_MAX_ROWS, the tile within FOREST_TILE_BYTES and the R * K items
// within FOREST_BLOCK * FOREST_MAX_ITEMS.
constexpr int forest_rows_per_wg(int F, int K) {
  return forest_tile_rows(F, K, FOREST_MAX_ROWS, FOREST_TILE_BYTES,
                          FOREST_BLOCK * FOREST_MAX_ITEMS);
}
static_assert(forest_rows_per_wg(64, 10) == 128 && forest_rows_per_wg(64, 32) == 64 &&
                  forest_rows_per_wg(5, 1) == 2048 && forest_rows_per_wg(300, 3) == 32 &&
                  forest_rows_per_wg(2048, 1) == 4 && forest_rows_per_wg(2049, 1) == 0,
              "forest_rows_per_wg and ops/forest.py rows_per_wg disagree");

// Trees per chunk: as many whole trees as are certain to fit, given the
// largest tree of the forest, at most FOREST_CHUNK_TREES, and at most `cap`
// when cap > 0. 0: one tree alone overflows a chunk.
constexpr int forest_trees_per_chunk(int max_tree_nodes, int cap) {
  if (max_tree_nodes < 1 || max_tree_nodes > FOREST_CHUNK_NODES) return 0;
  int n = FOREST_CHUNK_NODES / max_tree_nodes;
  if (n > FOREST_CHUNK_TREES) n = FOREST_CHUNK_TREES;
  if (cap > 0 && cap < n) n = cap;
  return n;
}

extern "C" {

// scores[b][k] = ((baseline[k] + leaf(tree k, b)) + leaf(tree K + k, b)) + ...
// for b < B, one fp64 rounding per addition; labels[b] = the first column
// with the largest score, or score > 0 when K == 1. X [B][F] fp32, 16-byte
// aligned; nodes [n_nodes]; tree_first [T + 1]; max_tree_nodes the largest
// tree's node count (the chunking depends on it; a kernel given a smaller
// number than the truth computes wrong scores but reads and writes nothing
// out of bounds). 0 launched, -2 the dynamic-LDS attribute failed, -3
// arguments outside the kernel's range (tabular_launch.h's convention).
int launch_forest_predict(const float* X, int B, int F, int K,
                          const ForestNode* nodes, int n_nodes,
                          const int* tree_first, int T, int max_tree_nodes,
                          int trees_per_chunk, const double* baseline,
                          double* scores, int* labels, hipStream_t stream);

}  // extern "C"
