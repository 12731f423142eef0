// CDNA4 (gfx950) inference of a gradient-boosted forest as (row, tree) walks
// spread over the whole device, followed by an ordered fp64 sum
// (docs/kernels.md "Split walk"; packed format, LDS carve and launcher rule:
// forest_split.h).
//
//   forest_split_walk_kernel<U>: for row b < B and tree t < T
//       leaf_rows[t][b] = the leaf_values row of the leaf that row b reaches in tree t
//   forest_split_sum_kernel: for row b < B and class k < K
//       scores[b][k] = (((0 + baseline[k]) + v[leaf_rows[k][b]]) + v[leaf_rows[K + k][b]]) + ...
//       labels[b]    = first k with the largest score       (K == 1: score > 0)
//
// one fp64 rounding per addition, in iteration order: the bits of sklearn's
// predictor, as forest_predict_kernel gives them. That kernel hands a row's
// trees to ONE workgroup, which makes a small batch one serial chain over all
// iterations and asks for a whole tree in an LDS chunk. Only the sum needs
// the order, so here the walks are items of their own:
//
//   walk  grid (row tiles, tree slices). A workgroup owns R consecutive rows
//         (R a power of two: the batch rounded up, at most what the tile
//         budget allows) and S consecutive trees, R * S about 1,024. It
//         stages its rows once as fp32 in LDS (odd dword stride), a table of
//         its trees (first node, node count) and the first P breadth-first
//         nodes of each of them: one slice, one set of loads, no chunk loop
//         and no double buffer. Items are j = tree * RP + row, the row the
//         fast lane index (top nodes are broadcasts, tile reads hit distinct
//         banks). A visit at local index < P is a ds_read_b64, any other one
//         8-byte global load, so a tree may have 2^20 nodes. A thread keeps U
//         walks in flight as fully unrolled register arrays. The walk itself
//         is the bagged kernel's (bagged_forest_predict.hip): the two are
//         kept apart so that kernel's code does not move.
//   sum   a workgroup owns pow2floor(256 / K) rows, item (row, class) with the
//         row the fast lane index, so a wave reads consecutive words of
//         leaf_rows. The index and value loads do not depend on the chain and
//         run eight iterations ahead of it. The scores pass through LDS as
//         [row][K] and leave as contiguous stores; one lane a row takes the
//         label.
//
// No atomics, no fences, no cross-workgroup hand-off: the stream orders the
// two launches. Every index derived from the forest's contents (node,
// feature, a tree's extent, leaf row) is clamped into its array.

#include <hip/hip_runtime.h>

#include "forest_device.h"
#include "forest_split.h"
#include "tabular_launch.h"

namespace {

constexpr int PRE = 8;                  // prefix loads a thread has in flight
constexpr int AHEAD = SPLIT_SUM_AHEAD;

typedef unsigned v2u __attribute__((ext_vector_type(2)));   // a BaggedNode as a native vector

template <int U>
__global__ void __launch_bounds__(FOREST_BLOCK)
forest_split_walk_kernel(const float* __restrict__ X,          // [B][F]
                         const v2u* __restrict__ nodes,        // [n_nodes] BaggedNode
                         const int* __restrict__ tree_first,   // [T + 1]
                         int* __restrict__ leaf_rows,          // [T][B]
                         int B, int F, int T, int n_nodes, int n_leaves,
                         int rshift,      // R = 1 << rshift
                         int S,           // trees a slice, 1..256
                         int p_cap,       // the most prefix nodes a tree (>= 0)
                         int f_magic,     // ceil(2^20 / F): t / F == (t * f_magic) >> 20, t < 256
                         int step_rows, int step_cols) {   // 256 / F, 256 % F
  extern __shared__ v2u lds[];
  char* lds_base = reinterpret_cast<char*>(lds);
  v2u* s_nodes = lds;
  int* s_first = reinterpret_cast<int*>(lds_base + SPLIT_LDS_TAB_OFF);
  int* s_count = s_first + SPLIT_SLICE_TREES;
  float* s_rows = reinterpret_cast<float*>(lds_base + SPLIT_LDS_TILE_OFF);

  const int tid = threadIdx.x;
  const int R = 1 << rshift;
  const int stride = forest_row_stride(F);
  const long long row0 = (long long)blockIdx.x << rshift;
  const int nrows = B - row0 < R ? (int)(B - row0) : R;
  const int t0 = (int)blockIdx.y * S;
  const int nt = T - t0 < S ? T - t0 : S;
  const int last_node = n_nodes - 1;

  int rs = 0;                                   // RP = 1 << rs >= nrows
  while ((1 << rs) < nrows) ++rs;
  // P nodes of each tree in LDS, tree s of the slice at slots [s << pe, ...)
  const int ps = SPLIT_PREFIX_SLOTS / S;        // >= 16
  const int ps_floor = 1 << (31 - __clz(ps));
  const int P = p_cap < ps_floor ? p_cap : ps_floor;
  int pe = 0;                                   // 1 << pe >= P, <= ps_floor
  while ((1 << pe) < P) ++pe;

  // ---- the slice's tree table: first node clamped into the node array, node
  // count clamped to what the array holds behind it and to the format's
  // limit; entries behind the forest repeat its last tree -------------------------
  {
    const long long t = (long long)t0 + tid;
    const int a = tree_first[t < T ? (int)t : T - 1];
    const int b = tree_first[t < T ? (int)t + 1 : T];
    const int first = a < 0 ? 0 : (a > last_node ? last_node : a);
    int n = b - a;
    const int room = n_nodes - first;
    n = n > room ? room : n;
    n = n > BAGGED_MAX_TREE_NODES ? BAGGED_MAX_TREE_NODES : n;
    s_first[tid] = first;
    s_count[tid] = n < 1 ? 1 : n;
  }
  __syncthreads();

  // ---- the prefixes: slot e = tid + q * 256 holds node e & (2^pe - 1) of tree
  // e >> pe. The loads of a round are unconditional and clamped (a slot beyond
  // its tree or beyond the slice reads some node of the forest), the stores
  // predicated -----------------------------------------------------------------------
  const int n_slots = P > 0 ? nt << pe : 0;     // <= SPLIT_PREFIX_SLOTS
  const int pe_mask = (1 << pe) - 1;
  for (int e0 = 0; e0 < n_slots; e0 += PRE * FOREST_BLOCK) {
    v2u nd[PRE];
#pragma unroll
    for (int q = 0; q < PRE; ++q) {
      const int e = e0 + q * FOREST_BLOCK + tid;
      const int s = e >> pe;
      const int p = s_first[s < SPLIT_SLICE_TREES ? s : SPLIT_SLICE_TREES - 1] + (e & pe_mask);
      nd[q] = nodes[p < last_node ? p : last_node];
    }
#pragma unroll
    for (int q = 0; q < PRE; ++q) {
      const int e = e0 + q * FOREST_BLOCK + tid;
      const int s = e >> pe, j = e & pe_mask;
      if (s < nt && j < P && j < s_count[s]) s_nodes[e] = nd[q];   // e < n_slots
    }
  }

  forest_stage_rows(s_rows, X, row0, nrows, F, stride, f_magic, step_rows, step_cols, tid);
  __syncthreads();

  // ---- walk: items (row, tree of the slice), U of a thread at a time -------------
  const int max_leaf = n_leaves - 1;
  const int n_walks = nt << rs;
  for (int j0 = 0; j0 < n_walks; j0 += U * FOREST_BLOCK) {
    int base[U], cnt[U], slot[U], idx[U], rowb[U], leaf[U];
    bool live[U], todo[U];
    bool busy = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * FOREST_BLOCK + tid;
      const int row = j & ((1 << rs) - 1), tc = j >> rs;
      live[u] = tc < nt && row < nrows;
      const int tcl = tc < nt ? tc : nt - 1;
      base[u] = s_first[tcl];
      cnt[u] = s_count[tcl];
      slot[u] = tcl << pe;
      rowb[u] = (row < nrows ? row : 0) * stride;
      idx[u] = 0;
      leaf[u] = 0;
      todo[u] = live[u];
      busy |= todo[u];
    }
    // an inner node's children lie behind it, so idx grows with every step
    // and stays below cnt <= 2^20: the loop ends on any input
    while (busy) {
      v2u nd[U];
      float x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        nd[u] = v2u{0u, 0u};
        if (todo[u]) {
          if (idx[u] < P) {
            nd[u] = s_nodes[slot[u] + idx[u]];
          } else {
            const int g = base[u] + idx[u];
            nd[u] = nodes[g < last_node ? g : last_node];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int f = (int)(nd[u].y & 0x7FFu);
        x[u] = s_rows[rowb[u] + (f < F ? f : F - 1)];
      }
      busy = false;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float thr = __uint_as_float(nd[u].x);
        const unsigned meta = nd[u].y;
        const int dist = (int)(meta >> BAGGED_META_DIST_SHIFT);
        const bool go_left =
            (x[u] != x[u]) ? (meta & BAGGED_META_MISSING_LEFT) != 0 : x[u] <= thr;
        const int next = idx[u] + dist + (go_left ? 0 : 1);
        // a leaf, or (a malformed tree) a child behind the tree's end
        const bool stop = dist == 0 || next >= cnt[u];
        leaf[u] = (todo[u] && stop) ? (int)nd[u].x : leaf[u];
        idx[u] = (todo[u] && !stop) ? next : idx[u];
        todo[u] = todo[u] && !stop;
        busy |= todo[u];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = j0 + u * FOREST_BLOCK + tid;
      const int row = j & ((1 << rs) - 1), tc = j >> rs;
      const int l = leaf[u] < 0 ? 0 : (leaf[u] > max_leaf ? max_leaf : leaf[u]);
      // consecutive lanes, consecutive words; nothing for a row >= B
      if (live[u]) leaf_rows[(size_t)(t0 + tc) * (size_t)B + (size_t)(row0 + row)] = l;
    }
  }
}

// The ordered combine: one (row, class) item a thread, i = class * rows + row.
__global__ void __launch_bounds__(FOREST_BLOCK)
forest_split_sum_kernel(const int* __restrict__ leaf_rows,        // [T][B]
                        const double* __restrict__ leaf_values,   // [n_leaves]
                        const double* __restrict__ baseline,      // [K]
                        double* __restrict__ scores,              // [>= B][K]
                        int* __restrict__ labels,                 // [>= B]
                        int B, int K, int n_iter,                 // T == n_iter * K
                        int n_leaves,
                        int rows_shift) {   // rows = 1 << rows_shift = pow2floor(256 / K)
  __shared__ double s_sc[FOREST_BLOCK];
  const int tid = threadIdx.x;
  const int rows = 1 << rows_shift;
  const int r = tid & (rows - 1), k = tid >> rows_shift;
  const long long row0 = (long long)blockIdx.x << rows_shift;
  const int nrows = B - row0 < rows ? (int)(B - row0) : rows;
  // a thread without an item reads what a neighbour reads and stores nothing
  const int kc = k < K ? k : K - 1;
  const int* __restrict__ src =
      leaf_rows + (size_t)kc * (size_t)B + (size_t)(row0 + (r < nrows ? r : 0));
  const size_t step = (size_t)K * (size_t)B;   // one iteration on
  const int max_leaf = n_leaves - 1;
  const int last_it = n_iter - 1;

  double acc = 0.0 + baseline[kc];              // sklearn starts from zeros + baseline
  int l[AHEAD];
#pragma unroll
  for (int q = 0; q < AHEAD; ++q) l[q] = src[(size_t)(q < last_it ? q : last_it) * step];
  for (int it0 = 0; it0 < n_iter; it0 += AHEAD) {
    double v[AHEAD];
#pragma unroll
    for (int q = 0; q < AHEAD; ++q)
      v[q] = leaf_values[l[q] < 0 ? 0 : (l[q] > max_leaf ? max_leaf : l[q])];
    // the next round's indices leave behind this round's values and ahead of
    // its additions
#pragma unroll
    for (int q = 0; q < AHEAD; ++q) {
      const int it = it0 + AHEAD + q;
      l[q] = src[(size_t)(it < last_it ? it : last_it) * step];
    }
#pragma unroll
    for (int q = 0; q < AHEAD; ++q) acc = it0 + q < n_iter ? acc + v[q] : acc;
  }

  if (k < K) s_sc[r * K + k] = acc;
  __syncthreads();
  if (tid < nrows * K) scores[(size_t)row0 * (size_t)K + (size_t)tid] = s_sc[tid];
  if (tid < nrows) {
    const double* s = s_sc + tid * K;
    labels[row0 + tid] = K == 1 ? (s[0] > 0.0 ? 1 : 0) : forest_first_largest(s, K);
  }
}

template <int U>
int launch_walks(const float* X, int B, int F, const BaggedNode* nodes, int n_nodes,
                 const int* tree_first, int T, int n_leaves, int S, int p_cap,
                 int* leaf_rows, const ForestTileLaunch& g, hipStream_t stream) {
  if (ensure_dynamic_lds<forest_split_walk_kernel<U>>(FOREST_LDS_BUDGET) != 0) return -2;
  hipLaunchKernelGGL(forest_split_walk_kernel<U>, dim3(g.blocks, (unsigned)((T + S - 1) / S)),
                     dim3(FOREST_BLOCK), SPLIT_LDS_TILE_OFF + g.tile_bytes, stream, X,
                     reinterpret_cast<const v2u*>(nodes), tree_first, leaf_rows, B, F, T,
                     n_nodes, n_leaves, g.rshift, S, p_cap, g.f_magic, g.step_rows,
                     g.step_cols);
  return 0;
}

}  // namespace

extern "C" {

int launch_forest_split_predict(const float* X, int B, int F, int K,
                                const BaggedNode* nodes, int n_nodes,
                                const int* tree_first, int T, int max_tree_nodes,
                                const double* leaf_values, int n_leaves,
                                const double* baseline, int prefix_nodes,
                                int trees_per_slice, int* leaf_rows,
                                double* scores, int* labels, hipStream_t stream) {
  const int tile_rows = forest_split_rows_per_wg(F);
  if (B < 1 || tile_rows == 0 || K < 1 || K > FOREST_MAX_CLASSES || trees_per_slice < 0 ||
      T < 1 || T > (1 << 30) || T % K != 0 || n_nodes < T || n_nodes > (1 << 30) ||
      n_leaves < 1 || n_leaves > n_nodes || max_tree_nodes < 1 ||
      max_tree_nodes > BAGGED_MAX_TREE_NODES)
    return -3;
  int R = 1;                                    // min(pow2ceil(B), the tile's rows)
  while (R < B && R < tile_rows) R <<= 1;
  const int S = forest_split_trees_per_slice(R, T, trees_per_slice);
  if ((T + S - 1) / S > 65535) return -3;       // the grid's second dimension
  const ForestTileLaunch g = forest_tile_launch(B, F, R);
  int p_cap = max_tree_nodes < SPLIT_PREFIX_SLOTS ? max_tree_nodes : SPLIT_PREFIX_SLOTS;
  if (prefix_nodes >= 0 && prefix_nodes < p_cap) p_cap = prefix_nodes;
  // walks a thread of the fullest workgroup has: U of them in flight
  const int walks = (R * S + FOREST_BLOCK - 1) / FOREST_BLOCK;
  int rc;
#define SPLIT_LAUNCH(U)                                                                   \
  rc = launch_walks<U>(X, B, F, nodes, n_nodes, tree_first, T, n_leaves, S, p_cap,        \
                       leaf_rows, g, stream)
  if (walks >= 4) SPLIT_LAUNCH(4);
  else if (walks >= 2) SPLIT_LAUNCH(2);
  else SPLIT_LAUNCH(1);
#undef SPLIT_LAUNCH
  if (rc != 0) return rc;

  const int rows = forest_split_sum_rows(K);
  int rows_shift = 0;
  while ((1 << rows_shift) < rows) ++rows_shift;
  hipLaunchKernelGGL(forest_split_sum_kernel,
                     dim3((unsigned)(((long long)B + rows - 1) >> rows_shift)),
                     dim3(FOREST_BLOCK), 0, stream, leaf_rows, leaf_values, baseline, scores,
                     labels, B, K, T / K, n_leaves, rows_shift);
  return 0;
}

}  // extern "C"
