// CDNA4 (gfx950) inference of a bagged forest: random forests, extra-trees
// and single decision trees (docs/kernels.md "Bagged-forest inference"; node
// format and LDS carve: bagged_forest.h).
//
//   bagged_forest_predict_kernel<U>: for row b < B and class k < K
//       probs[b][k] = (((0 + v(tree 0, b)[k]) + v(tree 1, b)[k]) + ...) / T
//       labels[b]   = first k with the largest probs[b][k]
//
// v(t, b) being the fp64 K-vector on the leaf that row b reaches in tree t:
// one fp64 rounding per addition, in tree order, and one for the division,
// which are the bits of sklearn's predict_proba / predict at n_jobs=None.
//
// Only the SUM needs the tree order; the walks do not. So the kernel splits
// a chunk of C trees into two phases with different work items:
//
//   walk  items (row, tree of the chunk), row the fast index: an item walks
//         to its leaf and leaves the leaf's leaf_values row in LDS
//         leaf_idx[tree][row]. One row's trees are walked by many lanes at
//         once; a lone row is walked through up to 256 trees in parallel.
//   sum   items (row, class), class the fast index: an item owns one fp64
//         sum and adds leaf_values[leaf_idx[c][row]][class] for the chunk's
//         trees c in order. The loads are independent and issued eight
//         ahead; the additions are a chain.
//
// A workgroup owns R consecutive rows (R a power of two, chosen by the host
// from F and K) and all trees for them. It stages its rows once as fp32 in
// LDS (odd dword stride). C is the workgroup's own: with `rows` rows
// (rounded up to a power of two, RP) a chunk is min(2048 / RP, 256, T)
// trees, so a short last workgroup or a single-row request gets more trees
// at once instead of idle lanes.
//
// Bagged trees are grown out (hundreds to tens of thousands of nodes), so a
// tree does not fit LDS. Its first P breadth-first nodes do: the top levels,
// which every row passes through. The 2,048 prefix slots are dealt out
// evenly, PS = 2048 / C (a power of two) slots a tree, P = min(PS, the
// largest tree). A visit at local index i < P reads LDS, any other reads
// global memory with one 8-byte load (the forest stays in L2). The next
// chunk's prefixes are loaded into registers before the current chunk is
// walked and stored behind the barrier that ends the walk (issue_chunk /
// store_chunk); the tree table (first node and node count of each tree of a
// chunk) runs one chunk further ahead in a double buffer, so that the
// prefix loads do not wait on a table load.
//
// A thread keeps U walks in flight (a template parameter): every per-walk
// value is a named element of a fully unrolled array, i.e. a register, and
// the U dependent read chains (node -> feature -> next node) overlap.
//
// No atomics, no fences, no matrix instructions: the kernel reads only
// memory that no one writes during the launch, and writes probs and labels
// of rows < B. Every index derived from the forest's contents is clamped
// into its array.

#include <hip/hip_runtime.h>

#include "bagged_forest.h"
#include "forest_device.h"
#include "tabular_launch.h"

namespace {

constexpr int PRE = BAGGED_PREFIX_SLOTS / FOREST_BLOCK;   // prefetched nodes per thread
constexpr int AHEAD = 8;                                  // leaf-value loads in flight

typedef unsigned v2u __attribute__((ext_vector_type(2)));   // a BaggedNode as a native vector

// The next chunk's prefixes and the table of the chunk after it, on their
// way from memory to LDS, in registers.
struct ChunkRegs {
  v2u n0, n1, n2, n3, n4, n5, n6, n7;
  int first, count;
};
static_assert(PRE == 8, "ChunkRegs names eight nodes");

// Table entry of tree t: its first node, clamped into the node array, and
// its node count, clamped to what the array holds behind it and to the
// format's limit. Trees behind the forest read the last entry.
__device__ __forceinline__ void load_table(int& first, int& count,
                                           const int* __restrict__ tree_first, long long t,
                                           int T, int n_nodes) {
  const int a = tree_first[t < T ? (int)t : T - 1];
  const int b = tree_first[t < T ? (int)t + 1 : T];
  first = a < 0 ? 0 : (a > n_nodes - 1 ? n_nodes - 1 : a);
  int n = b - a;
  const int room = n_nodes - first;
  n = n > room ? room : n;
  n = n > BAGGED_MAX_TREE_NODES ? BAGGED_MAX_TREE_NODES : n;
  count = n < 1 ? 1 : n;
}

// Start the loads of a chunk's prefixes: slot e = tid + J * 256 belongs to
// tree e >> ps_shift of the chunk and holds its node e & (PS - 1). Nothing
// is predicated, so that all eight loads leave together ahead of the walk: a
// slot beyond its tree or beyond the chunk reads some node of the forest
// (store_chunk drops it). `tab_first` is the chunk's table in LDS.
__device__ __forceinline__ void issue_chunk(ChunkRegs& r, const v2u* __restrict__ nodes,
                                            const int* tab_first, int ps_shift,
                                            int n_nodes, int tid) {
  const int last = n_nodes - 1;
  const int ps_mask = (1 << ps_shift) - 1;
#define BAGGED_ISSUE(J, N)                                              \
  {                                                                     \
    const int e = tid + J * FOREST_BLOCK;                               \
    const int s = e >> ps_shift;                                        \
    const int p = tab_first[s < BAGGED_CHUNK_TREES ? s : BAGGED_CHUNK_TREES - 1] + (e & ps_mask); \
    r.N = nodes[p < last ? p : last];                                   \
  }
  FOREST_EACH_NODE(BAGGED_ISSUE)
#undef BAGGED_ISSUE
}

// ... and put them into LDS: node j of the chunk's tree s, if the chunk has
// a tree s, the tree a node j, and j < P. The caller's barriers stand before
// (the last reader of the previous chunk) and after.
__device__ __forceinline__ void store_chunk(const ChunkRegs& r, v2u* s_nodes,
                                            const int* tab_count, int ps_shift, int P,
                                            int nt, int tid) {
  const int ps_mask = (1 << ps_shift) - 1;
#define BAGGED_STORE(J, N)                                              \
  {                                                                     \
    const int e = tid + J * FOREST_BLOCK;                               \
    const int s = e >> ps_shift, j = e & ps_mask;                       \
    if (s < nt && j < P && j < tab_count[s]) s_nodes[e] = r.N;          \
  }
  FOREST_EACH_NODE(BAGGED_STORE)
#undef BAGGED_STORE
}

template <int U>
__global__ void __launch_bounds__(FOREST_BLOCK)
bagged_forest_predict_kernel(const float* __restrict__ X,             // [B][F]
                             const v2u* __restrict__ nodes,           // [n_nodes] BaggedNode
                             const int* __restrict__ tree_first,      // [T + 1]
                             const double* __restrict__ leaf_values,  // [n_leaves][K]
                             double* __restrict__ probs,              // [>= B][K]
                             int* __restrict__ labels,                // [>= B]
                             int B, int F, int K, int T, int n_nodes, int n_leaves,
                             int rshift,      // R = 1 << rshift
                             int p_cap,       // the most prefix nodes a tree (>= 0)
                             int c_cap,       // the most trees a chunk, 0: no cap
                             int f_magic,     // ceil(2^20 / F): t / F == (t * f_magic) >> 20, t < 256
                             int step_rows, int step_cols,   // 256 / F, 256 % F
                             int k_magic) {   // ceil(2^20 / K): i / K == (i * k_magic) >> 20, i < 2048
  extern __shared__ v2u lds[];
  char* lds_base = reinterpret_cast<char*>(lds);
  v2u* s_nodes = lds;
  double* s_acc = reinterpret_cast<double*>(lds_base + BAGGED_LDS_ACC_OFF);
  int* s_leaf = reinterpret_cast<int*>(lds_base + BAGGED_LDS_LEAF_OFF);
  int* s_tab = reinterpret_cast<int*>(lds_base + BAGGED_LDS_TAB_OFF);
  float* s_rows = reinterpret_cast<float*>(lds_base + BAGGED_LDS_TILE_OFF);
  // table buffer q: first nodes at s_tab + q * 512, node counts 256 further on
  auto tab_first = [&](int q) { return s_tab + (q & 1) * 2 * BAGGED_CHUNK_TREES; };
  auto tab_count = [&](int q) { return tab_first(q) + BAGGED_CHUNK_TREES; };

  const int tid = threadIdx.x;
  const int R = 1 << rshift;
  const int stride = forest_row_stride(F);
  const long long row0 = (long long)blockIdx.x << rshift;
  const int nrows = B - row0 < R ? (int)(B - row0) : R;

  // ---- the workgroup's chunking (uniform) --------------------------------------
  int rs = 0;                                   // RP = 1 << rs >= nrows
  while ((1 << rs) < nrows) ++rs;
  const int C = bagged_trees_per_chunk(nrows, T, c_cap);
  const int n_chunks = (T + C - 1) / C;
  const int ps_shift = 31 - __clz(BAGGED_PREFIX_SLOTS / C);   // PS = 2^ps_shift <= 2048 / C
  const int P = p_cap < (1 << ps_shift) ? p_cap : (1 << ps_shift);
  const int last_node = n_nodes - 1;

  // ---- tables of chunks 0 and 1, zeroed sums ------------------------------------
  {
    int f0, c0, f1, c1;
    load_table(f0, c0, tree_first, tid, T, n_nodes);
    load_table(f1, c1, tree_first, (long long)C + tid, T, n_nodes);
    tab_first(0)[tid] = f0;
    tab_count(0)[tid] = c0;
    tab_first(1)[tid] = f1;
    tab_count(1)[tid] = c1;
    for (int i = tid; i < BAGGED_MAX_ITEMS; i += FOREST_BLOCK) s_acc[i] = 0.0;
  }
  __syncthreads();

  ChunkRegs regs;
  issue_chunk(regs, nodes, tab_first(0), ps_shift, n_nodes, tid);

  // the row tile, while chunk 0 is in flight
  forest_stage_rows(s_rows, X, row0, nrows, F, stride, f_magic, step_rows, step_cols, tid);

  store_chunk(regs, s_nodes, tab_count(0), ps_shift, P, T < C ? T : C, tid);
  __syncthreads();

  const int n_sums = nrows * K;
  const int max_leaf = n_leaves - 1;

  for (int c = 0; c < n_chunks; ++c) {
    const int t0 = c * C;
    const int nt = T - t0 < C ? T - t0 : C;
    const int nt_next = T - t0 - C < C ? T - t0 - C : C;   // <= 0 behind the last chunk
    const int* tfirst = tab_first(c);
    const int* tcount = tab_count(c);
    // the next chunk's prefixes and the table of the chunk after it leave
    // now, unconditionally (behind the forest they re-read its last entries
    // and are dropped)
    issue_chunk(regs, nodes, tab_first(c + 1), ps_shift, n_nodes, tid);
    load_table(regs.first, regs.count, tree_first, (long long)t0 + 2 * C + tid, T, n_nodes);

    // ---- walk: items (row, tree of the chunk), U of a thread at a time ---------
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
        base[u] = tfirst[tcl];
        cnt[u] = tcount[tcl];
        slot[u] = tcl << ps_shift;
        rowb[u] = (row < nrows ? row : 0) * stride;
        idx[u] = 0;
        leaf[u] = 0;
        todo[u] = live[u];
        busy |= todo[u];
      }
      // an inner node's children lie behind it, so idx grows with every
      // step and stays below cnt <= 2^20: the loop ends on any input
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
        const int l = leaf[u] < 0 ? 0 : (leaf[u] > max_leaf ? max_leaf : leaf[u]);
        if (live[u]) s_leaf[j] = l;   // j == tc * RP + row
      }
    }

    __syncthreads();   // the chunk's last walker; leaf_idx is complete

    // ---- sum: items (row, class), the chunk's trees in order ------------------
    for (int i = tid; i < n_sums; i += FOREST_BLOCK) {
      const int row = (int)(((unsigned)i * (unsigned)k_magic) >> 20);
      const int k = i - row * K;
      double acc = s_acc[i];
      for (int c0 = 0; c0 < nt; c0 += AHEAD) {
        double v[AHEAD];
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) {
          const int tc = c0 + q < nt ? c0 + q : nt - 1;
          const int l = s_leaf[(tc << rs) + row];
          v[q] = leaf_values[(size_t)l * (size_t)K + (size_t)k];
        }
#pragma unroll
        for (int q = 0; q < AHEAD; ++q) acc = c0 + q < nt ? acc + v[q] : acc;
      }
      s_acc[i] = acc;
    }

    // the walk is over: the next chunk's prefixes replace this one's, and
    // the table after next this chunk's
    if (nt_next > 0)
      store_chunk(regs, s_nodes, tab_count(c + 1), ps_shift, P, nt_next, tid);
    tab_first(c)[tid] = regs.first;
    tab_count(c)[tid] = regs.count;
    __syncthreads();
  }

  // ---- the mean, contiguous stores, and one lane a row for the label ----------
  const double trees = (double)T;
  double* __restrict__ out = probs + (size_t)row0 * (size_t)K;
  for (int i = tid; i < n_sums; i += FOREST_BLOCK) {
    const double p = s_acc[i] / trees;
    s_acc[i] = p;
    out[i] = p;
  }
  __syncthreads();
  for (int r = tid; r < nrows; r += FOREST_BLOCK)
    labels[row0 + r] = forest_first_largest(s_acc + r * K, K);
}

template <int U>
int launch_walks(const float* X, int B, int F, int K, const BaggedNode* nodes, int n_nodes,
                 const int* tree_first, int T, const double* leaf_values, int n_leaves,
                 int p_cap, int c_cap, double* probs, int* labels,
                 const ForestTileLaunch& g, hipStream_t stream) {
  if (ensure_dynamic_lds<bagged_forest_predict_kernel<U>>(FOREST_LDS_BUDGET) != 0) return -2;
  hipLaunchKernelGGL(bagged_forest_predict_kernel<U>, dim3(g.blocks), dim3(FOREST_BLOCK),
                     BAGGED_LDS_TILE_OFF + g.tile_bytes, stream, X,
                     reinterpret_cast<const v2u*>(nodes), tree_first, leaf_values, probs,
                     labels, B, F, K, T, n_nodes, n_leaves, g.rshift, p_cap, c_cap,
                     g.f_magic, g.step_rows, g.step_cols, ((1 << 20) + K - 1) / K);
  return 0;
}

}  // namespace

extern "C" {

int launch_bagged_forest_predict(const float* X, int B, int F, int K,
                                 const BaggedNode* nodes, int n_nodes,
                                 const int* tree_first, int T, int max_tree_nodes,
                                 const double* leaf_values, int n_leaves,
                                 int prefix_nodes, int trees_per_chunk,
                                 double* probs, int* labels, hipStream_t stream) {
  const int R = bagged_rows_per_wg(F, K);
  if (B < 1 || R == 0 || trees_per_chunk < 0 || T < 1 || T > (1 << 30) || n_nodes < T ||
      n_nodes > (1 << 30) || n_leaves < 1 || n_leaves > n_nodes || max_tree_nodes < 1 ||
      max_tree_nodes > BAGGED_MAX_TREE_NODES)
    return -3;
  const ForestTileLaunch g = forest_tile_launch(B, F, R);
  int p_cap = max_tree_nodes < BAGGED_PREFIX_SLOTS ? max_tree_nodes : BAGGED_PREFIX_SLOTS;
  if (prefix_nodes >= 0 && prefix_nodes < p_cap) p_cap = prefix_nodes;
  // walks a thread has in a chunk of the fullest workgroup: U of them in flight
  const int rows = B < R ? B : R;
  int rp = 1;
  while (rp < rows) rp <<= 1;
  const int walks = (rp * bagged_trees_per_chunk(rows, T, trees_per_chunk) + FOREST_BLOCK - 1) /
                    FOREST_BLOCK;
#define BAGGED_LAUNCH(U)                                                              \
  return launch_walks<U>(X, B, F, K, nodes, n_nodes, tree_first, T, leaf_values,      \
                         n_leaves, p_cap, trees_per_chunk, probs, labels, g, stream)
  if (walks >= 4) BAGGED_LAUNCH(4);   // eight in flight measured no faster (docs)
  if (walks >= 2) BAGGED_LAUNCH(2);
  BAGGED_LAUNCH(1);
#undef BAGGED_LAUNCH
}

}  // extern "C"
