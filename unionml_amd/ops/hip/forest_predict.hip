// CDNA4 (gfx950) inference of a gradient-boosted forest
// (docs/kernels.md "Forest inference"; node format and LDS carve: forest.h).
//
//   forest_predict_kernel<U>: for row b < B and class k < K
//       scores[b][k] = ((baseline[k] + leaf(tree k, b)) + leaf(tree K + k, b)) + ...
//       labels[b]    = first k with the largest score       (K == 1: score > 0)
//
// one fp64 rounding per addition, in iteration order: the bits of sklearn's
// predictor. Nothing here is a matrix product; the work is a chain of
// dependent 16-byte reads and compares over a read-only structure, so the
// kernel lives in LDS and the vector ALU.
//
// A workgroup owns R consecutive rows (R a power of two, chosen by the host
// from F and K) and ALL trees for them: splitting a row's trees over
// workgroups would reorder its fp64 sum. It stages its rows once as fp32 in
// LDS (odd dword stride) and walks the forest chunk by chunk, a chunk being
// `tpc` whole trees copied into LDS with coalesced 16-byte loads. The next
// chunk's loads are issued into registers before the current chunk is
// walked and stored behind the barrier that ends the walk (issue_chunk /
// store_chunk), its two boundary offsets one chunk earlier still.
//
// The unit of work is an item (row, class): the K trees of an iteration are
// independent, each adds to its own column. Item j = u * 256 + thread,
// row = j % R, class = j / R, so with R >= 64 a wave walks ONE tree for 64
// rows (root reads are broadcasts). A thread carries U = ceil(R * K / 256)
// items, U in 1..8 a template parameter: every per-item value is a named
// element of a fully unrolled array, i.e. a register, and the U dependent
// read chains (node -> feature -> next node) of a thread overlap.
//
// The walk is a per-lane loop with NO per-tree structure: an item that
// reaches a leaf (a node that points at itself) adds the leaf's value and
// jumps to the root of its next tree, K trees on, in the same step; the
// root's offset was read from the chunk's table alongside the node, so the
// jump costs no extra round trip. An item is done with the chunk when its
// next tree lies beyond it (the boundary may fall inside an iteration: the
// item's tree counter and score simply live on into the next chunk). The
// loop ends when the thread's items are all done. An inner node's child
// index is larger than its own, so an item visits a node at most once per
// chunk; the trip count is capped by the chunk's node count all the same,
// which only a malformed forest reaches.
//
// No atomics, no fences, no scratch: the kernel reads only memory that no
// one writes during the launch, and writes scores and labels of rows < B.

#include <hip/hip_runtime.h>

#include "forest.h"
#include "forest_device.h"
#include "tabular_launch.h"

namespace {

constexpr int PRE = FOREST_CHUNK_NODES / FOREST_BLOCK;   // prefetched nodes per thread

// The next chunk on its way from memory to LDS, in registers. The nodes are
// a native vector type: HIP's uint4 is a struct, its assignment from global
// memory and to LDS a memcpy between address spaces, and with those the
// compiler kept the whole of ChunkRegs in scratch (144 bytes per lane).
typedef unsigned v4u __attribute__((ext_vector_type(4)));
struct ChunkRegs {
  v4u n0, n1, n2, n3, n4, n5, n6, n7;
  int root;
};
static_assert(PRE == 8, "ChunkRegs names eight nodes");

// Start the loads of a chunk: `cnt` nodes from nodes[first] and the first
// nodes of its trees, trees t0 .. t0 + 256. Nothing is waited for and
// nothing is predicated, so that all nine loads leave together ahead of the
// walk: a piece beyond the chunk re-reads the forest's last node, an entry
// beyond the table its last one (store_chunk drops both).
__device__ __forceinline__ void issue_chunk(ChunkRegs& r, const uint4* __restrict__ nodes,
                                            const int* __restrict__ tree_first,
                                            int first, int n_nodes, int t0, int T,
                                            int tid) {
  const v4u* __restrict__ src = reinterpret_cast<const v4u*>(nodes);
  const int last = n_nodes - 1;
#define FOREST_ISSUE(J, N)                              \
  {                                                     \
    const int p = first + tid + J * FOREST_BLOCK;       \
    r.N = src[p < last ? p : last];                     \
  }
  FOREST_EACH_NODE(FOREST_ISSUE)
#undef FOREST_ISSUE
  const int t = t0 + tid;
  r.root = tree_first[t < T ? t : T];
}

// ... and put them into LDS, the roots as offsets within the chunk. The
// caller's barriers stand before (the last reader of the previous chunk)
// and after.
__device__ __forceinline__ void store_chunk(const ChunkRegs& r, uint4* s_nodes, int* s_tab,
                                            int first, int cnt, int nt, int tid) {
  v4u* dst = reinterpret_cast<v4u*>(s_nodes) + tid;
#define FOREST_STORE(J, N) \
  if (tid + J * FOREST_BLOCK < cnt) dst[J * FOREST_BLOCK] = r.N;
  FOREST_EACH_NODE(FOREST_STORE)
#undef FOREST_STORE
  if (tid < nt) s_tab[tid] = r.root - first;
}

template <int U>
__global__ void __launch_bounds__(FOREST_BLOCK)
forest_predict_kernel(const float* __restrict__ X,            // [B][F]
                      const uint4* __restrict__ nodes,        // [n_nodes] ForestNode
                      const int* __restrict__ tree_first,     // [T + 1]
                      const double* __restrict__ baseline,    // [K]
                      double* __restrict__ scores,            // [>= B][K]
                      int* __restrict__ labels,               // [>= B]
                      int B, int F, int K, int T, int n_nodes, int tpc, int n_chunks,
                      int rshift,    // R = 1 << rshift
                      int f_magic,   // ceil(2^20 / F): t / F == (t * f_magic) >> 20, t < 256
                      int step_rows, int step_cols) {  // 256 / F, 256 % F
  extern __shared__ uint4 lds[];
  uint4* s_nodes = lds;
  int* s_tab = reinterpret_cast<int*>(lds + FOREST_CHUNK_NODES);
  double* s_base = reinterpret_cast<double*>(s_tab + FOREST_CHUNK_TREES);
  float* s_rows = reinterpret_cast<float*>(reinterpret_cast<char*>(lds) +
                                           FOREST_LDS_TILE_OFF);
  const int tid = threadIdx.x;
  const int R = 1 << rshift;
  const int stride = forest_row_stride(F);
  const long long row0 = (long long)blockIdx.x << rshift;
  const int nrows = B - row0 < R ? (int)(B - row0) : R;

  // boundary c: the first node of chunk c, clamped into the node array so
  // that a malformed table cannot send a load outside it
  auto boundary = [&](int c) {
    const long long t = (long long)c * tpc;
    const int b = tree_first[t < T ? (int)t : T];
    return b < 0 ? 0 : (b > n_nodes ? n_nodes : b);
  };
  auto count = [&](int lo, int hi) {
    const int n = hi - lo;
    return n < 0 ? 0 : (n > FOREST_CHUNK_NODES ? FOREST_CHUNK_NODES : n);
  };
  auto trees_in = [&](int c) {
    const int left = T - c * tpc;
    return left < tpc ? left : tpc;
  };
  int b0 = boundary(0), b1 = boundary(1), b2 = boundary(2);

  ChunkRegs regs;
  int cnt = count(b0, b1), nt = trees_in(0);
  issue_chunk(regs, nodes, tree_first, b0, n_nodes, 0, T, tid);
  // the baseline reaches the items through LDS: loaded into their registers
  // directly it stayed a pending memory load by the compiler's count, and
  // the first leaf of every chunk waited for the NEXT chunk's loads
  if (tid < K) s_base[tid] = baseline[tid];

  // the row tile, while chunk 0 is in flight
  forest_stage_rows(s_rows, X, row0, nrows, F, stride, f_magic, step_rows, step_cols, tid);

  store_chunk(regs, s_nodes, s_tab, b0, cnt, nt, tid);
  __syncthreads();

  // ---- the thread's items -------------------------------------------------------
  double acc[U];   // the running score
  int tcur[U];     // the item's next tree; INT_MAX: no item, or a row >= B
  int rowb[U];     // its row's first dword in the tile
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * FOREST_BLOCK + tid;
    const int row = j & (R - 1), k = j >> rshift;
    const bool live = k < K && row < nrows;
    acc[u] = s_base[k < K ? k : 0];
    tcur[u] = live ? k : INT_MAX;
    rowb[u] = row * stride;
  }

  for (int c = 0; c < n_chunks; ++c) {
    const int t0 = c * tpc, t1 = t0 + nt;
    const int walk_cap = cnt;
    const bool more = c + 1 < n_chunks;
    // boundary c + 3 is asked for now and first used one chunk on; the next
    // chunk's loads leave unconditionally (behind the last chunk they
    // re-read the forest's last node and are dropped)
    const int b3 = boundary(c + 3);
    const int cnt_next = more ? count(b1, b2) : 0;
    const int nt_next = more ? trees_in(c + 1) : 0;
    issue_chunk(regs, nodes, tree_first, b1, n_nodes, t0 + tpc, T, tid);

    // ---- walk chunk c ---------------------------------------------------------
    int base[U], idx[U];
    bool busy = false;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const bool todo = tcur[u] < t1;
      base[u] = todo ? s_tab[tcur[u] - t0] : 0;
      idx[u] = base[u];
      busy |= todo;
    }
    for (int steps = 0; busy && steps <= walk_cap; ++steps) {
      uint4 nd[U];
      int jump[U];
      float x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        nd[u] = s_nodes[idx[u]];
        // the root of the item's next tree, or of the chunk's last one
        const int tn = tcur[u] < t1 - K ? tcur[u] + K : t1 - 1;
        jump[u] = s_tab[tn - t0];
      }
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = s_rows[rowb[u] + (int)(nd[u].y & 0xFFFFu)];
      busy = false;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const float thr = __uint_as_float(nd[u].x);
        const unsigned meta = nd[u].y;
        const bool go_left = (x[u] != x[u]) ? (meta >> 31) != 0 : x[u] <= thr;
        const int next = base[u] + (int)((meta >> 16) & 0x7FFFu) + (go_left ? 0 : 1);
        const bool take = next == idx[u] && tcur[u] < t1;   // on a leaf, not done
        const double v = __hiloint2double((int)nd[u].w, (int)nd[u].z);
        acc[u] = take ? acc[u] + v : acc[u];
        tcur[u] = take ? tcur[u] + K : tcur[u];
        base[u] = take ? jump[u] : base[u];
        idx[u] = take ? jump[u] : next;
        busy |= tcur[u] < t1;
      }
    }

    __syncthreads();   // the chunk's last reader
    if (more) {
      store_chunk(regs, s_nodes, s_tab, b1, cnt_next, nt_next, tid);
      __syncthreads();
    }
    cnt = cnt_next;
    nt = nt_next;
    b1 = b2;
    b2 = b3;
  }

  // ---- scores through LDS: coalesced stores, and a row's K together ------------
  // (the node area is free: the loop's last barrier stands behind its last
  // reader)
  double* s_sc = reinterpret_cast<double*>(s_nodes);
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = u * FOREST_BLOCK + tid;
    const int row = j & (R - 1), k = j >> rshift;
    if (k < K) s_sc[row * K + k] = acc[u];
  }
  __syncthreads();
  const int n_out = nrows * K;
  double* __restrict__ out = scores + (size_t)row0 * (size_t)K;
  for (int i = tid; i < n_out; i += FOREST_BLOCK) out[i] = s_sc[i];
  for (int r = tid; r < nrows; r += FOREST_BLOCK) {
    const double* s = s_sc + r * K;
    labels[row0 + r] = K == 1 ? (s[0] > 0.0 ? 1 : 0) : forest_first_largest(s, K);
  }
}

template <int U>
int launch_items(const float* X, int B, int F, int K, const ForestNode* nodes,
                 int n_nodes, const int* tree_first, int T, int tpc,
                 const double* baseline, double* scores, int* labels,
                 const ForestTileLaunch& g, hipStream_t stream) {
  if (ensure_dynamic_lds<forest_predict_kernel<U>>(FOREST_LDS_BUDGET) != 0) return -2;
  const int n_chunks = (T + tpc - 1) / tpc;
  hipLaunchKernelGGL(forest_predict_kernel<U>, dim3(g.blocks), dim3(FOREST_BLOCK),
                     FOREST_LDS_TILE_OFF + g.tile_bytes, stream, X,
                     reinterpret_cast<const uint4*>(nodes), tree_first, baseline,
                     scores, labels, B, F, K, T, n_nodes, tpc, n_chunks, g.rshift,
                     g.f_magic, g.step_rows, g.step_cols);
  return 0;
}

}  // namespace

extern "C" {

int launch_forest_predict(const float* X, int B, int F, int K,
                          const ForestNode* nodes, int n_nodes,
                          const int* tree_first, int T, int max_tree_nodes,
                          int trees_per_chunk, const double* baseline,
                          double* scores, int* labels, hipStream_t stream) {
  const int R = forest_rows_per_wg(F, K);
  const int tpc = forest_trees_per_chunk(max_tree_nodes, trees_per_chunk);
  if (B < 1 || R == 0 || tpc == 0 || trees_per_chunk < 0 || n_nodes < 1 || T < 1 ||
      T > (1 << 30) || T % K != 0 || n_nodes < T || n_nodes > (1 << 30))
    return -3;
  const ForestTileLaunch g = forest_tile_launch(B, F, R);
  const int items = (R * K + FOREST_BLOCK - 1) / FOREST_BLOCK;
  switch (items) {
#define FOREST_CASE(U)                                                            \
  case U:                                                                         \
    return launch_items<U>(X, B, F, K, nodes, n_nodes, tree_first, T, tpc,        \
                           baseline, scores, labels, g, stream);
    FOREST_CASE(1) FOREST_CASE(2) FOREST_CASE(3) FOREST_CASE(4)
    FOREST_CASE(5) FOREST_CASE(6) FOREST_CASE(7) FOREST_CASE(8)
#undef FOREST_CASE
  }
  return -3;
}

}  // extern "C"
