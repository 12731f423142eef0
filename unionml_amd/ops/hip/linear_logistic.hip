// CDNA4 (gfx950) logistic regression in fp64 on the matrix cores: the loss and
// gradient of sklearn's LinearModelLoss (the function L-BFGS calls), and the
// scores, probabilities and labels of a fitted model (docs/kernels.md
// "Logistic regression"; limits, LDS carve and launcher rule:
// linear_logistic.h).
//
//   logistic_loss_grad_kernel<RB, NCT, BINOMIAL>   slab row a workgroup
//   logistic_reduce_kernel                         slab rows -> out, in order
//   linear_predict_kernel<RB, NCT, BINOMIAL>       scores, probs, labels
//
// All arithmetic is fp64: v_mfma_f64_16x16x4_f64 with X converted from fp32
// on the LDS read. The instruction's lane maps, established on the device
// with asymmetric operands (lane l, group g = l / 16, column c = l % 16):
//
//   A [16][4]   the lane's one double is A[c][g]
//   B [4][16]   the lane's one double is B[g][c]
//   D [16][16]  the lane's four doubles are D[4 * r + g][c], r = 0..3
//
// A workgroup owns row blocks of RB rows, block g, g + grid, ... in ascending
// order. Of a block:
//
//   pass 1  Z^T = W X^T over 64-feature k-tiles staged in LDS: wave w owns the
//           16-row tiles [w * RB / 64, (w + 1) * RB / 64) of the block, A is a
//           W tile (class c, feature g * 16 + s), B an X tile (row c, the same
//           feature), so a lane's MFMA column is a ROW of X and its four
//           registers and four lane groups are CLASSES. Max, exp-sum and lse of
//           a row fold the registers first and the lane groups second (two
//           xor-shuffles). D = sw * (P - Y) goes to LDS as [class][row], the
//           weighted row losses behind it as one more row.
//   sums    gb and the loss: every (class, 16-row tile) is summed by one thread
//           in row order, then every class over its tiles in tile order.
//   pass 2  the k-tiles again, X from L2: wave w owns the 16-feature column
//           tile w of the k-tile and contracts D X over all RB rows (A is D:
//           class c, row g * 16 + s; B is X: that row, feature c). The
//           accumulators live for one k-tile, so registers do not grow with F.
//           The tile goes to the workgroup's slab row: the first block
//           stores, later blocks add to the same address from the same lane.
//
// A tile's global loads are issued into registers before the MFMAs of the
// tile before it and stored to LDS behind them. No atomics, no fences: the
// stream orders the two launches. The label, the only index derived from
// data, is clamped into [0, classes).

#include <hip/hip_runtime.h>

#include <type_traits>

#include "linear_logistic.h"
#include "tabular_launch.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = LOGISTIC_BLOCK;
constexpr int KT = LOGISTIC_KT;
constexpr int XS = LOGISTIC_XS;
constexpr int WS = LOGISTIC_WS;

template <int RB, int NCT>
struct Carve {
  static constexpr int NBUF = logistic_nbuf(RB, NCT);
  static constexpr int DS = logistic_ds(RB);
  static constexpr int CROWS = NCT * 16 + 1;        // class rows of D, and the loss row
  static constexpr int TILES = RB / 16;
  static constexpr int W_OFF = 0;
  static constexpr int D_OFF = W_OFF + NBUF * logistic_w_bytes(NCT);
  static constexpr int PART_OFF = D_OFF + logistic_d_bytes(RB, NCT);
  static constexpr int X_OFF = PART_OFF + logistic_part_bytes(RB, NCT);
  static constexpr int TOTAL = X_OFF + NBUF * logistic_x_bytes(RB);
  static_assert(TOTAL == logistic_lds_bytes(RB, NCT, NBUF) && D_OFF % 8 == 0 &&
                    PART_OFF % 8 == 0 && X_OFF % 8 == 0,
                "the carve of linear_logistic.h");
};

__device__ __forceinline__ f64x4 mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ double xor_max(double v) {
  v = fmax(v, __shfl_xor(v, 16, 64));
  return fmax(v, __shfl_xor(v, 32, 64));
}

// the same bits in every lane: each step adds a pair in both orders
__device__ __forceinline__ double xor_sum(double v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

// ---- staging: global -> registers -> LDS ---------------------------------------
//
// The X tile of a k-tile, RB / 4 floats a thread. With F a multiple of 4 (and
// X on a 16-byte boundary) a thread loads 16-byte vectors (row tid / 16 + 16 j,
// columns 4 * (tid % 16)), otherwise single floats (row tid / 64 + 4 j, column
// tid % 64). Every load is unconditional and from inside the block: an address
// is a uniform row base plus one of TWO per-thread offsets, the thread's own
// row of a full group of rows or, in the block's last (possibly partial)
// group, that row clamped to the last; a group behind the last reads the last
// again. Rows behind the block's last and features behind F are zeroed by a
// select. The LDS stores of a wave hit distinct banks in both
// forms (4 * column group + row, and column).
template <int RB>
__device__ __forceinline__ void load_x(float (&v)[RB / 4], const float* __restrict__ X,
                                       long long row0, int nrows, int F, int k0, bool vec,
                                       int tid) {
  const float* __restrict__ Xb = X + (size_t)row0 * (size_t)F;
  if (vec) {
    const int c = k0 + (tid & 15) * 4, r0 = tid >> 4;
    const bool cin = c < F;
    const int last = (nrows - 1) & ~15, r_last = nrows - 1 - last;
    const unsigned off_full = (unsigned)(r0 * F + (cin ? c : 0));
    const unsigned off_last = (unsigned)((r0 < r_last ? r0 : r_last) * F + (cin ? c : 0));
#pragma unroll
    for (int j = 0; j < RB / 16; ++j) {
      const bool full = 16 * j < last;                             // uniform
      const float4 q = *reinterpret_cast<const float4*>(
          Xb + (size_t)(full ? 16 * j : last) * (size_t)F + (full ? off_full : off_last));
      const bool in = cin && r0 + 16 * j < nrows;
      v[4 * j + 0] = in ? q.x : 0.f;
      v[4 * j + 1] = in ? q.y : 0.f;
      v[4 * j + 2] = in ? q.z : 0.f;
      v[4 * j + 3] = in ? q.w : 0.f;
    }
  } else {
    const int c = k0 + (tid & 63), r0 = tid >> 6;
    const bool cin = c < F;
    const int last = (nrows - 1) & ~3, r_last = nrows - 1 - last;
    const unsigned off_full = (unsigned)(r0 * F + (cin ? c : F - 1));
    const unsigned off_last = (unsigned)((r0 < r_last ? r0 : r_last) * F + (cin ? c : F - 1));
#pragma unroll
    for (int j = 0; j < RB / 4; ++j) {
      const bool full = 4 * j < last;                              // uniform
      const float q = Xb[(size_t)(full ? 4 * j : last) * (size_t)F + (full ? off_full : off_last)];
      v[j] = (cin && r0 + 4 * j < nrows) ? q : 0.f;
    }
  }
}

template <int RB>
__device__ __forceinline__ void store_x(float* xs, const float (&v)[RB / 4], bool vec, int tid) {
  if (vec) {
    const int c = (tid & 15) * 4, r0 = tid >> 4;
#pragma unroll
    for (int j = 0; j < RB / 16; ++j) {
#pragma unroll
      for (int q = 0; q < 4; ++q) xs[(r0 + 16 * j) * XS + c + q] = v[4 * j + q];
    }
  } else {
    const int c = tid & 63, r0 = tid >> 6;
#pragma unroll
    for (int j = 0; j < RB / 4; ++j) xs[(r0 + 4 * j) * XS + c] = v[j];
  }
}

// The W tile of a k-tile, NCT * 4 doubles a thread: class tid / 64 + 4 j,
// feature tid % 64; classes behind Kc and features behind F are zeros. The
// addresses are formed as load_x forms them.
template <int NCT>
__device__ __forceinline__ void load_w(double (&v)[NCT * 4], const double* __restrict__ W,
                                       int Kc, int F, int k0, int tid) {
  const int c = k0 + (tid & 63), r0 = tid >> 6;
  const bool cin = c < F;
  const int last = (Kc - 1) & ~3, r_last = Kc - 1 - last;
  const unsigned off_full = (unsigned)(r0 * F + (cin ? c : F - 1));
  const unsigned off_last = (unsigned)((r0 < r_last ? r0 : r_last) * F + (cin ? c : F - 1));
#pragma unroll
  for (int j = 0; j < NCT * 4; ++j) {
    const bool full = 4 * j < last;                                // uniform
    const double q = W[(size_t)(full ? 4 * j : last) * (size_t)F + (full ? off_full : off_last)];
    v[j] = (cin && r0 + 4 * j < Kc) ? q : 0.0;
  }
}

template <int NCT>
__device__ __forceinline__ void store_w(double* ws, const double (&v)[NCT * 4], int tid) {
  const int c = tid & 63, r0 = tid >> 6;
#pragma unroll
  for (int j = 0; j < NCT * 4; ++j) ws[(r0 + 4 * j) * WS + c] = v[j];
}

// ---- the forward pass both kernels share ----------------------------------------

// One k-tile of Z^T = W X^T for the wave's RT row tiles.
template <int RT, int NCT>
__device__ __forceinline__ void forward_tile(f64x4 (&acc)[RT][NCT], const float* xs,
                                             const double* ws, int wave, int g, int col) {
  const float* xr = xs + (wave * RT * 16 + col) * XS + g * 16;
  const double* wr = ws + col * WS + g * 16;
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    double a[NCT];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) a[ct] = wr[ct * 16 * WS + s];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const double x = (double)xr[rt * 16 * XS + s];
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = mfma(a[ct], x, acc[rt][ct]);
    }
  }
}

// What a step of the k-tile loop needs staged. Steps 0 .. nkt - 1 are pass 1
// (X and W), steps nkt .. 2 nkt - 1 pass 2 (X alone).
template <int RB, int NCT>
struct Stage {
  float x[RB / 4];
  double w[NCT * 4];

  __device__ __forceinline__ void load(const float* __restrict__ X, const double* __restrict__ W,
                                       long long row0, int nrows, int F, int Kc, int step,
                                       int nkt, bool vec, int tid) {
    const bool fwd = step < nkt;
    const int k0 = (fwd ? step : step - nkt) * KT;
    load_x<RB>(x, X, row0, nrows, F, k0, vec, tid);
    if (fwd) load_w<NCT>(w, W, Kc, F, k0, tid);
  }
  __device__ __forceinline__ void store(float* xs, double* ws, bool fwd, bool vec, int tid) {
    store_x<RB>(xs, x, vec, tid);
    if (fwd) store_w<NCT>(ws, w, tid);
  }
};

// the lane's bias values: class ct * 16 + 4 r + g
template <int NCT>
__device__ __forceinline__ void load_bias(double (&bias)[NCT][4], const double* __restrict__ b,
                                          int Kc, int g) {
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = ct * 16 + 4 * r + g;
      bias[ct][r] = (b != nullptr && c < Kc) ? b[c] : 0.0;
    }
  }
}

// sigma(z) without overflow: exp of a non-positive argument only
__device__ __forceinline__ double logistic(double z) {
  const double e = exp(-fabs(z));
  return z >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// The softmax of the lane's row from its registers: z in, e = exp(z - max)
// out (0 for the pad classes) -> (max, sum of e), the same in the four lanes
// of a row.
template <int NCT>
__device__ __forceinline__ void row_softmax(double (&z)[NCT][4], double (&e)[NCT][4], int Kc,
                                            int g, double& mx, double& sum) {
  mx = -1.7976931348623157e308;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (ct * 16 + 4 * r + g < Kc) mx = fmax(mx, z[ct][r]);
  }
  mx = xor_max(mx);
  sum = 0.0;
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      e[ct][r] = (ct * 16 + 4 * r + g < Kc) ? exp(z[ct][r] - mx) : 0.0;
      sum += e[ct][r];
    }
  }
  sum = xor_sum(sum);
}

// ---- loss and gradient -----------------------------------------------------------

template <int RB, int NCT, bool BINOMIAL>
__global__ void __launch_bounds__(BLOCK)
logistic_loss_grad_kernel(const float* __restrict__ X,     // [N][F]
                          const int* __restrict__ y,       // [N]
                          const double* __restrict__ sw,   // [N] or null
                          const double* __restrict__ W,    // [Kc][F]
                          const double* __restrict__ b,    // [Kc] or null
                          double* __restrict__ slabs,      // [grid][slab_stride]
                          int N, int F, int Kc, int slab_stride) {
  typedef Carve<RB, NCT> C;
  constexpr int RT = RB / 64;                  // 16-row tiles a wave
  extern __shared__ double lds_f64[];
  char* base = reinterpret_cast<char*>(lds_f64);
  double* s_w = reinterpret_cast<double*>(base + C::W_OFF);
  double* s_d = reinterpret_cast<double*>(base + C::D_OFF);
  double* s_part = reinterpret_cast<double*>(base + C::PART_OFF);
  float* s_x = reinterpret_cast<float*>(base + C::X_OFF);

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int nkt = (F + KT - 1) / KT;
  const bool vec = (F & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const long long n_blocks = ((long long)N + RB - 1) / RB;
  double* __restrict__ slab = slabs + (size_t)blockIdx.x * (size_t)slab_stride;
  const int gb_off = Kc * F;

  double bias[NCT][4];
  load_bias<NCT>(bias, b, Kc, g);

  for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const bool first = blk == (long long)blockIdx.x;
    const long long row0 = blk * RB;
    const int nrows = (long long)N - row0 < RB ? (int)((long long)N - row0) : RB;

    f64x4 acc[RT][NCT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    }

    Stage<RB, NCT> st;
    st.load(X, W, row0, nrows, F, Kc, 0, nkt, vec, tid);
    for (int step = 0; step < 2 * nkt; ++step) {
      const bool fwd = step < nkt;
      const int kt = fwd ? step : step - nkt;
      const int buf = step & (C::NBUF - 1);
      float* xs = s_x + buf * (RB * XS);
      double* ws = s_w + buf * (NCT * 16 * WS);
      st.store(xs, ws, fwd, vec, tid);
      __syncthreads();
      // the next tile's loads fly during this tile's MFMAs; pass 2's first
      // tile is loaded behind the head instead, whose registers it would crowd
      const bool head = step == nkt - 1;
      if (step + 1 < 2 * nkt && !head) st.load(X, W, row0, nrows, F, Kc, step + 1, nkt, vec, tid);

      if (fwd) {
        forward_tile<RT, NCT>(acc, xs, ws, wave, g, col);
        if (head) {
          // ---- the head: D = sw * (P - Y) and the weighted row losses ------------
#pragma unroll
          for (int rt = 0; rt < RT; ++rt) {
            const int row = (wave * RT + rt) * 16 + col;
            const bool live = row < nrows;
            const long long grow = row0 + (live ? row : 0);
            const int yr = y[grow];
            const double w_row = live ? (sw != nullptr ? sw[grow] : 1.0) : 0.0;
            double* drow = s_d + row;
            double loss;
            if (BINOMIAL) {
              const int yc = yr < 0 ? 0 : (yr > 1 ? 1 : yr);
              const double z = acc[rt][0][0] + bias[0][0];
              loss = log1p(exp(-fabs(z))) + fmax(z, 0.0) - (double)yc * z;
              const double d = w_row * (logistic(z) - (double)yc);
#pragma unroll
              for (int r = 0; r < 4; ++r) drow[(4 * r + g) * C::DS] = (g == 0 && r == 0) ? d : 0.0;
            } else {
              const int yc = yr < 0 ? 0 : (yr >= Kc ? Kc - 1 : yr);
              double z[NCT][4], e[NCT][4], mx, sum;
              double zy = 0.0;
#pragma unroll
              for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  z[ct][r] = acc[rt][ct][r] + bias[ct][r];
                  zy += (ct * 16 + 4 * r + g == yc) ? z[ct][r] : 0.0;
                }
              }
              row_softmax<NCT>(z, e, Kc, g, mx, sum);
              zy = xor_sum(zy);                  // one lane holds it, three hold 0
              loss = mx + log(sum) - zy;
#pragma unroll
              for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                  const int c = ct * 16 + 4 * r + g;
                  const double p = e[ct][r] / sum;       // 0 for a pad class
                  drow[c * C::DS] = w_row * (c == yc ? p - 1.0 : p);
                }
              }
            }
            if (g == 0) drow[NCT * 16 * C::DS] = w_row * loss;
          }
          __syncthreads();
          // ---- gb and the loss: (class, tile) sums in row order ... ----------------
          for (int i = tid; i < C::CROWS * C::TILES; i += BLOCK) {
            const double* d = s_d + (i / C::TILES) * C::DS + (i % C::TILES) * 16;
            double s = 0.0;
#pragma unroll
            for (int q = 0; q < 16; ++q) s += d[q];
            s_part[i] = s;
          }
          __syncthreads();
          // ---- ... then a class over its tiles in tile order ------------------------
          if (tid < C::CROWS && (tid < Kc || tid == NCT * 16)) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < C::TILES; ++j) s += s_part[tid * C::TILES + j];
            double* dst = slab + gb_off + (tid < Kc ? tid : Kc);
            *dst = first ? s : *dst + s;
          }
          st.load(X, W, row0, nrows, F, Kc, step + 1, nkt, vec, tid);
        }
      } else {
        // ---- pass 2: the wave's 16 features of this k-tile, D X over all rows ------
        f64x4 gacc[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) gacc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        const float* xr = xs + (g * 16) * XS + wave * 16 + col;
        const double* dr = s_d + col * C::DS + g * 16;
#pragma unroll
        for (int chunk = 0; chunk < RB / 64; ++chunk) {
#pragma unroll
          for (int s = 0; s < 16; ++s) {
            const double x = (double)xr[(chunk * 64 + s) * XS];
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
              gacc[ct] = mfma(dr[ct * 16 * C::DS + chunk * 64 + s], x, gacc[ct]);
          }
        }
        const int f = kt * KT + wave * 16 + col;
        if (f < F) {
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = ct * 16 + 4 * r + g;
              if (c < Kc) {
                double* dst = slab + (size_t)c * (size_t)F + f;
                *dst = first ? gacc[ct][r] : *dst + gacc[ct][r];
              }
            }
          }
        }
      }
      if (C::NBUF == 1) __syncthreads();       // the one tile is free again
    }
    if (C::NBUF == 2) __syncthreads();         // the next block's first store
  }
}

// out = the slab rows added in workgroup order, scaled, plus the penalty.
// Entry j of gW and gb is one thread's; the last workgroup has the loss and
// sums |W|^2 in a fixed order (a thread its strided share, then a tree).
__global__ void __launch_bounds__(BLOCK)
logistic_reduce_kernel(const double* __restrict__ slabs, int n_wg, int slab_stride,
                       const double* __restrict__ W, int Kc, int F, int with_b, double sw_sum,
                       double l2, double* __restrict__ out) {
  __shared__ double s_sq[BLOCK];
  const int tid = threadIdx.x;
  const int n_w = Kc * F;
  const int n_grad = n_w + (with_b ? Kc : 0);
  if (blockIdx.x + 1 < gridDim.x) {
    const long long j = (long long)blockIdx.x * BLOCK + tid;
    if (j < n_grad) {
      double s = 0.0;
      for (int w = 0; w < n_wg; ++w) s += slabs[(size_t)w * (size_t)slab_stride + (size_t)j];
      s /= sw_sum;
      out[j] = j < n_w ? s + l2 * W[j] : s;
    }
    return;
  }
  double sq = 0.0;
  for (int j = tid; j < n_w; j += BLOCK) sq += W[j] * W[j];
  s_sq[tid] = sq;
  __syncthreads();
  for (int half = BLOCK / 2; half > 0; half >>= 1) {
    if (tid < half) s_sq[tid] += s_sq[tid + half];
    __syncthreads();
  }
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += slabs[(size_t)w * (size_t)slab_stride + (size_t)(n_w + Kc)];
    out[n_grad] = s / sw_sum + 0.5 * l2 * s_sq[0];
  }
}

// ---- predict ---------------------------------------------------------------------

template <int RB, int NCT, bool BINOMIAL>
__global__ void __launch_bounds__(BLOCK)
linear_predict_kernel(const float* __restrict__ X,      // [B][F]
                      const double* __restrict__ W,     // [Kc][F]
                      const double* __restrict__ b,     // [Kc] or null
                      double* __restrict__ scores,      // [>= B][Kc]
                      double* __restrict__ probs,       // [>= B][K] or null
                      int* __restrict__ labels,         // [>= B]
                      int B, int F, int Kc) {
  typedef Carve<RB, NCT> C;
  constexpr int RT = RB / 64;
  extern __shared__ double lds_f64[];
  char* base = reinterpret_cast<char*>(lds_f64);
  double* s_w = reinterpret_cast<double*>(base + C::W_OFF);
  float* s_x = reinterpret_cast<float*>(base + C::X_OFF);

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int nkt = (F + KT - 1) / KT;
  const bool vec = (F & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
  const long long n_blocks = ((long long)B + RB - 1) / RB;

  double bias[NCT][4];
  load_bias<NCT>(bias, b, Kc, g);

  for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    const long long row0 = blk * RB;
    const int nrows = (long long)B - row0 < RB ? (int)((long long)B - row0) : RB;
    f64x4 acc[RT][NCT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int ct = 0; ct < NCT; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    Stage<RB, NCT> st;
    st.load(X, W, row0, nrows, F, Kc, 0, nkt, vec, tid);
    for (int step = 0; step < nkt; ++step) {
      const int buf = step & (C::NBUF - 1);
      float* xs = s_x + buf * (RB * XS);
      double* ws = s_w + buf * (NCT * 16 * WS);
      st.store(xs, ws, true, vec, tid);
      __syncthreads();
      if (step + 1 < nkt) st.load(X, W, row0, nrows, F, Kc, step + 1, nkt, vec, tid);
      forward_tile<RT, NCT>(acc, xs, ws, wave, g, col);
      if (C::NBUF == 1) __syncthreads();
    }
    if (C::NBUF == 2) __syncthreads();

#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const int row = (wave * RT + rt) * 16 + col;
      const bool live = row < nrows;
      const size_t grow = (size_t)(row0 + (live ? row : 0));
      if (BINOMIAL) {
        const double z = acc[rt][0][0] + bias[0][0];
        if (live && g == 0) {
          const double p = logistic(z);
          scores[grow] = z;
          if (probs != nullptr) {
            probs[2 * grow] = 1.0 - p;
            probs[2 * grow + 1] = p;
          }
          labels[grow] = z > 0.0 ? 1 : 0;
        }
      } else {
        double z[NCT][4], e[NCT][4], mx, sum;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
          for (int r = 0; r < 4; ++r) z[ct][r] = acc[rt][ct][r] + bias[ct][r];
        }
        row_softmax<NCT>(z, e, Kc, g, mx, sum);
        // the first largest: the lane's lowest class at the row max, then the
        // lowest of the four lanes
        int best = Kc;
#pragma unroll
        for (int ct = NCT - 1; ct >= 0; --ct) {
#pragma unroll
          for (int r = 3; r >= 0; --r) {
            const int c = ct * 16 + 4 * r + g;
            if (c < Kc && z[ct][r] == mx) best = c;
          }
        }
        const int o16 = __shfl_xor(best, 16, 64);
        best = o16 < best ? o16 : best;
        const int o32 = __shfl_xor(best, 32, 64);
        best = o32 < best ? o32 : best;
        if (live) {
#pragma unroll
          for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int c = ct * 16 + 4 * r + g;
              if (c < Kc) {
                scores[grow * (size_t)Kc + c] = z[ct][r];
                if (probs != nullptr) probs[grow * (size_t)Kc + c] = e[ct][r] / sum;
              }
            }
          }
          if (g == 0) labels[grow] = best < Kc ? best : 0;   // a NaN row: class 0
        }
      }
    }
  }
}

// ---- launchers ---------------------------------------------------------------------

int cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
    return 0;
  return n;
}

template <int RB, int NCT, bool BINOMIAL>
int launch_loss_grad(const float* X, const int* y, const double* sw, const double* W,
                     const double* b, int N, int F, int Kc, double* slabs, int slab_stride,
                     int grid, hipStream_t stream) {
  using C = Carve<RB, NCT>;
  constexpr auto kernel = logistic_loss_grad_kernel<RB, NCT, BINOMIAL>;
  if (ensure_dynamic_lds<kernel>(C::TOTAL) != 0) return -2;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), C::TOTAL, stream, X, y, sw, W,
                     b, slabs, N, F, Kc, slab_stride);
  return 0;
}

template <int RB, int NCT, bool BINOMIAL>
int launch_predict(const float* X, const double* W, const double* b, int B, int F, int Kc,
                   double* scores, double* probs, int* labels, int grid, hipStream_t stream) {
  using C = Carve<RB, NCT>;
  constexpr auto kernel = linear_predict_kernel<RB, NCT, BINOMIAL>;
  if (ensure_dynamic_lds<kernel>(C::TOTAL) != 0) return -2;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), C::TOTAL, stream, X, W, b,
                     scores, probs, labels, B, F, Kc);
  return 0;
}

// the instantiation for Kc: the head is binomial at Kc == 1, the class tiles
// one up to 16 classes and two beyond. fn(NCT, BINOMIAL) takes them as
// integral constants.
template <typename Fn>
int dispatch(int Kc, Fn&& fn) {
  if (Kc == 1) return fn(std::integral_constant<int, 1>{}, std::true_type{});
  if (Kc <= 16) return fn(std::integral_constant<int, 1>{}, std::false_type{});
  return fn(std::integral_constant<int, 2>{}, std::false_type{});
}

bool shape_ok(int N, int F, int Kc) {
  return N >= 1 && F >= 1 && F <= LOGISTIC_MAX_FEATURES && Kc >= 1 && Kc <= LOGISTIC_MAX_CLASSES;
}

}  // namespace

extern "C" {

int logistic_launch_shape(long long N, int rows_per_wg, int max_wgs, int* rb) {
  if (N < 1 || max_wgs < 0 || (rows_per_wg != 0 && rows_per_wg != LOGISTIC_RB)) return -3;
  if (max_wgs == 0) {
    static const int cus = cu_count();
    if (cus < 1) return -3;
    max_wgs = 2 * cus;
  }
  *rb = LOGISTIC_RB;
  return logistic_grid(N, *rb, max_wgs);
}

int launch_logistic_loss_grad(const float* X, const int* y, const double* sw, const double* W,
                              const double* b, int N, int F, int Kc, double sw_sum, double l2,
                              double* slabs, int slab_rows, int slab_stride, double* out,
                              int rows_per_wg, int max_wgs, hipStream_t stream) {
  if (!shape_ok(N, F, Kc) || slab_stride < logistic_slab_stride(Kc, F) || !(sw_sum > 0.0) ||
      !(l2 >= 0.0))
    return -3;
  int rb = 0;
  const int grid = logistic_launch_shape(N, rows_per_wg, max_wgs, &rb);
  if (grid < 1) return -3;
  if (grid > slab_rows) return -1;
  const int rc = dispatch(Kc, [&](auto nct, auto bin) {
    return launch_loss_grad<LOGISTIC_RB, decltype(nct)::value, decltype(bin)::value>(
        X, y, sw, W, b, N, F, Kc, slabs, slab_stride, grid, stream);
  });
  if (rc != 0) return rc;
  const int n_grad = Kc * F + (b != nullptr ? Kc : 0);
  hipLaunchKernelGGL(logistic_reduce_kernel, dim3((n_grad + BLOCK - 1) / BLOCK + 1), dim3(BLOCK),
                     0, stream, slabs, grid, slab_stride, W, Kc, F, b != nullptr ? 1 : 0, sw_sum,
                     l2, out);
  return 0;
}

int launch_linear_predict(const float* X, const double* W, const double* b, int B, int F, int Kc,
                          double* scores, double* probs, int* labels, int rows_per_wg,
                          int max_wgs, hipStream_t stream) {
  if (!shape_ok(B, F, Kc)) return -3;
  int rb = 0;
  const int grid = logistic_launch_shape(B, rows_per_wg, max_wgs, &rb);
  if (grid < 1) return -3;
  return dispatch(Kc, [&](auto nct, auto bin) {
    return launch_predict<LOGISTIC_RB, decltype(nct)::value, decltype(bin)::value>(
        X, W, b, B, F, Kc, scores, probs, labels, grid, stream);
  });
}

}  // extern "C"
