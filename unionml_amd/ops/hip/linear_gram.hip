// CDNA4 (gfx950) ridge regression: the centred, weighted Gram matrix
// Xc^T S Xc (+ alpha I) and the moment matrix Xc^T S Yc in fp64 on the matrix
// cores, from the fp32 X the logistic path holds (docs/kernels.md "Ridge
// regression"; limits, job and slice split, LDS carve: linear_gram.h).
//
//   gram_moments_kernel          sum w x | sum w y | sum w, a slab row a workgroup
//   gram_moments_finish_kernel   slab rows -> mean, in workgroup order
//   ridge_gram_kernel<TPAD>      one output tile of one row slice -> its slab
//   ridge_reduce_kernel<TPAD>    slices -> A (both triangles), Xy, in order
//
// The lane maps of v_mfma_f64_16x16x4_f64 are those of linear_logistic.hip
// (lane l, group g = l / 16, column c = l % 16): A[c][g], B[g][c],
// D[4 r + g][c]. Lane group g contracts the g-th sixteenth of a 64-row chunk.
//
// A Gram workgroup is one job and one row slice. A pair job (i, j) streams the
// slice through LDS as two fp32 panels (columns of tile i and of tile j; one
// panel when i == j); wave w owns the 32 x 32 quadrant (w / 2, w % 2) as four
// accumulators. An operand is read as fp32, converted, centred against the
// lane's column mean (one register a tile: a lane's column is fixed) and, on
// the left side, multiplied by w_i. A strip job contracts D = w (Y - ybar),
// fp64 in LDS, with the centred panel: wave w owns 16 features, all targets.
// Rows behind N carry w = 0 and D = 0, columns behind F carry x = 0 and
// mean 0: exact zeros either way.
//
// No atomics, no fences, no index derived from data; the stream orders the
// launches.

#include <hip/hip_runtime.h>

#include "linear_gram.h"
#include "tabular_launch.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int BLOCK = GRAM_BLOCK;
constexpr int XS = GRAM_XS;
constexpr int DS = GRAM_DS;
constexpr int TILE = GRAM_TILE;
constexpr int CHUNK = GRAM_CHUNK;

__device__ __forceinline__ f64x4 mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bool can_vec(const float* X, int F) {
  return (F & 3) == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
}

// ---- column moments ----------------------------------------------------------------

// Workgroup b takes the 64-row blocks b, b + grid, ... in ascending order. A
// pass covers 64 column units (four columns with 16-byte loads, else one): wave
// v sums rows v, v + 4, ... of every block for the pass's units, a lane a unit,
// and the four waves' sums are added in wave order. The last pass takes the T
// columns of Y and, as unit T, the weights themselves.
__global__ void __launch_bounds__(BLOCK)
gram_moments_kernel(const float* __restrict__ X, const double* __restrict__ Y,
                    const double* __restrict__ sw, double* __restrict__ slabs, int N, int F,
                    int T) {
  __shared__ double s_part[4][64 * 4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const bool vec = can_vec(X, F);
  const int width = vec ? 4 : 1;
  const int units = F / width;
  const int x_passes = (units + 63) / 64;
  const long long n_blocks = gram_chunks(N);
  double* __restrict__ slab = slabs + (size_t)blockIdx.x * (size_t)gram_moment_stride(F, T);

  for (int pass = 0; pass <= x_passes; ++pass) {
    const bool is_y = pass == x_passes;                    // uniform
    const int u = pass * 64 + lane;
    const int n_units = is_y ? T + 1 : units;
    const bool active = is_y ? lane < n_units : u < n_units;
    const int uc = is_y ? (lane < T ? lane : T - 1) : (active ? u : 0);   // a column in range
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
      const long long row0 = blk * CHUNK;
      const int nrows = (long long)N - row0 < CHUNK ? (int)((long long)N - row0) : CHUNK;
#pragma unroll 4
      for (int j = 0; j < CHUNK / 4; ++j) {
        const int r = wave + 4 * j;
        const bool in = active && r < nrows;
        const size_t row = (size_t)(row0 + (r < nrows ? r : nrows - 1));
        const double w = sw != nullptr ? sw[row] : 1.0;
        if (is_y) {
          const double y = Y[row * (size_t)T + uc];
          acc[0] += in ? (lane < T ? w * y : w) : 0.0;
        } else if (vec) {
          const float4 q = *reinterpret_cast<const float4*>(X + row * (size_t)F + 4 * uc);
          acc[0] += in ? w * (double)q.x : 0.0;
          acc[1] += in ? w * (double)q.y : 0.0;
          acc[2] += in ? w * (double)q.z : 0.0;
          acc[3] += in ? w * (double)q.w : 0.0;
        } else {
          acc[0] += in ? w * (double)X[row * (size_t)F + uc] : 0.0;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_part[wave][lane * 4 + k] = acc[k];
    __syncthreads();
    if (wave == 0 && active) {
      const int n_k = (!is_y && vec) ? 4 : 1;
      for (int k = 0; k < n_k; ++k) {
        double s = 0.0;
#pragma unroll
        for (int v = 0; v < 4; ++v) s += s_part[v][lane * 4 + k];
        slab[is_y ? F + lane : u * width + k] = s;
      }
    }
    __syncthreads();
  }
}

// mean[j] = (the slab rows added in workgroup order) / sum w; zeros without
// centring (n_wg == 0: no slab is read)
__global__ void __launch_bounds__(BLOCK)
gram_moments_finish_kernel(const double* __restrict__ slabs, int n_wg, int F, int T,
                           double* __restrict__ mean) {
  const int j = blockIdx.x * BLOCK + threadIdx.x;
  if (j >= F + T) return;
  if (n_wg == 0) {
    mean[j] = 0.0;
    return;
  }
  const size_t stride = (size_t)gram_moment_stride(F, T);
  double s = 0.0, sw_sum = 0.0;
  for (int g = 0; g < n_wg; ++g) {
    s += slabs[(size_t)g * stride + j];
    sw_sum += slabs[(size_t)g * stride + F + T];
  }
  mean[j] = s / sw_sum;
}

// ---- Gram tiles ----------------------------------------------------------------------

// job -> (i, j) of the upper triangle, row-major; at most nt steps
__device__ __forceinline__ void pair_of(int job, int nt, int& i, int& j) {
  i = 0;
  while (job >= nt - i) {
    job -= nt - i;
    ++i;
  }
  j = i + job;
}

// A chunk's panel of tile `tile`, 16 floats a thread: with 16-byte loads row
// tid / 16 + 16 q, columns 4 * (tid % 16); otherwise row tid / 64 + 4 q, column
// tid % 64. Every load is unconditional, its row clamped to the chunk's last
// and its column into [0, F); zeros come from the select.
__device__ __forceinline__ void load_panel(float (&v)[16], const float* __restrict__ Xb, int nrows,
                                           int F, int tile, bool vec, int tid) {
  if (vec) {
    const int c = tile * TILE + (tid & 15) * 4, r0 = tid >> 4;
    const bool cin = c < F;
    const int cc = cin ? c : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int r = r0 + 16 * q;
      const float4 x = *reinterpret_cast<const float4*>(Xb + (r < nrows ? r : nrows - 1) * F + cc);
      const bool in = cin && r < nrows;
      v[4 * q + 0] = in ? x.x : 0.f;
      v[4 * q + 1] = in ? x.y : 0.f;
      v[4 * q + 2] = in ? x.z : 0.f;
      v[4 * q + 3] = in ? x.w : 0.f;
    }
  } else {
    const int c = tile * TILE + (tid & 63), r0 = tid >> 6;
    const bool cin = c < F;
    const int cc = cin ? c : F - 1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int r = r0 + 4 * q;
      const float x = Xb[(r < nrows ? r : nrows - 1) * F + cc];
      v[q] = (cin && r < nrows) ? x : 0.f;
    }
  }
}

__device__ __forceinline__ void store_panel(float* xs, const float (&v)[16], bool vec, int tid) {
  if (vec) {
    const int c = (tid & 15) * 4, r0 = tid >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int k = 0; k < 4; ++k) xs[(r0 + 16 * q) * XS + c + k] = v[4 * q + k];
    }
  } else {
    const int c = tid & 63, r0 = tid >> 6;
#pragma unroll
    for (int q = 0; q < 16; ++q) xs[(r0 + 4 * q) * XS + c] = v[q];
  }
}

// the weight of the chunk's row `r`: 0 behind the chunk's last row
__device__ __forceinline__ double load_weight(const double* __restrict__ sw, long long row0,
                                              int nrows, int r) {
  const double w = sw != nullptr ? sw[(size_t)(row0 + (r < nrows ? r : nrows - 1))] : 1.0;
  return r < nrows ? w : 0.0;
}

template <int TPAD>
__global__ void __launch_bounds__(BLOCK)
ridge_gram_kernel(const float* __restrict__ X,        // [N][F]
                  const double* __restrict__ Y,       // [N][T]
                  const double* __restrict__ sw,      // [N] or null
                  const double* __restrict__ mean,    // [F + T]
                  double* __restrict__ slabs,         // [slices][slab_stride]
                  int N, int F, int T, long long slab_stride) {
  constexpr int NTT = TPAD / 16;                      // target tiles
  constexpr int YV = TPAD / 4;                        // values of Y a thread
  extern __shared__ double lds_f64[];
  char* base = reinterpret_cast<char*>(lds_f64);
  float* s_l = reinterpret_cast<float*>(base);
  float* s_r = reinterpret_cast<float*>(base + GRAM_PANEL_BYTES);
  double* s_d = reinterpret_cast<double*>(base + GRAM_PANEL_BYTES);
  double* s_w = reinterpret_cast<double*>(base + 2 * GRAM_PANEL_BYTES);

  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63, g = lane >> 4, col = lane & 15;
  const int nt = gram_tiles(F), n_pairs = nt * (nt + 1) / 2;
  const int job = blockIdx.x, slice = blockIdx.y, S = gridDim.y;
  const bool vec = can_vec(X, F);
  const long long chunks = gram_chunks(N);
  const long long c_begin = chunks * slice / S, c_end = chunks * (slice + 1) / S;
  double* __restrict__ slab = slabs + (size_t)slice * (size_t)slab_stride;

  if (job < n_pairs) {
    // ---- a tile pair: the wave's 32 x 32 quadrant of tile (ti, tj) ----------------
    int ti, tj;
    pair_of(job, nt, ti, tj);
    const bool diag = ti == tj;
    const int qr = wave >> 1, qc = wave & 1;
    double mu_l[2], mu_r[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int p = ti * TILE + qr * 32 + a * 16 + col, q = tj * TILE + qc * 32 + a * 16 + col;
      mu_l[a] = p < F ? mean[p] : 0.0;
      mu_r[a] = q < F ? mean[q] : 0.0;
    }
    f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
      for (int b = 0; b < 2; ++b) acc[a][b] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    const float* xr_base = diag ? s_l : s_r;
    const float* pl = s_l + (g * 16) * XS + qr * 32 + col;
    const float* pr = xr_base + (g * 16) * XS + qc * 32 + col;

    float vl[16], vr[16];
    double vw = 0.0;
    auto load = [&](long long chunk) {
      const long long row0 = chunk * CHUNK;
      const int nrows = (long long)N - row0 < CHUNK ? (int)((long long)N - row0) : CHUNK;
      const float* __restrict__ Xb = X + (size_t)row0 * (size_t)F;
      load_panel(vl, Xb, nrows, F, ti, vec, tid);
      if (!diag) load_panel(vr, Xb, nrows, F, tj, vec, tid);
      if (tid < CHUNK) vw = load_weight(sw, row0, nrows, tid);
    };
    load(c_begin);
    for (long long chunk = c_begin; chunk < c_end; ++chunk) {
      store_panel(s_l, vl, vec, tid);
      if (!diag) store_panel(s_r, vr, vec, tid);
      if (tid < CHUNK) s_w[tid] = vw;
      __syncthreads();
      // the next chunk's loads fly during this chunk's MFMAs
      if (chunk + 1 < c_end) load(chunk + 1);
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double w = s_w[g * 16 + s];
        double l[2], r[2];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
          l[a] = w * ((double)pl[s * XS + a * 16] - mu_l[a]);
          r[a] = (double)pr[s * XS + a * 16] - mu_r[a];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = mfma(l[a], r[b], acc[a][b]);
        }
      }
      __syncthreads();                         // the one buffer is free again
    }
    // the lower quadrant of a diagonal tile is never read: the reduce mirrors
    if (!(diag && qr > qc)) {
      double* __restrict__ dst = slab + (size_t)job * (TILE * TILE);
#pragma unroll
      for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            dst[(qr * 32 + a * 16 + 4 * r + g) * TILE + qc * 32 + b * 16 + col] = acc[a][b][r];
        }
      }
    }
  } else {
    // ---- a moment strip: the wave's 16 features of tile ti, all targets ------------
    const int ti = job - n_pairs;
    const int f = ti * TILE + wave * 16 + col;
    const double mu = f < F ? mean[f] : 0.0;
    // the thread's values of Y: row tid % 64, targets tid / 64 + 4 k
    const int yrow = tid & 63, t0 = tid >> 6;
    double ybar[YV];
#pragma unroll
    for (int k = 0; k < YV; ++k) {
      const int t = t0 + 4 * k;
      ybar[k] = mean[F + (t < T ? t : T - 1)];
    }
    f64x4 acc[NTT];
#pragma unroll
    for (int ct = 0; ct < NTT; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    const float* px = s_l + (g * 16) * XS + wave * 16 + col;
    const double* pd = s_d + col * DS + g * 16;

    float vl[16];
    double vy[YV], vw = 0.0;
    auto load = [&](long long chunk) {
      const long long row0 = chunk * CHUNK;
      const int nrows = (long long)N - row0 < CHUNK ? (int)((long long)N - row0) : CHUNK;
      load_panel(vl, X + (size_t)row0 * (size_t)F, nrows, F, ti, vec, tid);
      vw = load_weight(sw, row0, nrows, yrow);
      const double* __restrict__ Yr =
          Y + (size_t)(row0 + (yrow < nrows ? yrow : nrows - 1)) * (size_t)T;
#pragma unroll
      for (int k = 0; k < YV; ++k) {
        const int t = t0 + 4 * k;
        vy[k] = Yr[t < T ? t : T - 1];
      }
    };
    load(c_begin);
    for (long long chunk = c_begin; chunk < c_end; ++chunk) {
      store_panel(s_l, vl, vec, tid);
#pragma unroll
      for (int k = 0; k < YV; ++k) {
        const int t = t0 + 4 * k;
        // vw is 0 behind the chunk's last row; a pad target is an exact zero
        s_d[t * DS + yrow] = t < T ? vw * (vy[k] - ybar[k]) : 0.0;
      }
      __syncthreads();
      if (chunk + 1 < c_end) load(chunk + 1);
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const double x = (double)px[s * XS] - mu;
#pragma unroll
        for (int ct = 0; ct < NTT; ++ct) acc[ct] = mfma(pd[ct * 16 * DS + s], x, acc[ct]);
      }
      __syncthreads();
    }
    double* __restrict__ dst =
        slab + (size_t)n_pairs * (TILE * TILE) + (size_t)ti * (TILE * TPAD);
#pragma unroll
    for (int ct = 0; ct < NTT; ++ct) {
#pragma unroll
      for (int r = 0; r < 4; ++r) dst[(ct * 16 + 4 * r + g) * TILE + wave * 16 + col] = acc[ct][r];
    }
  }
}

// An entry of a job's tile, a thread: the slices added in ascending order.
// A_pq and A_qp come from the same sum (of a diagonal tile only p <= q is
// read), alpha goes on the diagonal, nothing is written for pads.
template <int TPAD>
__global__ void __launch_bounds__(BLOCK)
ridge_reduce_kernel(const double* __restrict__ slabs, int S, long long slab_stride, int F, int T,
                    double alpha, double* __restrict__ A, double* __restrict__ Xy) {
  const int nt = gram_tiles(F), n_pairs = nt * (nt + 1) / 2;
  const int job = blockIdx.y;
  const int e = blockIdx.x * BLOCK + threadIdx.x;      // < 64 * 64
  size_t off;
  int p, q = 0;
  const bool pair = job < n_pairs;
  if (pair) {
    int ti, tj;
    pair_of(job, nt, ti, tj);
    p = ti * TILE + e / TILE;
    q = tj * TILE + e % TILE;
    if (p >= F || q >= F || (ti == tj && p > q)) return;
    off = (size_t)job * (TILE * TILE) + e;
  } else {
    const int ti = job - n_pairs;
    p = ti * TILE + e % TILE;
    q = e / TILE;                                      // the target
    if (e >= TILE * TPAD || p >= F || q >= T) return;
    off = (size_t)n_pairs * (TILE * TILE) + (size_t)ti * (TILE * TPAD) + e;
  }
  double s = 0.0;
  for (int k = 0; k < S; ++k) s += slabs[(size_t)k * (size_t)slab_stride + off];
  if (pair) {
    if (p == q) s += alpha;
    A[p * F + q] = s;
    A[q * F + p] = s;
  } else {
    Xy[p * T + q] = s;
  }
}

// ---- launchers -------------------------------------------------------------------------

int cu_count() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
    return 0;
  return n;
}

bool shape_ok(long long N, int F, int T) {
  return N >= 1 && N <= INT_MAX && F >= 1 && F <= RIDGE_MAX_FEATURES && T >= 1 &&
         T <= RIDGE_MAX_TARGETS;
}

template <int TPAD>
int launch_gram(const float* X, const double* Y, const double* sw, const double* mean, int N,
                int F, int T, double alpha, double* A, double* Xy, double* slabs,
                long long slab_stride, int S, hipStream_t stream) {
  constexpr auto kernel = ridge_gram_kernel<TPAD>;
  if (ensure_dynamic_lds<kernel>(GRAM_LDS_BYTES) != 0) return -2;
  const int jobs = gram_jobs(F);
  hipLaunchKernelGGL(kernel, dim3(jobs, S), dim3(BLOCK), GRAM_LDS_BYTES, stream, X, Y, sw, mean,
                     slabs, N, F, T, slab_stride);
  hipLaunchKernelGGL(ridge_reduce_kernel<TPAD>, dim3(TILE * TILE / BLOCK, jobs), dim3(BLOCK), 0,
                     stream, slabs, S, slab_stride, F, T, alpha, A, Xy);
  return 0;
}

}  // namespace

extern "C" {

int ridge_launch_shape(long long N, int F, int T, int row_slices, int* slices,
                       long long* slab_stride, int* moment_rows) {
  if (!shape_ok(N, F, T) || row_slices < 0 || row_slices > GRAM_MAX_SLICES) return -3;
  if (row_slices == 0) {
    static const int cus = cu_count();
    if (cus < 1) return -3;
    *slices = gram_slices(N, F, 2 * cus);
  } else {
    *slices = (int)(row_slices < gram_chunks(N) ? row_slices : gram_chunks(N));
  }
  *slab_stride = gram_slab_stride(F, T);
  *moment_rows = gram_moment_rows(N);
  return 0;
}

int launch_ridge_gram(const float* X, const double* Y, const double* sw, int N, int F, int T,
                      double alpha, int center, double* mean, double* A, double* Xy,
                      double* slabs, long long slab_doubles, double* moment_slabs,
                      int moment_slab_rows, int row_slices, hipStream_t stream) {
  int S = 0, moment_rows = 0;
  long long stride = 0;
  if (!(alpha >= 0.0) || ridge_launch_shape(N, F, T, row_slices, &S, &stride, &moment_rows) != 0)
    return -3;
  if (slab_doubles < (long long)S * stride || moment_slab_rows < moment_rows) return -1;
  const int n_wg = center ? moment_rows : 0;
  if (center)
    hipLaunchKernelGGL(gram_moments_kernel, dim3(moment_rows), dim3(BLOCK), 0, stream, X, Y, sw,
                       moment_slabs, N, F, T);
  hipLaunchKernelGGL(gram_moments_finish_kernel, dim3((F + T + BLOCK - 1) / BLOCK), dim3(BLOCK),
                     0, stream, moment_slabs, n_wg, F, T, mean);
  return gram_tpad(T) == 16
             ? launch_gram<16>(X, Y, sw, mean, N, F, T, alpha, A, Xy, slabs, stride, S, stream)
             : launch_gram<32>(X, Y, sw, mean, N, F, T, alpha, A, Xy, slabs, stride, S, stream);
}

}  // extern "C"
