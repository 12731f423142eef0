// Ridge regression on the device (linear_gram.hip): the limits, the job and
// slice split, the LDS carve and the launchers' declarations. ops/linear.py is
// the Python side. docs/kernels.md "Ridge regression".
//
//   X [N][F]  fp32, row-major        Y  [N][T] fp64, used without rounding
//   sw [N]    fp64 or absent (every weight 1)
//
// With w_i = sw_i, mu the weighted column means of X and ybar those of Y
// (both zero when `center` is off), ridge_gram writes
//
//   mean [F + T]   mu | ybar
//   A    [F][F]    A_pq = sum_i w_i (x_ip - mu_p)(x_iq - mu_q), + alpha at p == q
//   Xy   [F][T]    sum_i w_i (x_ip - mu_p)(y_it - ybar_t)
//
// in four stream-ordered launches: column moments (one slab row a workgroup),
// their finish (rows added in workgroup order), the Gram tiles (one slab tile
// a job and row slice) and the reduce (slices added in ascending order, both
// triangles of A written from one sum).
#pragma once

#include <climits>

#include <hip/hip_runtime_api.h>

constexpr int GRAM_BLOCK = 256;            // four waves
constexpr int GRAM_TILE = 64;              // columns of an output tile
constexpr int GRAM_CHUNK = 64;             // rows a chunk staged in LDS
constexpr int RIDGE_MAX_FEATURES = 4096;   // A is 134 MB at the limit
constexpr int RIDGE_MAX_TARGETS = 32;      // two 16-wide target tiles
constexpr int GRAM_MAX_SLICES = 65535;     // the launch's second grid dimension
// Workgroups of the moments kernel at most. A constant, not the CU count: the
// order of the moment sums depends on N alone.
constexpr int GRAM_MOMENT_WGS = 512;

// targets padded to one or two MFMA tiles
constexpr int gram_tpad(int T) { return T <= 16 ? 16 : 32; }

// Jobs of a launch: tile pairs (i, j), i <= j, row-major over the upper
// triangle, then one moment strip a tile.
constexpr int gram_tiles(int F) { return (F + GRAM_TILE - 1) / GRAM_TILE; }
constexpr int gram_pairs(int F) { return gram_tiles(F) * (gram_tiles(F) + 1) / 2; }
constexpr int gram_jobs(int F) { return gram_pairs(F) + gram_tiles(F); }
// doubles of one row slice of the slabs: a 64 x 64 tile a pair, Tpad x 64 a strip
constexpr long long gram_slab_stride(int F, int T) {
  return (long long)gram_pairs(F) * GRAM_TILE * GRAM_TILE +
         (long long)gram_tiles(F) * GRAM_TILE * gram_tpad(T);
}
static_assert(gram_tiles(1) == 1 && gram_tiles(64) == 1 && gram_tiles(65) == 2 &&
                  gram_pairs(130) == 6 && gram_jobs(130) == 9 &&
                  gram_jobs(RIDGE_MAX_FEATURES) == 2144,
              "nt (nt + 1) / 2 pair jobs and nt strip jobs");
static_assert(gram_slab_stride(RIDGE_MAX_FEATURES, RIDGE_MAX_TARGETS) == 8650752 &&
                  RIDGE_MAX_FEATURES * RIDGE_MAX_FEATURES <= INT_MAX &&
                  (GRAM_CHUNK - 1) * RIDGE_MAX_FEATURES + RIDGE_MAX_FEATURES <= INT_MAX,
              "a slice of the slabs, an index into A and an offset into a chunk of X fit an "
              "int; slice * stride and row * F are formed in 64 bits");

// Row slices of a launch: S = clamp(ceil(target / jobs), 1, chunks), slice s
// the chunks [s * chunks / S, (s + 1) * chunks / S): contiguous, none empty.
constexpr long long gram_chunks(long long N) { return (N + GRAM_CHUNK - 1) / GRAM_CHUNK; }
constexpr int gram_slices(long long N, int F, int target) {
  const long long want = (target + gram_jobs(F) - 1) / gram_jobs(F);
  const long long s = want < gram_chunks(N) ? want : gram_chunks(N);
  return (int)(s < 1 ? 1 : (s > GRAM_MAX_SLICES ? GRAM_MAX_SLICES : s));
}
constexpr long long gram_slice_begin(long long chunks, int S, int s) { return chunks * s / S; }
static_assert(gram_slices(442, 10, 512) == 7 && gram_slices(60000, 784, 512) == 5 &&
                  gram_slices(1, 1, 512) == 1 && gram_slices(2147483647LL, 4096, 512) == 1 &&
                  gram_slice_begin(5, 3, 1) == 1 && gram_slice_begin(5, 3, 2) == 3 &&
                  gram_slice_begin(5, 3, 3) == 5,
              "the slice rule; 259 rows are chunks {0}, {1, 2}, {3, 4} over three slices");

// workgroups (slab rows) of the moments kernel: a 64-row block each, capped
constexpr int gram_moment_rows(long long N) {
  return (int)(gram_chunks(N) < GRAM_MOMENT_WGS ? gram_chunks(N) : GRAM_MOMENT_WGS);
}
// doubles of a moment slab row: sum w x | sum w y | sum w
constexpr int gram_moment_stride(int F, int T) { return F + T + 1; }

// LDS of a Gram workgroup, bytes from the base of dynamic LDS. The LDS has 64
// dword banks; an 8-byte read is served in two halves of 32 lanes.
//   panel L  [64][64] fp32 at stride 65 dwords (= 1 mod 64)        16,640
//   panel R  the same; a strip job keeps D = w (Y - ybar) here,
//            fp64 [Tpad][64] at stride 65 doubles (= 1 mod 32)     16,640
//   w        fp64 [64], the chunk's weights (0 behind the last row)    512
// Every operand read is row (lane / 16) * 16 + s, column c0 + lane % 16 of a
// panel: bank 16 * 65 * group + lane % 16 = 16 * group + lane % 16 (+ const),
// 64 distinct banks (lane group g contracts the g-th sixteenth of the chunk,
// as in linear_logistic.h). D is read as target lane % 16, row
// group * 16 + s: bank pair target + 16 * group + s, 32 distinct a half.
// One buffer: 33,792 bytes, four workgroups a CU by LDS; the next chunk's
// global loads wait in registers during a chunk's MFMAs.
constexpr int GRAM_XS = GRAM_TILE + 1;
constexpr int GRAM_DS = GRAM_CHUNK + 1;
constexpr int GRAM_PANEL_BYTES = GRAM_CHUNK * GRAM_XS * 4;
constexpr int GRAM_LDS_BYTES = 2 * GRAM_PANEL_BYTES + GRAM_CHUNK * 8;
static_assert(GRAM_PANEL_BYTES == 16640 && GRAM_LDS_BYTES == 33792 &&
                  RIDGE_MAX_TARGETS * GRAM_DS * 8 <= GRAM_PANEL_BYTES && GRAM_PANEL_BYTES % 8 == 0,
              "the carve of docs/kernels.md; D of two target tiles fits panel R exactly");

extern "C" {

// The launch of a ridge_gram call on the current device -> row slices in
// *slices (row_slices 0: by the rule above with a target of twice the CU
// count; otherwise min(row_slices, chunks)), doubles of one slice of the
// slabs in *slab_stride, rows of the moment slabs in *moment_rows. 0, or -3
// for a shape outside the limits or row_slices outside 0..GRAM_MAX_SLICES.
int ridge_launch_shape(long long N, int F, int T, int row_slices, int* slices,
                       long long* slab_stride, int* moment_rows);

// mean, A, Xy as in the header comment. slabs holds slab_doubles >= slices *
// slab_stride doubles, moment_slabs [moment_slab_rows >= moment_rows][F + T + 1];
// both are overwritten. sw may be null; its sum must be positive. No atomics,
// no fences, no index derived from data: the same call gives the same bits.
// 0 launched, -1 slabs or moment slabs too small, -2 the dynamic-LDS attribute
// failed, -3 arguments outside the kernels' range (tabular_launch.h's
// convention).
int launch_ridge_gram(const float* X, const double* Y, const double* sw, int N, int F, int T,
                      double alpha, int center, double* mean, double* A, double* Xy,
                      double* slabs, long long slab_doubles, double* moment_slabs,
                      int moment_slab_rows, int row_slices, hipStream_t stream);

}  // extern "C"
