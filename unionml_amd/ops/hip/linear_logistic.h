// Logistic regression on the device (linear_logistic.hip): the limits, the LDS
// carve, the launcher rule and the launchers' declarations. ops/linear.py is
// the Python side. docs/kernels.md "Logistic regression".
//
//   X [N][F]  fp32, row-major        y  [N] int32 class indices
//   W [Kc][F] fp64, row-major        b  [Kc] fp64 or absent
//   sw [N]    fp64 or absent (every weight 1)
//
// Kc == 1 is the binomial head (two classes, one score, as sklearn's
// HalfBinomialLoss), Kc >= 2 the multinomial head over Kc classes.
//
// logistic_loss_grad is two stream-ordered launches: logistic_loss_grad_kernel
// leaves one slab row [Kc * F + Kc + 1] fp64 a workgroup (gW row-major, gb,
// the loss sum, none of them scaled), logistic_reduce_kernel adds the rows in
// workgroup order and writes
//
//   out [Kc * F]            gW = sum / sw_sum + l2 * W
//   out [Kc]                gb = sum / sw_sum          (only with b)
//   out [1]                 loss = sum / sw_sum + l2 / 2 * |W|^2
#pragma once

#include <hip/hip_runtime_api.h>

constexpr int LOGISTIC_BLOCK = 256;          // four waves
constexpr int LOGISTIC_KT = 64;              // features a k-tile
constexpr int LOGISTIC_MAX_CLASSES = 32;     // two 16-wide class tiles
// Kc * F + Kc + 1 and every index into W stay far inside an int
constexpr int LOGISTIC_MAX_FEATURES = 1 << 20;
// Rows a row block. Measured (profiles/r28_logreg.md): 64-row blocks beat
// 256-row blocks at 1,797 rows (more CUs busy) and at 60,000 x 784 alike, by
// more than the spread of the timing windows, so 64 is the one compiled size;
// the kernels stay templates over it.
constexpr int LOGISTIC_RB = 64;
constexpr int LOGISTIC_LDS_SHARED = 80 * 1024;   // two workgroups share a CU

// LDS row strides. The LDS has 64 dword banks; an 8-byte read is served in
// two halves of 32 lanes, each over 32 pairs of banks.
//   X tile [RB][64] fp32, stride 65 dwords (= 1 mod 64). Pass 1 reads
//     row (lane % 16), feature (lane / 16) * 16 + s: bank row + 16 * group
//     + s, 64 distinct banks. Pass 2 reads row (lane / 16) * 16 + s, feature
//     f0 + lane % 16: bank 16 * 65 * group + lane % 16 = 16 * group + lane % 16
//     (+ const), 64 distinct banks again. The MFMA contracts over four values
//     of k at a time and does not care which four: lane group g takes the
//     g-th SIXTEENTH of the contracted range rather than k = 4 * s + g, which
//     is what makes one odd stride serve both reads.
//   W tile [Kc padded][64] fp64, stride 65 doubles (= 1 mod 32): class
//     lane % 16, feature group * 16 + s: pair-of-banks class + 16 * group + s,
//     32 distinct a half.
//   D [Kc padded + 1][RB] fp64, stride RB + 1 doubles (= 1 mod 32): pass 2
//     reads class lane % 16, row group * 16 + s: the W pattern.
constexpr int LOGISTIC_XS = LOGISTIC_KT + 1;
constexpr int LOGISTIC_WS = LOGISTIC_KT + 1;
constexpr int logistic_ds(int RB) { return RB + 1; }

// The carve of a workgroup with RB rows and NCT class tiles, bytes from the
// base of dynamic LDS (doubles first, the fp32 tile last):
//   W tiles   NBUF * NCT * 16 * 65 * 8
//   D         (NCT * 16 + 1) * (RB + 1) * 8   sw * (P - Y), and the row losses
//                                             as row NCT * 16
//   partials  (NCT * 16 + 1) * (RB / 16) * 8  sums of D over 16-row tiles
//   X tiles   NBUF * RB * 65 * 4
// NBUF is 2 where the doubled tiles leave room for two workgroups a CU (one
// class tile), otherwise 1 (two class tiles: 51,496 bytes, three a CU); the
// next tile's global loads are in flight in registers during a tile's MFMAs
// either way.
constexpr int logistic_w_bytes(int NCT) { return NCT * 16 * LOGISTIC_WS * 8; }
constexpr int logistic_x_bytes(int RB) { return RB * LOGISTIC_XS * 4; }
constexpr int logistic_d_bytes(int RB, int NCT) { return (NCT * 16 + 1) * logistic_ds(RB) * 8; }
constexpr int logistic_part_bytes(int RB, int NCT) { return (NCT * 16 + 1) * (RB / 16) * 8; }
constexpr int logistic_lds_bytes(int RB, int NCT, int nbuf) {
  return nbuf * (logistic_w_bytes(NCT) + logistic_x_bytes(RB)) + logistic_d_bytes(RB, NCT) +
         logistic_part_bytes(RB, NCT);
}
constexpr int logistic_nbuf(int RB, int NCT) {
  return logistic_lds_bytes(RB, NCT, 2) <= LOGISTIC_LDS_SHARED ? 2 : 1;
}
static_assert(logistic_lds_bytes(64, 1, 2) == 59304 && logistic_nbuf(64, 1) == 2 &&
                  logistic_lds_bytes(64, 2, 1) == 51496 && logistic_nbuf(64, 2) == 1,
              "the carve table of docs/kernels.md");

// Workgroups of a launch: a workgroup a row block, capped at max_wgs (0: twice
// the CU count, the fastest of 1x, 2x and 4x at 60,000 x 784). Workgroup g
// takes blocks g, g + grid, ... in ascending order, so the order of every sum
// depends on (N, RB, grid) alone.
constexpr int logistic_grid(long long N, int RB, int max_wgs) {
  const long long blocks = (N + RB - 1) / RB;
  return (int)(blocks < max_wgs ? blocks : max_wgs);
}
static_assert(logistic_grid(1, 64, 512) == 1 && logistic_grid(259, 64, 3) == 3 &&
                  logistic_grid(60000, 64, 512) == 512 && logistic_grid(2147483647LL, 64, 512) == 512,
              "min(ceil(N / RB), max_wgs)");

// doubles of one slab row
constexpr int logistic_slab_stride(int Kc, int F) { return Kc * F + Kc + 1; }
static_assert(logistic_slab_stride(LOGISTIC_MAX_CLASSES, LOGISTIC_MAX_FEATURES) == 33554465,
              "a slab row at the limits fits an int");

extern "C" {

// The launch of a call on the current device -> rows a block in *rb and the
// workgroup count; rows_per_wg 0 or the compiled size, max_wgs 0: twice the
// CU count. -3 when rows_per_wg is no compiled size or N < 1.
int logistic_launch_shape(long long N, int rows_per_wg, int max_wgs, int* rb);

// out as in the header comment. slabs [slab_rows][slab_stride] fp64 scratch,
// slab_stride >= logistic_slab_stride(Kc, F), overwritten. b and sw may be
// null. A label outside [0, classes) counts as the nearest class. Two launches
// on `stream`, no atomics, no fences: the same call gives the same bits.
// 0 launched, -1 fewer slab rows than workgroups, -2 the dynamic-LDS attribute
// failed, -3 arguments outside the kernels' range (tabular_launch.h's
// convention).
int launch_logistic_loss_grad(const float* X, const int* y, const double* sw, const double* W,
                              const double* b, int N, int F, int Kc, double sw_sum, double l2,
                              double* slabs, int slab_rows, int slab_stride, double* out,
                              int rows_per_wg, int max_wgs, hipStream_t stream);

// scores [B][Kc] = X W^T + b; probs [B][K] the softmax of a row (K = Kc), or
// [1 - s, s] with s the logistic function of the score (Kc == 1, K = 2);
// labels [B] the first largest score, or score > 0 (Kc == 1). probs may be
// null. One launch on `stream`. Return codes as above.
int launch_linear_predict(const float* X, const double* W, const double* b, int B, int F, int Kc,
                          double* scores, double* probs, int* labels, int rows_per_wg,
                          int max_wgs, hipStream_t stream);

}  // extern "C"
