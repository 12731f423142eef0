// CDNA4 (gfx950) row shuffle of a staged training set: the launch that
// opens a shuffled epoch (docs/kernels.md "Shuffled epochs").
//
//   shuffle_rows_kernel<HEAD>: for destination row i < N
//       src    = P(i; N, seed, t_dev[0])        (tabular_shuffle.h)
//       Xs[i]  = Xbf[src]                       inp bf16, inp % 32 == 0
//       ys[i]  = y[src]                         an int32 label, or cpad floats
//       perm_out[i] = src                       (optional)
//
// Pure bandwidth. A wave takes a group of RG = 1 << rg_shift consecutive
// destination rows. Lane l < RG walks the permutation for row l of the
// group ONCE; the lanes that copy a row fetch its index from that lane
// (ds_bpermute: the crossbar, no LDS allocation). The group's rows are then
// one contiguous destination range of RG * pieces 16-byte pieces, which the
// 64 lanes sweep in order: every store instruction writes 1 KiB contiguous,
// every load reads whole 64-byte-aligned runs of source rows. Four pieces
// per lane are in flight before the first store. RG shrinks for wide rows
// (launch_shuffle) so that a wide-row set still spreads over every CU.
//
// Row offsets are 64-bit. No atomics, no LDS, no fences: the kernel boundary
// orders the copy before the steps that read Xs and ys, and the Adam
// kernels that advance t_dev run later in the stream than this launch's one
// read of it. Writes nothing but Xs, ys and perm_out.

#include <hip/hip_runtime.h>

#include "tabular_common.h"
#include "tabular_shuffle.h"

namespace {

constexpr int SHUF_BLOCK = 256;
constexpr int SHUF_WAVES = SHUF_BLOCK / 64;
constexpr int SHUF_UNROLL = 4;

// Copy `rows` gathered rows of `pieces` 16-byte pieces each into the
// contiguous destination dst[0 .. rows * pieces). src_of_lane holds, in
// lane r < rows, the source row of destination row r. Called by a whole
// wave: the index exchange and the loads run with every lane active, only
// the stores are predicated.
__device__ __forceinline__ void copy_group(const uint4* __restrict__ src,
                                           uint4* __restrict__ dst, int pieces,
                                           int rows, unsigned src_of_lane,
                                           int lane) {
  const int total = rows * pieces;   // the launcher keeps RG * pieces <= 2^30
  // this lane's first piece c = lane as (row r, piece p), then c += 64 per
  // step without a division
  const int dr = 64 / pieces, dp = 64 % pieces;
  int r = lane / pieces, p = lane % pieces;
  // one piece of this lane: fetch its row's source index, load the piece,
  // move (r, p) on by 64 pieces. The load is unconditional, so that four
  // are in flight with no branch between them: past the group's end
  // (r >= rows) the index comes from some lane, which holds a row below N
  // (0 where it walked none), and p < pieces always, so the address stays
  // inside the source; only the stores are predicated. v0..v3 are named
  // registers, not an array: an indexed one is spilled or parked in LDS.
  auto fetch = [&](uint4& v) {
    const unsigned s = (unsigned)__shfl((int)src_of_lane, r & 63);
    v = src[(size_t)s * (size_t)pieces + (size_t)p];
    r += dr;
    p += dp;
    if (p >= pieces) {
      p -= pieces;
      ++r;
    }
  };
  static_assert(SHUF_UNROLL == 4, "fetch is written out four times");
  for (int c0 = lane; c0 < total + lane; c0 += 64 * SHUF_UNROLL) {
    uint4 v0, v1, v2, v3;
    fetch(v0);
    fetch(v1);
    fetch(v2);
    fetch(v3);
    if (c0 < total) dst[(size_t)c0] = v0;
    if (c0 + 64 < total) dst[(size_t)(c0 + 64)] = v1;
    if (c0 + 128 < total) dst[(size_t)(c0 + 128)] = v2;
    if (c0 + 192 < total) dst[(size_t)(c0 + 192)] = v3;
  }
}

template <int HEAD>
__global__ void __launch_bounds__(SHUF_BLOCK)
shuffle_rows_kernel(const uint4* __restrict__ Xbf,   // [N][x_pieces] 16-byte pieces
                    const head_target_t<HEAD>* __restrict__ y,
                    uint4* __restrict__ Xs, head_target_t<HEAD>* __restrict__ ys,
                    int* __restrict__ perm_out,      // [N] or null
                    const int* __restrict__ t_dev, unsigned seed, int N,
                    int x_pieces, int y_pieces, int rg_shift) {
  const int lane = threadIdx.x & 63;
  const int RG = 1 << rg_shift;
  const ShufflePerm perm((unsigned)N, seed, (unsigned)t_dev[0]);
  const long long n_groups = ((long long)N + RG - 1) >> rg_shift;
  const long long wave0 = (long long)blockIdx.x * SHUF_WAVES + (threadIdx.x >> 6);
  const long long n_waves = (long long)gridDim.x * SHUF_WAVES;
  for (long long grp = wave0; grp < n_groups; grp += n_waves) {
    const long long row0 = grp << rg_shift;
    const int rows = (int)(N - row0 < RG ? N - row0 : RG);
    unsigned s = 0;
    if (lane < rows) {
      s = perm((unsigned)(row0 + lane));
      if (perm_out) perm_out[row0 + lane] = (int)s;
      if constexpr (HEAD == HEAD_XENT) ys[row0 + lane] = y[s];
    }
    copy_group(Xbf, Xs + (size_t)row0 * (size_t)x_pieces, x_pieces, rows, s, lane);
    if constexpr (HEAD == HEAD_REG)
      copy_group(reinterpret_cast<const uint4*>(y),
                 reinterpret_cast<uint4*>(ys) + (size_t)row0 * (size_t)y_pieces,
                 y_pieces, rows, s, lane);
  }
}

// rows per wave: 64, halved while a group holds more than 16 KiB of
// features (down to 8), so that wide rows still make enough waves
int group_shift(int x_pieces) {
  int shift = 6;
  while (shift > 3 && ((long long)x_pieces << shift) * 16 > 16384) --shift;
  return shift;
}

template <int HEAD>
int launch_shuffle(const unsigned short* Xbf, const head_target_t<HEAD>* y,
                   unsigned short* Xs, head_target_t<HEAD>* ys, int* perm_out,
                   const int* t_dev, unsigned seed, long long N, int inp, int cpad,
                   hipStream_t stream) {
  if (N < 1 || N > INT_MAX || inp < 32 || inp % 32 != 0) return -3;
  if (HEAD == HEAD_REG && cpad != 16 && cpad != 32) return -3;
  const int x_pieces = inp / 8;                       // bf16: 8 per 16 bytes
  const int y_pieces = HEAD == HEAD_REG ? cpad / 4 : 0;
  const int shift = group_shift(x_pieces);
  // copy_group counts a group's pieces, and a step past them, in an int
  if (((long long)x_pieces << shift) > (1LL << 30)) return -3;
  // sized by volume: one wave per row group up to 2048 workgroups (8 waves
  // for each SIMD of the chip), a grid-stride loop beyond
  const long long groups = (N + (1LL << shift) - 1) >> shift;
  long long blocks = (groups + SHUF_WAVES - 1) / SHUF_WAVES;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(shuffle_rows_kernel<HEAD>, dim3((unsigned)blocks),
                     dim3(SHUF_BLOCK), 0, stream,
                     reinterpret_cast<const uint4*>(Xbf), y,
                     reinterpret_cast<uint4*>(Xs), ys, perm_out, t_dev, seed, (int)N,
                     x_pieces, y_pieces, shift);
  return 0;
}

}  // namespace

extern "C" {

int launch_shuffle_rows(const unsigned short* Xbf, const int* y,
                        unsigned short* Xs, int* ys, int* perm_out,
                        const int* t_dev, unsigned seed, long long N, int inp,
                        hipStream_t stream) {
  return launch_shuffle<HEAD_XENT>(Xbf, y, Xs, ys, perm_out, t_dev, seed, N, inp, 0,
                                   stream);
}

int launch_shuffle_rows_reg(const unsigned short* Xbf, const float* Yt,
                            unsigned short* Xs, float* Yts, int* perm_out,
                            const int* t_dev, unsigned seed, long long N, int inp,
                            int cpad, hipStream_t stream) {
  return launch_shuffle<HEAD_REG>(Xbf, Yt, Xs, Yts, perm_out, t_dev, seed, N, inp,
                                  cpad, stream);
}

}  // extern "C"
