// Shuffled epochs: the keyed permutation of [0, N), defined ONCE for the
// device (tabular_shuffle.hip) and the host (the shuffle_perm_host binding),
// and the shuffle launchers' declarations. ops/reference.py shuffle_perm is
// the Python copy of the permutation; tests hold the three equal.
//
//   src = P(i; N, seed, t)     32-bit unsigned arithmetic only
//
// A balanced Feistel network over 2 * half bits, half = max(1,
// ceil(ceil(log2 N) / 2)), so its domain D = 4^half satisfies N <= D < 4N
// (N = 1: D = 4). SHUFFLE_ROUNDS rounds of
//   (L, R) -> (R, L ^ (fmix32(R ^ rk_r) & mask))
// with fmix32 the murmur3 finalizer and the round keys
//   rk_r = fmix32(seed ^ fmix32(t ^ (0x9E3779B9 * (r + 1) mod 2^32))).
// A result >= N is fed through the network again (cycle walking).
//
// No iteration cap: every Feistel round is invertible, so the network is a
// bijection of [0, D), and i < N lies on a cycle of it. Walking that cycle
// from i comes back to i, which is below N, so a value below N turns up
// after at most D - N + 1 applications (the cycle holds at most D - N
// values that are not). No sort, no state, no floating point: every thread
// evaluates its own index.
#pragma once

#include <hip/hip_runtime_api.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TABULAR_PERM_FN __host__ __device__ __forceinline__
#else
#define TABULAR_PERM_FN inline
#endif

constexpr int SHUFFLE_ROUNDS = 6;
constexpr unsigned SHUFFLE_GOLDEN = 0x9E3779B9u;

TABULAR_PERM_FN unsigned fmix32(unsigned h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

struct ShufflePerm {
  unsigned n;      // rows, 1 <= n <= INT_MAX
  unsigned half;   // bits of a Feistel half, 1..16
  unsigned mask;   // (1 << half) - 1
  unsigned rk[SHUFFLE_ROUNDS];

  TABULAR_PERM_FN ShufflePerm(unsigned n_, unsigned seed, unsigned t) : n(n_) {
    unsigned bits = 0;                       // ceil(log2 n)
    while (bits < 32 && (1ull << bits) < n) ++bits;
    half = bits < 2 ? 1u : (bits + 1) / 2;
    mask = (1u << half) - 1u;
    for (int r = 0; r < SHUFFLE_ROUNDS; ++r)
      rk[r] = fmix32(seed ^ fmix32(t ^ (SHUFFLE_GOLDEN * (unsigned)(r + 1))));
  }

  // one application of the network to x < 4^half
  TABULAR_PERM_FN unsigned feistel(unsigned x) const {
    unsigned L = x >> half, R = x & mask;
    for (int r = 0; r < SHUFFLE_ROUNDS; ++r) {   // constant trip count: unrolled
      const unsigned nr = L ^ (fmix32(R ^ rk[r]) & mask);
      L = R;
      R = nr;
    }
    return (L << half) | R;   // half = 16: L < 2^16, the shift stays in 32 bits
  }

  // P(i), i < n; ends by the argument in the header comment
  TABULAR_PERM_FN unsigned operator()(unsigned i) const {
    unsigned x = feistel(i);
    while (x >= n) x = feistel(x);
    return x;
  }
};

extern "C" {

// ---- tabular_shuffle.hip ------------------------------------------------------

// Destination row i < N of Xs (and of ys / Yts, and perm_out[i] when given)
// receives source row P(i; N, seed, t_dev[0]). Rows are inp bf16 (inp a
// positive multiple of 32) and an int32 label or cpad (16 or 32) floats;
// every matrix 16-byte aligned, sources and destinations disjoint.
// 0 launched, -3 arguments outside that (tabular_launch.h's convention).
int launch_shuffle_rows(const unsigned short* Xbf, const int* y,
                        unsigned short* Xs, int* ys, int* perm_out,
                        const int* t_dev, unsigned seed, long long N, int inp,
                        hipStream_t stream);
int launch_shuffle_rows_reg(const unsigned short* Xbf, const float* Yt,
                            unsigned short* Xs, float* Yts, int* perm_out,
                            const int* t_dev, unsigned seed, long long N, int inp,
                            int cpad, hipStream_t stream);

}  // extern "C"
