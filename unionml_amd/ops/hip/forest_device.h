// Device code that forest_predict.hip and bagged_forest_predict.hip run
// identically: the row-tile stage and the label of a row. Included by those
// two files only (forest.h and bagged_forest.h are read by the host compiler
// as well). docs/kernels.md "The forests' row tile".
#pragma once

#include <hip/hip_runtime.h>

#include "forest_limits.h"

// the eight nodes that a kernel's ChunkRegs names, with their piece number
#define FOREST_EACH_NODE(X) X(0, n0) X(1, n1) X(2, n2) X(3, n3) X(4, n4) X(5, n5) X(6, n6) X(7, n7)

// The workgroup's rows X[row0 .. row0 + nrows) as fp32 into the LDS tile:
// element e = row * F + col of the workgroup's contiguous block goes to
// s_rows[row * stride + col]; a thread takes e = tid, tid + 256, ... and
// moves (row, col) on by 256 elements with an add and a compare. Four
// loads are in flight before the first LDS store; they are unconditional
// (past the end they re-read the block's last element), the stores are
// predicated. No barrier: the caller's stands behind it.
__device__ __forceinline__ void forest_stage_rows(float* s_rows, const float* X,
                                                  long long row0, int nrows, int F, int stride,
                                                  int f_magic, int step_rows, int step_cols,
                                                  int tid) {
  const float* __restrict__ Xw = X + (size_t)row0 * (size_t)F;
  const int n = nrows * F;
  int e = tid;
  int row = (int)(((unsigned)tid * (unsigned)f_magic) >> 20);
  int col = tid - row * F;
  auto fetch = [&](float& v, int& at) {
    v = Xw[e < n ? e : n - 1];
    at = row * stride + col;
    e += FOREST_BLOCK;
    row += step_rows;
    col += step_cols;
    if (col >= F) {
      col -= F;
      ++row;
    }
  };
  for (int e0 = tid; e0 - tid < n; e0 += 4 * FOREST_BLOCK) {
    float v0, v1, v2, v3;
    int a0, a1, a2, a3;
    fetch(v0, a0);
    fetch(v1, a1);
    fetch(v2, a2);
    fetch(v3, a3);
    if (e0 < n) s_rows[a0] = v0;
    if (e0 + FOREST_BLOCK < n) s_rows[a1] = v1;
    if (e0 + 2 * FOREST_BLOCK < n) s_rows[a2] = v2;
    if (e0 + 3 * FOREST_BLOCK < n) s_rows[a3] = v3;
  }
}

// The first column with the largest of a row's K values.
__device__ __forceinline__ int forest_first_largest(const double* s, int K) {
  int best = 0;
  double top = s[0];
  for (int k = 1; k < K; ++k) {
    const double v = s[k];
    if (v > top) {   // strict: ties stay with the lowest class
      top = v;
      best = k;
    }
  }
  return best;
}
