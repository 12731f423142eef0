// Device helpers shared by the specialized (tabular_kernels.hip) and the
// generalized (tabular_gen.hip) tabular kernels: bf16 conversion, the one
// Adam update, the packed-weight-image stores and the classifier-head
// pieces. Everything here is arithmetic only; how a kernel stages its
// operands and stores its partial sums stays in the kernel.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "tabular_launch.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned short u16;

__device__ __forceinline__ float bf2f(u16 v) {
  union { float f; unsigned u; } c;
  c.u = ((unsigned)v) << 16;
  return c.f;
}

__device__ __forceinline__ u16 f2bf(float f) {
  union { float f; unsigned u; } c;
  c.f = f;
  unsigned lsb = (c.u >> 16) & 1u;
  c.u += 0x7fffu + lsb;        // round-to-nearest-even
  return (u16)(c.u >> 16);
}

__device__ __forceinline__ float fast_rcp(float x) {
  return __builtin_amdgcn_rcpf(x);   // v_rcp_f32, ~1 ulp — no div sequence
}

// sum over the 16 lanes that share l>>4 (the row axis of an MFMA D tile)
__device__ __forceinline__ float row_sum16(float x) {
  x += __shfl_xor(x, 1, 64);
  x += __shfl_xor(x, 2, 64);
  x += __shfl_xor(x, 4, 64);
  x += __shfl_xor(x, 8, 64);
  return x;
}

// ---------------------------------------------------------------------------
// Adam. Every kernel that steps the optimizer calls adam_update, so the
// expression order (and with it the last bit of every weight) is the same
// on every training path.
// ---------------------------------------------------------------------------

// bias-correction factor 1/(1 - beta^t), from the power beta^t
__device__ __forceinline__ float adam_corr(float beta_pow_t) {
  return fast_rcp(1.f - beta_pow_t);
}

// both factors for step t (the step being applied, counted from 1)
__device__ __forceinline__ void adam_bias_corr(float beta1, float beta2, float t,
                                               float& corr1, float& corr2) {
  corr1 = adam_corr(__powf(beta1, t));
  corr2 = adam_corr(__powf(beta2, t));
}

// p/m/v hold the old values on entry and the new ones on return
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g,
                                            float lr, float beta1, float beta2,
                                            float eps, float corr1, float corr2) {
  const float mi = beta1 * m + (1.f - beta1) * g;
  const float vi = beta2 * v + (1.f - beta2) * g * g;
  m = mi;
  v = vi;
  p = p - lr * (mi * corr1) * fast_rcp(sqrtf(vi * corr2) + eps);
}

// ---------------------------------------------------------------------------
// packed weight images: Adam-phase maintenance, flat param index i -> the
// image element(s) that mirror it (biases have none)
// ---------------------------------------------------------------------------

// specialized layout: the three LDS images incl. their K-pads
// (tabular_launch.h DIGITS_WIMG_*)
__device__ __forceinline__ void wimg_write(u16* __restrict__ wimg, int i, u16 wb) {
  static_assert(DIGITS_HID == 32 && DIGITS_CPAD == 16, "shifts below");
  if (i < DIGITS_OFF_B1) {                              // W1: i = in*HID + h
    const int in = i >> 5;                              // /HID
    const int h = i & 31;
    wimg[DIGITS_WIMG_W1T + h * DIGITS_XS + in] = wb;
  } else if (i >= DIGITS_OFF_W2 && i < DIGITS_OFF_B2) { // W2: j = h*CPAD + c
    const int j = i - DIGITS_OFF_W2;
    const int h = j >> 4;                               // /CPAD
    const int c = j & 15;
    wimg[DIGITS_WIMG_W2S + h * DIGITS_WS + c] = wb;
    wimg[DIGITS_WIMG_W2T + c * DIGITS_WS + h] = wb;
  }
}

// generalized layout (bf16 elems): W1T [hid][inp], then W2s [hid][32]
// (cols >= cpad zero), then W2T [cpad][hid]
__device__ __forceinline__ int wimg_w2s_off(int hid, int inp) { return hid * inp; }
__device__ __forceinline__ int wimg_w2t_off(int hid, int inp) {
  return hid * inp + hid * 32;
}

__device__ __forceinline__ void wimg_write_gen(u16* __restrict__ wimg, int inp,
                                               int hid, int cpad, int i, u16 wb) {
  const int off_b1 = inp * hid;
  const int off_w2 = off_b1 + hid;
  const int off_b2 = off_w2 + hid * cpad;
  if (i < off_b1) {                       // W1: i = in*hid + h
    wimg[(i % hid) * inp + (i / hid)] = wb;
  } else if (i >= off_w2 && i < off_b2) { // W2: j = h*cpad + c
    const int j = i - off_w2;
    const int h = j / cpad, c = j % cpad;
    wimg[wimg_w2s_off(hid, inp) + h * 32 + c] = wb;
    wimg[wimg_w2t_off(hid, inp) + c * hid + h] = wb;
  }
}

// ---------------------------------------------------------------------------
// classifier head over NCT 16-class MFMA tiles (1 for the specialized
// kernels, G::NCT for the generalized ones). The logits arrive transposed
// (L^T), so lane l holds, for batch row l&15, the classes
// c = ct*16 + (l>>4)*4 + r: a row's classes live in registers (ct, r) and
// across the four lane groups lg = l>>4.
// ---------------------------------------------------------------------------

// masked logits: acc + b2 for real classes, -1e30 for the pad
template <int NCT>
__device__ __forceinline__ void head_logits(float (&logit)[NCT][4],
                                            const f32x4 (&acc)[NCT],
                                            const float* b2, int cls, int lg) {
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = ct * 16 + lg * 4 + r;
      logit[ct][r] = (c < cls) ? acc[ct][r] + b2[c] : -1e30f;
    }
  }
}

// row max: fold the register-resident tile axis, then the 4 lane groups
template <int NCT>
__device__ __forceinline__ float head_row_max(const float (&logit)[NCT][4]) {
  float mx = -1e30f;
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, logit[ct][r]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  return mx;
}

// e = exp(logit - mx) for real classes (0 for the pad); returns the row sum
template <int NCT>
__device__ __forceinline__ float head_exp_sum(float (&e)[NCT][4],
                                              const float (&logit)[NCT][4],
                                              float mx, int cls, int lg) {
  float s = 0.f;
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = ct * 16 + lg * 4 + r;
      e[ct][r] = (c < cls) ? __expf(logit[ct][r] - mx) : 0.f;
      s += e[ct][r];
    }
  }
  s += __shfl_xor(s, 16, 64);
  s += __shfl_xor(s, 32, 64);
  return s;
}

// row argmax; ties pick the lowest class (match torch.argmax)
template <int NCT>
__device__ __forceinline__ void head_argmax(const float (&logit)[NCT][4], int cls,
                                            int lg, float& best, int& bcol) {
  best = -1e30f;
  bcol = cls;
  #pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (logit[ct][r] > best) { best = logit[ct][r]; bcol = ct * 16 + lg * 4 + r; }
    }
  }
  #pragma unroll
  for (int d = 16; d < 64; d <<= 1) {
    const float ov = __shfl_xor(best, d, 64);
    const int oc = __shfl_xor(bcol, d, 64);
    if (ov > best || (ov == best && oc < bcol)) { best = ov; bcol = oc; }
  }
}
