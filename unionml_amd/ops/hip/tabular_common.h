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

// Heads of the generalized kernels (tabular_gen.hip), a compile-time
// choice: softmax + cross-entropy over classes, or squared error over
// continuous targets.
constexpr int HEAD_XENT = 0;
constexpr int HEAD_REG = 1;

// a row's target as the step kernel reads it: an int class label, or a row
// of fp32 standardized targets padded to CPAD columns
template <int HEAD> struct head_target { typedef int type; };
template <> struct head_target<HEAD_REG> { typedef float type; };
template <int HEAD> using head_target_t = typename head_target<HEAD>::type;

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

// x as seen from the lane a DPP control selects within this lane's row of
// 16. Every lane of the row must be active.
template <int CTRL>
__device__ __forceinline__ float dpp_row_f32(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(
      0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// sum over the 16 lanes that share l>>4 (the row axis of an MFMA D tile),
// every lane receiving the sum. Four DPP row operations (v_add_f32_dpp):
// nothing goes through the LDS crossbar, which the ds_bpermute behind
// __shfl_xor does.
//
// Bit for bit the xor-1/2/4/8 __shfl_xor butterfly: the quad_perm stages
// ARE xor 1 and xor 2. After them every lane of a quad holds the identical
// sum (IEEE add is commutative, so both partners of a pair compute the
// same number). Hence lane l^7 holds what lane l^4 holds, and
// row_half_mirror (lane l reads lane l^7) adds the same two numbers the
// xor-4 stage added; after it every lane of a half row agrees, lane l^15
// holds what lane l^8 holds, and row_mirror (l reads l^15) is the xor-8
// stage. Same pairing tree, same rounding.
__device__ __forceinline__ float row_sum16(float x) {
  x += dpp_row_f32<0xB1>(x);    // quad_perm [1,0,3,2]  == xor 1
  x += dpp_row_f32<0x4E>(x);    // quad_perm [2,3,0,1]  == xor 2
  x += dpp_row_f32<0x141>(x);   // row_half_mirror      ~  xor 4
  x += dpp_row_f32<0x140>(x);   // row_mirror           ~  xor 8
  return x;
}

// The two operands of a fold across lanes l and l ^ D, D = 16 or 32 (the
// lane-group axis of an MFMA D tile), without the LDS crossbar:
// v_permlane16_swap exchanges the odd rows of its first operand with the
// even rows of its second, v_permlane32_swap the upper half of the first
// with the lower half of the second. With x in both, the first comes back
// holding the lower partner's x on both lanes and the second the upper
// partner's. The same two numbers meet as in x op __shfl_xor(x, D), and the
// folds built on this are commutative, so no bit changes. Every lane must
// be active. (Measured against ds_bpermute in the fused step:
// profiles/r03_fused_chain.md.)
template <int D>
__device__ __forceinline__ void group_pair(float x, float& a, float& b) {
  static_assert(D == 16 || D == 32, "row-of-16 or half-wave exchange");
  const int xi = __float_as_int(x);
  if constexpr (D == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap(xi, xi, false, false);
    a = __int_as_float(r[0]);
    b = __int_as_float(r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap(xi, xi, false, false);
    a = __int_as_float(r[0]);
    b = __int_as_float(r[1]);
  }
}

// x + (x of lane l ^ D), every lane receiving the result
template <int D>
__device__ __forceinline__ float group_sum(float x) {
  float a, b;
  group_pair<D>(x, a, b);
  return a + b;
}

// max(x, x of lane l ^ D)
template <int D>
__device__ __forceinline__ float group_max(float x) {
  float a, b;
  group_pair<D>(x, a, b);
  return fmaxf(a, b);
}

// ---------------------------------------------------------------------------
// Transposed LDS read of an MFMA 16x16x32 operand whose K axis runs DOWN the
// rows of a row-major image T[k][stride] of 16-bit elements (gfx950
// ds_read_b64_tr_b16).
//
// Operand map: lane l (lg = l>>4, lr = l&15) receives, for k-step ks, the
// eight elements T[ks*32 + lg*8 + 0..7][tile*16 + lr] in registers 0..7. These
// are the elements, in the register positions, that ONE ds_read_b128 of
// TT[tile*16 + lr][ks*32 + lg*8] takes from a transposed copy TT of T, so an
// MFMA fed either way accumulates the same products in the same order.
//
// The instruction, per group of 16 consecutive lanes: the group reads a block
// of 4 rows x 16 columns; lane 4q+p of the group SUPPLIES the address of the
// block's row q, columns 4p..4p+3 (8 bytes); lane i of the group RECEIVES
// column i, row q in its element q. One operand is two such reads, K rows
// +0..3 (half 0, registers 0..3) and +4..7 (half 1, registers 4..7).
// tr_read_elem is the address a lane supplies, as an element offset from
// T[0][0]; tr_read_map_ok replays the instruction's gather over all 64 lanes
// and checks what each register receives against the operand map, and that
// every address is 8-byte aligned (T[0][0] 8-byte aligned at least). A wrong
// map is a failed static_assert, not a wrong gradient.
//
// EXEC: the ISA requires EXEC to be all ones for this instruction, because
// the gather crosses lanes: a masked lane still supplies an address (whatever
// its register holds) for data that active lanes receive. Call tr_read_k8
// only where control flow is uniform over the wave (straight-line code, or a
// branch on a per-wave value such as `wave < 2`, taken by all 64 lanes or by
// none), never under a lane-dependent branch or after an early return of
// part of the wave.
// ---------------------------------------------------------------------------

constexpr int tr_read_elem(int lane, int ks, int tile, int half, int stride) {
  const int lg = lane >> 4, lr = lane & 15;
  return (ks * 32 + lg * 8 + half * 4 + (lr >> 2)) * stride + tile * 16 + (lr & 3) * 4;
}

// KS k-steps of 32 rows, TILES column tiles of 16, rows of `stride` elements
constexpr bool tr_read_map_ok(int stride, int KS, int TILES) {
  if (stride < TILES * 16) return false;   // a row holds its columns
  for (int ks = 0; ks < KS; ++ks)
    for (int tile = 0; tile < TILES; ++tile)
      for (int half = 0; half < 2; ++half)
        for (int lane = 0; lane < 64; ++lane) {
          if ((tr_read_elem(lane, ks, tile, half, stride) * 2) % 8 != 0) return false;
          const int group = lane & ~15, i = lane & 15;
          for (int q = 0; q < 4; ++q) {
            // register half*4 + q of this lane: element i&3 of the 8 bytes
            // that lane 4q + (i>>2) of the group points at
            const int got = tr_read_elem(group + 4 * q + (i >> 2), ks, tile, half, stride) + (i & 3);
            const int want_row = ks * 32 + (lane >> 4) * 8 + half * 4 + q;
            const int want_col = tile * 16 + i;
            if (got / stride != want_row || got % stride != want_col) return false;
          }
        }
  return true;
}

template <int STRIDE, int KS, int TILES>
__device__ __forceinline__ bf16x8 tr_read_k8(const u16 (*T)[STRIDE], int ks, int tile,
                                             int lane) {
  static_assert(tr_read_map_ok(STRIDE, KS, TILES), "transposed-read address map");
  typedef __attribute__((ext_vector_type(4))) short s16x4;
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  const u16* base = &T[0][0];
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s16x4*)(base + tr_read_elem(lane, ks, tile, 0, STRIDE)));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_s16x4*)(base + tr_read_elem(lane, ks, tile, 1, STRIDE)));
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// ---------------------------------------------------------------------------
// Accesses to memory that another workgroup of the SAME launch writes or
// reads (the fused step's gradient slabs and their epoch tags). Every one is
// a global-address-space access carrying sc1: an sc1 store is written
// through, so the bytes leave the XCD's L2 as they are stored and no agent
// release has to write them back; an sc1 load bypasses the CU's L1, the one
// cache another CU's stores never refresh, so no agent acquire has to
// invalidate it. Both hold only if EVERY access to such a byte goes through
// these helpers (guide §6 G16, Rule); none of them waits or orders anything.
// ---------------------------------------------------------------------------

typedef __attribute__((address_space(1))) float xwg_f32;
typedef __attribute__((address_space(1))) unsigned xwg_u32;

// 4-byte store / load (global_store_dword / global_load_dword ... sc1)
__device__ __forceinline__ void xwg_store(float* p, float x) {
  __hip_atomic_store((xwg_f32*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void xwg_store(unsigned* p, unsigned x) {
  __hip_atomic_store((xwg_u32*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float xwg_load(const float* p) {
  return __hip_atomic_load((const xwg_f32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned xwg_load(const unsigned* p) {
  return __hip_atomic_load((const xwg_u32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// 16-byte store of the four consecutive floats base[i .. i+3] as ONE
// buffer_store_dwordx4 ... sc1 (aux bit 4); base + i 16-byte aligned. There
// is no 16-byte atomic to ask for, hence the raw buffer form. The descriptor
// lives in scalar registers, so base and n (the floats it spans) must be
// uniform over the wave and only i may differ from lane to lane; a store
// that would reach past base[n) is dropped by the hardware.
__device__ __forceinline__ void xwg_store4(float* base, int n, int i, f32x4 x) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
  const __amdgpu_buffer_rsrc_t rsrc =       // raw, stride 0, 32-bit data format
      __builtin_amdgcn_make_buffer_rsrc(base, 0, n * 4, 0x00020000);
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), rsrc, i * 4, 0, 16);
}

// ---------------------------------------------------------------------------
// Adam. Every kernel that steps the optimizer calls adam_update. Sharing the
// source expression is not enough to share its bits: left to itself the
// compiler contracts the inlined a*b + c*d sums into a different fma at
// different call sites (adam_step_kernel and adam_step_gen_kernel rounded
// the moments differently from the three fused kernels). So adam_update
// leaves the compiler no such choice (see below); each call site then
// compiles to the same arithmetic and the last bit of m, v and every
// weight is the same on every training path.
// (adam_bias_corr is separate: the persistent kernel keeps its own
// running-product beta^t, docs/kernels.md "Determinism".)
// ---------------------------------------------------------------------------

// bias-correction factor 1/(1 - beta^t), from the power beta^t
__device__ __forceinline__ float adam_corr(float beta_pow_t) {
  return fast_rcp(1.f - beta_pow_t);
}

// one factor for step t (the step being applied, counted from 1)
__device__ __forceinline__ float adam_bias_corr_one(float beta, float t) {
  return adam_corr(__powf(beta, t));
}

// both factors for step t
__device__ __forceinline__ void adam_bias_corr(float beta1, float beta2, float t,
                                               float& corr1, float& corr2) {
  corr1 = adam_bias_corr_one(beta1, t);
  corr2 = adam_bias_corr_one(beta2, t);
}

// p/m/v hold the old values on entry and the new ones on return. With rn()
// one fp32 rounding:
//   m' = fma(1-beta1, g, rn(beta1*m))
//   v' = fma(g, rn((1-beta2)*g), rn(beta2*v))
//   p' = fma(-rn(lr*rn(m'*corr1)), rcp(sqrt(rn(v'*corr2)) + eps), p)
// The three products that feed an fma are rounded on their own (contraction
// off in their block) and the two moment fmas are explicit, so no call site
// can pick another pairing. The last line has a single product under its
// subtraction, hence a single way to contract it. The statements keep the
// evaluation order of the plain expression they replace, so the three
// fused kernels compile to the instructions they had before.
__device__ __forceinline__ void adam_update(float& p, float& m, float& v, float g,
                                            float lr, float beta1, float beta2,
                                            float eps, float corr1, float corr2) {
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  float bm, bv, gs;
  {
    #pragma clang fp contract(off)
    bm = beta1 * m;
    bv = beta2 * v;
    gs = omb2 * g;
  }
  const float mi = __builtin_fmaf(omb1, g, bm);
  const float vi = __builtin_fmaf(g, gs, bv);
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

// the same for one tile whose bias array is padded to the tile (16 floats):
// the caller reads its lane's four values b2[lg*4 .. lg*4+3] as ONE 16-byte
// read, unconditionally and as early as it likes, and the pad is masked
// here. (The form above reads each b2[c] under its c < cls branch: four
// serial LDS round trips between the fwd2 MFMA and the row max.) Same adds,
// same select, same bits.
__device__ __forceinline__ void head_logits_padded(float (&logit)[1][4],
                                                   const f32x4 (&acc)[1],
                                                   f32x4 b2v, int cls, int lg) {
  #pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int c = lg * 4 + r;
    logit[0][r] = (c < cls) ? acc[0][r] + b2v[r] : -1e30f;
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
  mx = group_max<16>(mx);
  mx = group_max<32>(mx);
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
  s = group_sum<16>(s);
  s = group_sum<32>(s);
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
