// CDNA4 (gfx950) device-side evaluation of the generalized tabular MLP:
// a forward-only kernel that ends in metrics instead of gradients or
// predictions, and the one-workgroup kernel that finishes them.
//
//   mlp_eval_gen_kernel<HID, RT, CP, HEAD>: grid = ceil(B / RT). Reads what
//     the step kernel reads (staged bf16 Xbf, the packed weight image, the
//     biases from master, the targets in the step's format) and writes ONE
//     row of unnormalised fp32 sums per workgroup, part[wg][.]:
//       classifier  [0] sum of -log softmax(z)[y]   [1] rows with argmax == y
//       regression  [0] sum of 0.5 * sum_c (z-y)^2  [1 + c] sum of (z-y)^2
//     fwd1 issues its MFMAs in mlp_predict_gen_kernel's order (tile by tile,
//     ks ascending, same fragment roles), so the logits carry predict's fp32
//     bits and the correct count equals predict's argmax compared on the
//     host, row for row.
//   eval_finish_kernel: adds the workgroups' rows in index order in fp64,
//     rounds once to fp32 and writes one metrics record into a history
//     array at a device-resident slot, which it then advances: a captured
//     epoch that ends in an evaluation replays with no host involvement.
//
// Summation order. A workgroup's sums run over its RT/16 row tiles. Each
// tile's partial (its 16 rows by row_sum16's fixed butterfly, the scalars
// also over the lane groups) is stored to the tile's own row of L.part;
// one thread per entry then adds the rows tile 0 first, left to right,
// one fp32 rounding per addition (docs/kernels.md "Ordered tile sums").
// No atomics, no arrival order anywhere; the kernel boundary is the
// cross-workgroup barrier, as with reduce_adam_gen.

#include <hip/hip_runtime.h>

#include "tabular_common.h"
#include "tabular_gen_tiles.h"

namespace gen {

// entries of a workgroup's partial row and of a metrics record, by head
template <int HEAD, int CPAD>
constexpr int eval_rec_n() {
  return HEAD == HEAD_REG ? EVAL_REC_FIRST_MSE + CPAD : EVAL_REC_CLS_N;
}

template <int HID, int RT, int CP, int HEAD>
__global__ void __launch_bounds__(512)
mlp_eval_gen_kernel(const u16* __restrict__ Xbf,   // [B][inp] staged bf16 (zero-padded)
                    const head_target_t<HEAD>* __restrict__ y, int B,
                    int inp, int cls,
                    const u16* __restrict__ wimg,      // packed weight images
                    const float* __restrict__ master,  // biases
                    float* __restrict__ part, int part_stride) {
  using G = GG<HID, RT, CP>;
  constexpr int NREC = eval_rec_n<HEAD, G::CPAD>();
  static_assert(NREC <= G::PS, "a tile's metrics fit its partial row");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  G L;
  L.carve(smem);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, lr = l & 15;
  const long long row0 = (long long)blockIdx.x * RT;

  const int off_b1 = inp * HID;
  const int off_b2 = off_b1 + HID + HID * G::CPAD;

  load_w2_images(L, wimg, inp);
  for (int i = tid; i < HID; i += G::BLOCK) L.b1s[i] = master[off_b1 + i];
  if (tid < G::CPAD) L.b2s[tid] = master[off_b2 + tid];
  __syncthreads();

  // ---- fwd1: H^T = W1T @ B(Xs), K streamed in TK tiles, double-buffered
  // where LDS allows (the step's loop; predict's MFMA order over k)
  f32x4 acc1[G::SLOTS];
  #pragma unroll
  for (int s = 0; s < G::SLOTS; ++s) acc1[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = (inp + G::TK - 1) / G::TK;
  load_xs_tile(L, 0, Xbf, inp, row0, (long long)B, 0, min(G::TK, inp));
  load_w1t_tile(L, 0, wimg, inp, 0, min(G::TK, inp));
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = G::DB ? (kt & 1) : 0;
    if (G::DB && kt + 1 < nkt) {
      const int k0n = (kt + 1) * G::TK;
      const int kvn = min(G::TK, inp - k0n);
      load_xs_tile(L, cur ^ 1, Xbf, inp, row0, (long long)B, k0n, kvn);
      load_w1t_tile(L, cur ^ 1, wimg, inp, k0n, kvn);
    }
    u16 (*W1Tc)[G::W1S] = L.W1T(cur);
    u16 (*Xsc)[G::XSS] = L.Xs(cur);
    #pragma unroll
    for (int s = 0; s < G::SLOTS; ++s) {
      const int t = wave + G::WAVES * s;
      if (t < G::NT1) {
        const int mt = t % (HID / 16);
        const int rt = t / (HID / 16);
        f32x4 acc = acc1[s];
        #pragma unroll
        for (int ks = 0; ks < G::TK / 32; ++ks) {
          const bf16x8 a = *(const bf16x8*)&W1Tc[mt * 16 + lr][ks * 32 + lg * 8];
          const bf16x8 b = *(const bf16x8*)&Xsc[rt * 16 + lr][ks * 32 + lg * 8];
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
        }
        acc1[s] = acc;
      }
    }
    __syncthreads();  // prefetched buffer complete / current reads done
    if (!G::DB && kt + 1 < nkt) {
      const int k0n = (kt + 1) * G::TK;
      const int kvn = min(G::TK, inp - k0n);
      load_xs_tile(L, 0, Xbf, inp, row0, (long long)B, k0n, kvn);
      load_w1t_tile(L, 0, wimg, inp, k0n, kvn);
      __syncthreads();
    }
  }
  // bias + relu, bf16 rounding into Hs (as predict)
  #pragma unroll
  for (int s = 0; s < G::SLOTS; ++s) {
    const int t = wave + G::WAVES * s;
    if (t < G::NT1) {
      const int mt = t % (HID / 16);
      const int rt = t / (HID / 16);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = mt * 16 + lg * 4 + r;
        const int row = rt * 16 + lr;
        float hv = acc1[s][r] + L.b1s[h];
        L.Hs[row][h] = f2bf(hv > 0.f ? hv : 0.f);
      }
    }
  }
  __syncthreads();

  // ---- fwd2 + the head's metrics, one 16-row tile per wave pass ------------
  for (int t2 = wave; t2 < RT / 16; t2 += G::WAVES) {
    // this lane's targets, issued BEFORE the MFMAs so the round trip hides
    // under them. A tail row loads row B-1 and is masked after the wait:
    // the load sits under no branch.
    const long long yrow = min(row0 + t2 * 16 + lr, (long long)B - 1);
    [[maybe_unused]] f32x4 yt[G::NCT];
    [[maybe_unused]] int label = 0;
    if constexpr (HEAD == HEAD_REG) {
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        yt[ct] = *(const f32x4*)&y[yrow * G::CPAD + ct * 16 + lg * 4];
      }
    } else {
      label = y[yrow];
    }
    f32x4 acc[G::NCT];
    #pragma unroll
    for (int ct = 0; ct < G::NCT; ++ct) {
      acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < HID / 32; ++ks) {
        const bf16x8 a = *(const bf16x8*)&L.W2Tt[ct * 16 + lr][ks * 32 + lg * 8];
        const bf16x8 b = *(const bf16x8*)&L.Hs[t2 * 16 + lr][ks * 32 + lg * 8];
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[ct], 0, 0, 0);
      }
    }
    const int row = t2 * 16 + lr;
    const bool valid = (row0 + row) < (long long)B;
    float loss_acc = 0.f;
    if constexpr (HEAD == HEAD_REG) {
      // (z - y)^2 on real targets of valid rows, exactly 0 on pad columns
      // and tail rows (selects, so a pad can leak nothing); a column's sum
      // over the tile's rows goes to the tile's partial row, the row loss
      // 0.5 * sum_c folds over registers here and the lane groups below
      float col[G::NCT][4];
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + lg * 4 + r;
          const bool on = valid && c < cls;
          const float d = (acc[ct][r] + L.b2s[c]) - yt[ct][r];
          const float sq = on ? d * d : 0.f;
          col[ct][r] = sq;
          loss_acc += sq;
        }
      }
      loss_acc *= 0.5f;
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) col[ct][r] = row_sum16(col[ct][r]);
      }
      if (lr == 0) {
        #pragma unroll
        for (int ct = 0; ct < G::NCT; ++ct) {
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            L.part[t2][EVAL_REC_FIRST_MSE + ct * 16 + lg * 4 + r] = col[ct][r];
          }
        }
      }
    } else {
      // a label outside [0, cls) matches no real class: exact zeros
      const bool scored = valid && label >= 0 && label < cls;
      float best;
      int bcol;
      float logit[G::NCT][4], e[G::NCT][4];
      head_logits<G::NCT>(logit, acc, L.b2s, cls, lg);
      head_argmax<G::NCT>(logit, cls, lg, best, bcol);   // best is the row max
      const float logs = __logf(head_exp_sum<G::NCT>(e, logit, best, cls, lg));
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + lg * 4 + r;
          loss_acc += (scored && c == label) ? -(logit[ct][r] - best - logs) : 0.f;
        }
      }
      // every lane group of a row holds the same argmax: group 0 counts it
      float hit = (scored && lg == 0 && bcol == label) ? 1.f : 0.f;
      hit = row_sum16(hit);
      hit = group_sum<16>(hit);
      hit = group_sum<32>(hit);
      if (l == 0) L.part[t2][EVAL_REC_CORRECT] = hit;
    }
    loss_acc = row_sum16(loss_acc);
    loss_acc = group_sum<16>(loss_acc);
    loss_acc = group_sum<32>(loss_acc);
    if (l == 0) L.part[t2][EVAL_REC_LOSS] = loss_acc;
  }
  __syncthreads();

  // ---- the row tiles' partials summed in tile order, ((p0 + p1) + p2) + ...,
  // by one thread per entry, into this workgroup's row (plain stores) --------
  if (tid < NREC) {
    float s = L.part[0][tid];
    #pragma unroll
    for (int j = 1; j < RT / 16; ++j) s += L.part[j][tid];
    part[(long long)blockIdx.x * part_stride + tid] = s;
  }
}

// One workgroup, one thread per record entry: the workgroups' rows added in
// index order in fp64, divided by the row count, rounded once to fp32. The
// classifier's correct count is a sum of integers, exact in fp64, stored as
// the int32's bits. The record goes to hist[min(*slot, cap - 1)]; the slot
// is read by every thread before the barrier and advanced by one thread
// after all of them have written.
__global__ void __launch_bounds__(64)
eval_finish_kernel(const float* __restrict__ part, int n_wg, int part_stride,
                   int nrec, int count_at, int B, float* __restrict__ hist,
                   int hist_stride, int cap, int* __restrict__ slot) {
  const int i = threadIdx.x;
  const int at = *slot;
  const int rowi = max(0, min(at, cap - 1));
  if (i < nrec) {
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += (double)part[(long long)w * part_stride + i];
    float* rec = hist + (long long)rowi * hist_stride;
    if (i == count_at) {
      rec[i] = __int_as_float((int)s);
    } else {
      rec[i] = (float)(s / (double)B);
    }
  }
  __syncthreads();
  if (i == 0) *slot = at + 1;
}

}  // namespace gen

// ---------------------------------------------------------------------------
// host launchers (extern "C"; stream-ordered, capture-safe)
// ---------------------------------------------------------------------------

namespace {

// what a call passes on to the two kernels besides the head's targets
struct EvalOut {
  float* part;
  int part_rows, part_stride;
  float* hist;
  int hist_stride, cap;
  int* slot;
};

template <int HID, int RT, int CP, int HEAD>
int launch_eval_gen_t(const unsigned short* Xbf, const head_target_t<HEAD>* y,
                      int B, int inp, int cls, const unsigned short* wimg,
                      const float* master, const EvalOut& o, hipStream_t stream) {
  using G = gen::GG<HID, RT, CP>;
  constexpr auto kernel = gen::mlp_eval_gen_kernel<HID, RT, CP, HEAD>;
  constexpr int nrec = gen::eval_rec_n<HEAD, CP>();
  const int blocks = (B + RT - 1) / RT;
  if (blocks > o.part_rows) return -1;
  if (o.part_stride < nrec || o.hist_stride < nrec || o.cap < 1) return -3;
  if (ensure_dynamic_lds<kernel>(G::TOTAL) != 0) return -2;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(G::BLOCK), G::TOTAL, stream, Xbf,
                     y, B, inp, cls, wimg, master, o.part, o.part_stride);
  hipLaunchKernelGGL(gen::eval_finish_kernel, dim3(1), dim3(64), 0, stream,
                     (const float*)o.part, blocks, o.part_stride, nrec,
                     HEAD == HEAD_REG ? -1 : EVAL_REC_CORRECT, B, o.hist,
                     o.hist_stride, o.cap, o.slot);
  return 0;
}

// the evaluation kernels exist at the predict rows of the table: the larger
// RT of each (HID, CPAD), both heads
template <int HEAD>
int dispatch_eval_gen(const unsigned short* Xbf, const head_target_t<HEAD>* y,
                      int B, int inp, int hid, int n_out,
                      const unsigned short* wimg, const float* master,
                      const EvalOut& o, hipStream_t stream) {
  if (B < 1 || n_out < 1 || n_out > 32 ||
      !GenGeometry{inp, hid, GenGeometry::cpad_for(n_out)}.ok()) {
    return -3;
  }
  const int cpad = GenGeometry::cpad_for(n_out);
  #define EVAL_ROW(H, R, C, PREDICT)                                          \
    if constexpr (PREDICT) {                                                  \
      if (hid == H && cpad == C)                                              \
        return launch_eval_gen_t<H, R, C, HEAD>(Xbf, y, B, inp, n_out, wimg,  \
                                                master, o, stream);           \
    }
  TABULAR_GEN_INSTANTIATIONS(EVAL_ROW)
  #undef EVAL_ROW
  return -3;
}

}  // namespace

extern "C" {

int eval_rows_per_wg(int hid, int cpad) {
  #define EVAL_RT_ROW(H, R, C, PREDICT) \
    if (PREDICT && hid == H && cpad == C) return R;
  TABULAR_GEN_INSTANTIATIONS(EVAL_RT_ROW)
  #undef EVAL_RT_ROW
  return 0;
}

int launch_mlp_eval_gen(const unsigned short* Xbf, const int* y, int B, int inp,
                        int hid, int cls, const unsigned short* wimg,
                        const float* master, float* part, int part_rows,
                        int part_stride, float* hist, int hist_stride, int cap,
                        int* slot, hipStream_t stream) {
  return dispatch_eval_gen<HEAD_XENT>(
      Xbf, y, B, inp, hid, cls, wimg, master,
      EvalOut{part, part_rows, part_stride, hist, hist_stride, cap, slot}, stream);
}

int launch_mlp_eval_reg_gen(const unsigned short* Xbf, const float* Yt, int B,
                            int inp, int hid, int targets,
                            const unsigned short* wimg, const float* master,
                            float* part, int part_rows, int part_stride,
                            float* hist, int hist_stride, int cap, int* slot,
                            hipStream_t stream) {
  return dispatch_eval_gen<HEAD_REG>(
      Xbf, Yt, B, inp, hid, targets, wimg, master,
      EvalOut{part, part_rows, part_stride, hist, hist_stride, cap, slot}, stream);
}

}  // extern "C"
