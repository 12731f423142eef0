// CDNA4 (gfx950) GENERALIZED tabular MLP kernels: any (in_features,
// hidden, classes) geometry, not just the tuned 64x32x10 flagship of
// tabular_kernels.hip.
//
// Design (MI355X-first, not a port — the reference unionai-oss/unionml
// has no kernels; behavior mirrors its pytorch quickstart trainer,
// tests/integration/pytorch_app/quickstart.py:14-70):
//
//   * Template parameters are ONLY <HID, RT> (hidden width, rows per
//     workgroup). The input width is RUNTIME: it appears solely in
//     k-tile counts and global strides, so four instantiations
//     (HID 32/64/128/256) cover every geometry. Odd widths are
//     zero-padded by the Python layer (exact math: zero-init + zero
//     gradient keeps Adam at exactly zero for pad params).
//   * The input dimension streams through LDS in TK=64 k-tiles (a
//     784-feature MNIST row set no longer has to fit in LDS whole);
//     weights live in packed global "images" in kernel-friendly
//     layouts (W1T row-major over K, W2s K-padded, W2T) kept in sync
//     by the in-kernel Adam phase — the same packed-image scheme the
//     specialized kernel's wimg uses.
//   * The training step is TWO kernels: the slab-producing MFMA
//     fwd/bwd (grid = batch rows / rows-per-WG, plain per-WG stores,
//     no atomics) and a wide-grid reduce+Adam kernel whose launch
//     boundary doubles as the inter-workgroup barrier — at generalized
//     nparam sizes an in-grid reduce is bandwidth-starved (memory
//     parallelism scales with resident CUs), so the specialized
//     kernel's G16 epoch-tag handshake is deliberately NOT used here
//     (A/B trail: profiles/r02_gen_kernel_stats.md). MFMA
//     __builtin_amdgcn_mfma_f32_16x16x32_bf16 with the
//     hardware-verified fragment mapping documented in the header of
//     tabular_kernels.hip. Classes are runtime (<= 32, one or two
//     MFMA tiles): the wave-shuffle softmax (tabular_common.h head_*)
//     masks c >= cls and folds across the register-resident
//     class-tile axis.
//   * The head is a compile-time choice of the step and the predict
//     kernel (HEAD_XENT / HEAD_REG): the regression head swaps the
//     softmax/xent epilogue for squared error over cls = T continuous
//     targets and the argmax for the de-standardized outputs. Everything
//     else (fwd1, dH, dW2, dW1, slabs, reduce+Adam) is shared, and
//     every <HID, RT, CPAD> instantiation exists for both heads.
//
// All launches are stream-ordered and hipGraph-capturable; the Adam
// step counter lives in device memory so bias correction is exact
// under graph replay.

#include <hip/hip_runtime.h>

#include "tabular_common.h"
#include "tabular_gen_tiles.h"

namespace gen {

template <typename G>
__device__ __forceinline__ void zero_dl_pad(const G& L) {
  if constexpr (G::CPAD < 32) {
    constexpr int PADW = 32 - G::CPAD;
    for (int i = threadIdx.x; i < G::RT * PADW; i += G::BLOCK) {
      const int r = i / PADW, c = G::CPAD + (i % PADW);
      L.DLs[r][c] = 0;
    }
  }
}

// ---------------------------------------------------------------------------
// fused generalized step kernel
// ---------------------------------------------------------------------------

// The head is a compile-time choice (tabular_common.h HEAD_*): the
// softmax/xent classifier, or squared error over cls = T continuous
// targets. What a row's target is differs with it: an int label y[N], or
// fp32 standardized targets Yt[N][CPAD], pad columns zero. Everything
// outside the fwd2 epilogue is shared.
//
// Summation order (both heads, every instantiation). A workgroup's db1,
// db2 and loss are sums over its RT/16 row tiles of 16 rows. Each tile's
// partial (its 16 rows summed by row_sum16's fixed butterfly, the loss also
// over the lane groups) is STORED to the tile's own row of L.part by one
// lane; nothing is accumulated in arrival order. The last block of the
// kernel adds the rows tile 0 first, left to right,
//   ((part[0] + part[1]) + part[2]) + ... + part[RT/16 - 1],
// one fp32 rounding per addition, and writes the slab entry. A tile of tail
// rows only contributes an exact zero. With reduce_adam_gen's fixed slab
// order this makes the step bit-reproducible by construction
// (tests/test_gpu_gen_order.py holds the kernel to this order bit for bit).
// The stores and the final sum lie outside the head's if constexpr: keep
// them shared, the classifier head has no exact probe of its own.
template <int HID, int RT, int CP, int HEAD = HEAD_XENT>
__global__ void __launch_bounds__(512)
mlp_step_gen_kernel(const u16* __restrict__ Xbf,   // [N][inp] staged bf16 (zero-padded)
                    const head_target_t<HEAD>* __restrict__ y, int B,
                    int inp, int cls,
                    const u16* __restrict__ wimg,  // packed weight images
                    const float* __restrict__ master,  // biases prefetch
                    float* __restrict__ slabs, int slab_stride,
                    float invBtot) {
  using G = GG<HID, RT, CP>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  G L;
  L.carve(smem);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, lr_ = l & 15;
  const long long row0 = (long long)blockIdx.x * RT;

  const int off_b1 = inp * HID;
  const int off_w2 = off_b1 + HID;
  const int off_b2 = off_w2 + HID * G::CPAD;
  const int nparam = off_b2 + G::CPAD;

  zero_dl_pad(L);
  load_w2_images(L, wimg, inp);
  for (int i = tid; i < HID; i += G::BLOCK) L.b1s[i] = master[off_b1 + i];
  if (tid < G::CPAD) L.b2s[tid] = master[off_b2 + tid];
  __syncthreads();

  // ---- fwd1: H^T = W1T @ B(Xs), K streamed in TK tiles over inp.
  // Double-buffered where LDS allows (G::DB): the NEXT tile's
  // cooperative load issues before this tile's MFMAs, so the L2/HBM
  // round trip overlaps compute instead of serializing each k step.
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
          const bf16x8 a = *(const bf16x8*)&W1Tc[mt * 16 + lr_][ks * 32 + lg * 8];
          const bf16x8 b = *(const bf16x8*)&Xsc[rt * 16 + lr_][ks * 32 + lg * 8];
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
  // epilogue: bias + relu, store Hs and HT
  #pragma unroll
  for (int s = 0; s < G::SLOTS; ++s) {
    const int t = wave + G::WAVES * s;
    if (t < G::NT1) {
      const int mt = t % (HID / 16);
      const int rt = t / (HID / 16);
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = mt * 16 + lg * 4 + r;
        const int row = rt * 16 + lr_;
        float hv = acc1[s][r] + L.b1s[h];
        hv = hv > 0.f ? hv : 0.f;
        const u16 hb = f2bf(hv);
        L.Hs[row][h] = hb;
        L.HT[h][row] = hb;
      }
    }
  }
  __syncthreads();

  // prefetch dW1's FIRST transposed-X tile now: xbuf is free (fwd1's
  // last Xs read retired at the barrier above) and nothing between
  // here and dW1 touches it, so the load's round trip hides under the
  // fwd2/dH/dW2 phases
  load_xt_tile(L, 0, Xbf, inp, row0, (long long)B, 0, min(G::TK, inp));

  // ---- fwd2: L^T = W2T @ B(Hs); wave-shuffle softmax + xent over NCT
  // class tiles (classes <= 16: one MFMA tile; 17..32: two tiles, the
  // max/sum folds across the register-resident tile axis first, then
  // the 4 lane-groups). The regression head swaps the softmax block for
  // dz = (z - y) / Btot; the DLs/DLT dual stores, the db2 row sums and the
  // loss fold below are the same code for both heads ------------------------
  for (int t2 = wave; t2 < RT / 16; t2 += G::WAVES) {
    // regression: this lane's targets, 4 consecutive columns per class
    // tile (one aligned 16-byte load each), issued BEFORE the MFMAs so
    // the round trip hides under them. A tail row loads row B-1 and is
    // masked after the wait: the load sits under no branch.
    [[maybe_unused]] f32x4 yt[G::NCT];
    if constexpr (HEAD == HEAD_REG) {
      const long long yrow = min(row0 + t2 * 16 + lr_, (long long)B - 1);
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        yt[ct] = *(const f32x4*)&y[yrow * G::CPAD + ct * 16 + lg * 4];
      }
    }
    f32x4 acc[G::NCT];
    #pragma unroll
    for (int ct = 0; ct < G::NCT; ++ct) {
      acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < HID / 32; ++ks) {
        const bf16x8 a = *(const bf16x8*)&L.W2Tt[ct * 16 + lr_][ks * 32 + lg * 8];
        const bf16x8 b = *(const bf16x8*)&L.Hs[t2 * 16 + lr_][ks * 32 + lg * 8];
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[ct], 0, 0, 0);
      }
    }
    const int row = t2 * 16 + lr_;
    const bool valid = (row0 + row) < (long long)B;
    float db2_acc[G::NCT][4];
    float loss_acc = 0.f;
    if constexpr (HEAD == HEAD_REG) {
      // dz = (z - y) / Btot on real targets of valid rows, exactly 0 on
      // pad columns and tail rows (selects, so a pad can leak nothing);
      // row loss 0.5 / Btot * sum (z - y)^2, folded over registers here
      // and over the lane groups below
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + lg * 4 + r;
          const bool on = valid && c < cls;
          const float d = (acc[ct][r] + L.b2s[c]) - yt[ct][r];
          const float dz = on ? d * invBtot : 0.f;
          const u16 dzb = f2bf(dz);
          L.DLs[row][c] = dzb;
          L.DLT[c][row] = dzb;
          db2_acc[ct][r] = dz;
          loss_acc += on ? d * d : 0.f;
        }
      }
      loss_acc *= 0.5f * invBtot;
    } else {
      const int label = valid ? y[row0 + row] : -1;

      float logit[G::NCT][4], e[G::NCT][4];
      head_logits<G::NCT>(logit, acc, L.b2s, cls, lg);
      const float mx = head_row_max<G::NCT>(logit);
      const float ssum = head_exp_sum<G::NCT>(e, logit, mx, cls, lg);
      const float rs = fast_rcp(ssum);
      const float logs = __logf(ssum);
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + lg * 4 + r;
          const float dl =
              valid ? (e[ct][r] * rs - (c == label ? 1.f : 0.f)) * invBtot : 0.f;
          const u16 dlb = f2bf(dl);
          L.DLs[row][c] = dlb;
          L.DLT[c][row] = dlb;
          db2_acc[ct][r] = dl;
          if (valid && c == label) loss_acc = -(logit[ct][r] - mx - logs) * invBtot;
        }
      }
    }
    // in-row sums first (DPP, every lane active), predicated stores after:
    // this tile's db2 and loss partials go to its own row of L.part, one
    // writing lane per entry (shared by both heads: the if constexpr above
    // has ended)
    #pragma unroll
    for (int ct = 0; ct < G::NCT; ++ct) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) db2_acc[ct][r] = row_sum16(db2_acc[ct][r]);
    }
    loss_acc = row_sum16(loss_acc);
    if (lr_ == 0) {
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          L.part[t2][HID + ct * 16 + lg * 4 + r] = db2_acc[ct][r];
        }
      }
    }
    loss_acc = group_sum<16>(loss_acc);
    loss_acc = group_sum<32>(loss_acc);
    if (l == 0) L.part[t2][HID + G::CPAD] = loss_acc;
  }
  __syncthreads();

  // ---- dH^T = W2s @ B(DLs) + relu mask + db1 -------------------------------
  #pragma unroll
  for (int s = 0; s < G::SLOTS; ++s) {
    const int t = wave + G::WAVES * s;
    if (t < G::NT1) {
      const int mt = t % (HID / 16);
      const int rt = t / (HID / 16);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const bf16x8 a = *(const bf16x8*)&L.W2s[mt * 16 + lr_][lg * 8];
      const bf16x8 b = *(const bf16x8*)&L.DLs[rt * 16 + lr_][lg * 8];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      float db1_acc[4];
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = mt * 16 + lg * 4 + r;
        const int row = rt * 16 + lr_;
        const float hv = bf2f(L.HT[h][row]);
        const float dh = hv > 0.f ? acc[r] : 0.f;
        L.DHT[h][row] = f2bf(dh);
        db1_acc[r] = row_sum16(dh);
      }
      if (lr_ == 0) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) L.part[rt][mt * 16 + lg * 4 + r] = db1_acc[r];
      }
    }
  }
  __syncthreads();  // DHT complete

  float* slab = slabs + (long long)blockIdx.x * slab_stride;

  // ---- dW2 = HT @ B(DLT) -> slab (plain stores) ----------------------------
  for (int t = wave; t < (HID / 16) * G::NCT; t += G::WAVES) {
    const int ht = t % (HID / 16);
    const int ct = t / (HID / 16);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int ks = 0; ks < RT / 32; ++ks) {
      const bf16x8 a = *(const bf16x8*)&L.HT[ht * 16 + lr_][ks * 32 + lg * 8];
      const bf16x8 b = *(const bf16x8*)&L.DLT[ct * 16 + lr_][ks * 32 + lg * 8];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = ht * 16 + lg * 4 + r;
      slab[off_w2 + h * G::CPAD + ct * 16 + lr_] = acc[r];
    }
  }

  // ---- dW1^T = DHT @ B(XT), K'-streamed over inp -> slab -------------------
  // (tile 0 was prefetched before fwd2; the barrier below also covers
  // the dH phase's db1 partials)
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int cur = G::DB ? (kt & 1) : 0;
    if (G::DB && kt + 1 < nkt) {
      const int k0n = (kt + 1) * G::TK;
      load_xt_tile(L, cur ^ 1, Xbf, inp, row0, (long long)B, k0n,
                   min(G::TK, inp - k0n));
    }
    const int k0 = kt * G::TK;
    const int kv = min(G::TK, inp - k0);
    u16 (*XTc)[G::XTS] = L.XT(cur);
    const int ntw = (HID / 16) * (kv / 16);
    for (int t = wave; t < ntw; t += G::WAVES) {
      const int mt = t % (HID / 16);
      const int it = t / (HID / 16);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int ks = 0; ks < RT / 32; ++ks) {
        const bf16x8 a = *(const bf16x8*)&L.DHT[mt * 16 + lr_][ks * 32 + lg * 8];
        const bf16x8 b = *(const bf16x8*)&XTc[it * 16 + lr_][ks * 32 + lg * 8];
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = mt * 16 + lg * 4 + r;
        const int in = k0 + it * 16 + lr_;
        slab[in * HID + h] = acc[r];
      }
    }
    __syncthreads();
    if (!G::DB && kt + 1 < nkt) {
      const int k0n = (kt + 1) * G::TK;
      load_xt_tile(L, 0, Xbf, inp, row0, (long long)B, k0n,
                   min(G::TK, inp - k0n));
      __syncthreads();
    }
  }

  // ---- bias grads + loss into the slab: the row tiles' partials summed in
  // tile order, ((p0 + p1) + p2) + ..., by one thread per entry (part is
  // complete: every tile, an all-tail one included, stored its row, and the
  // barriers of the dW1 loop lie between those stores and here) -------------
  for (int i = tid; i < HID + G::CPAD + 1; i += G::BLOCK) {
    float s = L.part[0][i];
    #pragma unroll
    for (int j = 1; j < RT / 16; ++j) s += L.part[j][i];
    const int at = i < HID ? off_b1 + i : i < HID + G::CPAD ? off_b2 + (i - HID) : nparam;
    slab[at] = s;
  }
}

// ---------------------------------------------------------------------------
// wide-grid reduce + Adam: sums the per-WG slabs and applies Adam (or,
// in grads_out mode, hands the summed grads to the RCCL all-reduce).
//
// Design note vs the specialized kernel's single-launch handshake
// (tabular_kernels.hip G16): at generalized geometries nparam is large
// (MNIST shape: ~102k params -> ~8 MB of slab+state traffic per step)
// and the step grid is tiny (ceil(B/RT) WGs), so an in-kernel reduce is
// bandwidth-starved — memory parallelism scales with resident CUs. A
// separate kernel launches with hundreds of WGs, reaches full-chip
// bandwidth, and the kernel boundary IS the inter-WG barrier, so the
// epoch-tag handshake disappears. Stream-ordered + hipGraph-capturable;
// t advances via bump_t_kernel so every WG sees one consistent t.
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
reduce_adam_gen_kernel(const float* __restrict__ slabs, int n_wg,
                       int slab_stride, int nparam, int inp, int hid, int cpad,
                       float* __restrict__ master, u16* __restrict__ bfmirror,
                       float* __restrict__ m, float* __restrict__ v,
                       int* __restrict__ t_dev,
                       float* __restrict__ loss_out,
                       float lr, float beta1, float beta2, float eps,
                       u16* __restrict__ wimg,
                       float* __restrict__ grads_out,
                       unsigned* __restrict__ done_counter) {
  const float t_new = (float)(*t_dev + 1);
  float corr1, corr2;
  adam_bias_corr(beta1, beta2, t_new, corr1, corr2);
  for (int i = blockIdx.x * 256 + threadIdx.x; i <= nparam;
       i += gridDim.x * 256) {
    float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f;
    int w = 0;
    for (; w + 4 <= n_wg; w += 4) {
      g0 += slabs[(long long)w * slab_stride + i];
      g1 += slabs[(long long)(w + 1) * slab_stride + i];
      g2 += slabs[(long long)(w + 2) * slab_stride + i];
      g3 += slabs[(long long)(w + 3) * slab_stride + i];
    }
    for (; w < n_wg; ++w) g0 += slabs[(long long)w * slab_stride + i];
    const float g = (g0 + g1) + (g2 + g3);
    if (grads_out) {          // reduce-only: RCCL takes it from here
      grads_out[i] = g;
      continue;
    }
    if (i == nparam) {
      *loss_out = g;
      continue;
    }
    float p = master[i], mi = m[i], vi = v[i];
    adam_update(p, mi, vi, g, lr, beta1, beta2, eps, corr1, corr2);
    m[i] = mi;
    v[i] = vi;
    master[i] = p;
    const u16 wb = f2bf(p);
    bfmirror[i] = wb;
    if (wimg) wimg_write_gen(wimg, inp, hid, cpad, i, wb);
  }
  // advance the Adam step counter in-kernel: every WG read t_dev at
  // entry (the last-done WG writes only after all WGs passed their
  // read), saving the separate 1-thread bump kernel (~4.7 us/launch
  // of pure launch overhead per step)
  if (threadIdx.x == 0) {
    const unsigned done = atomicAdd(done_counter, 1u) + 1u;
    if (done == gridDim.x) {
      *done_counter = 0u;
      if (!grads_out) *t_dev = (int)t_new;
    }
  }
}

// ---------------------------------------------------------------------------
// generalized fused predict: standardize + fwd + argmax (+softmax)
// ---------------------------------------------------------------------------

// What the predict epilogue needs besides its fp32 output matrix, per
// head. The classifier writes the argmax to int preds[B] (and softmax
// probabilities to the optional out [B][cls]); the regression head writes
// out[row][c] = z * y_scale[c] + y_mean[c], the target de-standardization
// fused into the epilogue, into out [B][ldo], ldo >= cls. The classifier's
// argument list (int* preds, float* probs) stays what it was.
struct RegAffine {
  const float* y_mean;   // [cls]
  const float* y_scale;  // [cls]
  int ldo;
};
template <int HEAD> struct predict_aux { typedef int* __restrict__ type; };
template <> struct predict_aux<HEAD_REG> { typedef RegAffine type; };

template <int HID, int RT, int CP, int HEAD = HEAD_XENT>
__global__ void __launch_bounds__(512)
mlp_predict_gen_kernel(const float* __restrict__ X,  // [B][draw] raw fp32
                       int B, int draw, int inp, int cls,
                       const float* __restrict__ mean,
                       const float* __restrict__ invstd,
                       const u16* __restrict__ wimg,
                       const float* __restrict__ master,  // biases
                       typename predict_aux<HEAD>::type aux,
                       float* __restrict__ out) {
  using G = GG<HID, RT, CP>;
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

  // fwd1 with standardize-on-load, K streamed
  f32x4 acc1[G::SLOTS];
  #pragma unroll
  for (int s = 0; s < G::SLOTS; ++s) acc1[s] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nkt = (inp + G::TK - 1) / G::TK;
  u16 (*Xs0)[G::XSS] = L.Xs(0);
  u16 (*W1T0)[G::W1S] = L.W1T(0);
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * G::TK;
    for (int i = tid; i < RT * G::TK; i += G::BLOCK) {
      const int r = i / G::TK, j = i % G::TK;
      const int c = k0 + j;
      float v = 0.f;
      if (row0 + r < B && c < draw) {
        v = (X[(row0 + r) * draw + c] - mean[c]) * invstd[c];
      }
      Xs0[r][j] = f2bf(v);
    }
    load_w1t_tile(L, 0, wimg, inp, k0, min(G::TK, inp - k0));
    __syncthreads();
    #pragma unroll
    for (int s = 0; s < G::SLOTS; ++s) {
      const int t = wave + G::WAVES * s;
      if (t < G::NT1) {
        const int mt = t % (HID / 16);
        const int rt = t / (HID / 16);
        f32x4 acc = acc1[s];
        #pragma unroll
        for (int ks = 0; ks < G::TK / 32; ++ks) {
          const bf16x8 a = *(const bf16x8*)&W1T0[mt * 16 + lr][ks * 32 + lg * 8];
          const bf16x8 b = *(const bf16x8*)&Xs0[rt * 16 + lr][ks * 32 + lg * 8];
          acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
        }
        acc1[s] = acc;
      }
    }
    __syncthreads();
  }
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

  // regression: this lane's de-standardization pairs, fetched once ahead
  // of the MFMAs (index clamped instead of branched; c >= cls never stores)
  [[maybe_unused]] float ysc[G::NCT][4], ymn[G::NCT][4];
  if constexpr (HEAD == HEAD_REG) {
    #pragma unroll
    for (int ct = 0; ct < G::NCT; ++ct) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = min(ct * 16 + lg * 4 + r, cls - 1);
        ysc[ct][r] = aux.y_scale[c];
        ymn[ct][r] = aux.y_mean[c];
      }
    }
  }

  // fwd2 + argmax / softmax (or the regression outputs) over NCT class tiles
  for (int t2 = wave; t2 < RT / 16; t2 += G::WAVES) {
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
    if constexpr (HEAD == HEAD_REG) {
      #pragma unroll
      for (int ct = 0; ct < G::NCT; ++ct) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = ct * 16 + lg * 4 + r;
          if (c < cls && row0 + row < B) {
            out[(row0 + row) * aux.ldo + c] =
                (acc[ct][r] + L.b2s[c]) * ysc[ct][r] + ymn[ct][r];
          }
        }
      }
    } else {
      int* __restrict__ preds = aux;
      float* __restrict__ probs = out;
      float best;
      int bcol;
      float logit[G::NCT][4];
      head_logits<G::NCT>(logit, acc, L.b2s, cls, lg);
      head_argmax<G::NCT>(logit, cls, lg, best, bcol);
      if (lg == 0 && row0 + row < B) preds[row0 + row] = bcol;
      if (probs != nullptr) {
        float e[G::NCT][4];
        const float rs = fast_rcp(head_exp_sum<G::NCT>(e, logit, best, cls, lg));
        #pragma unroll
        for (int ct = 0; ct < G::NCT; ++ct) {
          #pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int c = ct * 16 + lg * 4 + r;
            if (c < cls && row0 + row < B) probs[(row0 + row) * cls + c] = e[ct][r] * rs;
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// generalized Adam (DP path): grid-strided over a runtime param count.
// The step counter is advanced by a separate 1-thread kernel launched
// AFTER this one (stream-ordered) so every WG sees the same t.
// ---------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
adam_step_gen_kernel(float* __restrict__ master, u16* __restrict__ bfmirror,
                     const float* __restrict__ grads, float* __restrict__ m,
                     float* __restrict__ v, const int* __restrict__ t_dev,
                     int nparam, int inp, int hid, int cpad,
                     float lr, float beta1, float beta2, float eps,
                     u16* __restrict__ wimg) {
  float corr1, corr2;
  adam_bias_corr(beta1, beta2, (float)(*t_dev + 1), corr1, corr2);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < nparam; i += gridDim.x * 256) {
    float p = master[i], mi = m[i], vi = v[i];
    adam_update(p, mi, vi, grads[i], lr, beta1, beta2, eps, corr1, corr2);
    m[i] = mi;
    v[i] = vi;
    master[i] = p;
    const u16 wb = f2bf(p);
    bfmirror[i] = wb;
    if (wimg) wimg_write_gen(wimg, inp, hid, cpad, i, wb);
  }
}

__global__ void bump_t_kernel(int* __restrict__ t_dev) { ++(*t_dev); }

}  // namespace gen

// ---------------------------------------------------------------------------
// host launchers (extern "C"; stream-ordered, capture-safe)
// ---------------------------------------------------------------------------

namespace {

template <int HID, int RT, int CP, int HEAD>
int launch_step_gen_t(const unsigned short* Xbf, const head_target_t<HEAD>* y,
                      int B, int inp, int cls, const unsigned short* wimg,
                      const float* master, float* slabs, int slab_stride,
                      int max_slabs, float invBtot, hipStream_t stream) {
  using G = gen::GG<HID, RT, CP>;
  constexpr auto kernel = gen::mlp_step_gen_kernel<HID, RT, CP, HEAD>;
  const int blocks = (B + RT - 1) / RT;
  if (blocks > max_slabs) return -1;
  if (ensure_dynamic_lds<kernel>(G::TOTAL) != 0) return -2;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(G::BLOCK), G::TOTAL, stream, Xbf,
                     y, B, inp, cls, wimg, master, slabs, slab_stride, invBtot);
  return 0;
}

template <int HID, int RT, int CP, int HEAD>
int launch_predict_gen_t(const float* X, int B, int draw, int inp, int cls,
                         const float* mean, const float* invstd,
                         const unsigned short* wimg, const float* master,
                         typename gen::predict_aux<HEAD>::type aux, float* out,
                         hipStream_t stream) {
  using G = gen::GG<HID, RT, CP>;
  constexpr auto kernel = gen::mlp_predict_gen_kernel<HID, RT, CP, HEAD>;
  if (ensure_dynamic_lds<kernel>(G::TOTAL) != 0) return -2;
  const int blocks = (B + RT - 1) / RT;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(G::BLOCK), G::TOTAL, stream, X, B,
                     draw, inp, cls, mean, invstd, wimg, master, aux, out);
  return 0;
}

// what both dispatchers refuse before they look at the table; n_out is the
// head's class or target count
bool gen_args_ok(int B, int inp, int hid, int n_out) {
  return B >= 1 && n_out >= 1 && n_out <= 32 &&
         GenGeometry{inp, hid, GenGeometry::cpad_for(n_out)}.ok();
}

// The two dispatchers are the only users of TABULAR_GEN_INSTANTIATIONS and
// the only callers of launch_*_gen_t: a kernel is compiled if and only if
// the table has its row.
template <int HEAD>
int dispatch_step_gen(const unsigned short* Xbf, const head_target_t<HEAD>* y,
                      int B, int inp, int hid, int n_out, int rt,
                      const unsigned short* wimg, const float* master,
                      float* slabs, int slab_stride, int max_slabs,
                      float invBtot, hipStream_t stream) {
  if (!gen_args_ok(B, inp, hid, n_out)) return -3;
  const int cpad = GenGeometry::cpad_for(n_out);
  #define STEP_ROW(H, R, C, PREDICT)                                          \
    if (hid == H && rt == R && cpad == C)                                     \
      return launch_step_gen_t<H, R, C, HEAD>(Xbf, y, B, inp, n_out, wimg,    \
                                              master, slabs, slab_stride,     \
                                              max_slabs, invBtot, stream);
  TABULAR_GEN_INSTANTIATIONS(STEP_ROW)
  #undef STEP_ROW
  return -3;
}

template <int HEAD>
int dispatch_predict_gen(const float* X, int B, int draw, int inp, int hid,
                         int n_out, const float* mean, const float* invstd,
                         const unsigned short* wimg, const float* master,
                         typename gen::predict_aux<HEAD>::type aux, float* out,
                         hipStream_t stream) {
  if (!gen_args_ok(B, inp, hid, n_out) || draw < 1 || draw > inp) return -3;
  const int cpad = GenGeometry::cpad_for(n_out);
  #define PREDICT_ROW(H, R, C, PREDICT)                                       \
    if constexpr (PREDICT) {                                                  \
      if (hid == H && cpad == C)                                              \
        return launch_predict_gen_t<H, R, C, HEAD>(X, B, draw, inp, n_out,    \
                                                   mean, invstd, wimg, master, \
                                                   aux, out, stream);         \
    }
  TABULAR_GEN_INSTANTIATIONS(PREDICT_ROW)
  #undef PREDICT_ROW
  return -3;
}

}  // namespace

extern "C" {

int launch_mlp_step_gen(const unsigned short* Xbf, const int* y, int B, int inp,
                        int hid, int cls, int rt, const unsigned short* wimg,
                        const float* master, float* slabs, int slab_stride,
                        int max_slabs, float invBtot, hipStream_t stream) {
  return dispatch_step_gen<HEAD_XENT>(Xbf, y, B, inp, hid, cls, rt, wimg, master,
                                      slabs, slab_stride, max_slabs, invBtot,
                                      stream);
}

// a regressor has no specialized kernels: every shape lands here
int launch_mlp_step_reg_gen(const unsigned short* Xbf, const float* Yt, int B,
                            int inp, int hid, int targets, int rt,
                            const unsigned short* wimg, const float* master,
                            float* slabs, int slab_stride, int max_slabs,
                            float invBtot, hipStream_t stream) {
  return dispatch_step_gen<HEAD_REG>(Xbf, Yt, B, inp, hid, targets, rt, wimg,
                                     master, slabs, slab_stride, max_slabs,
                                     invBtot, stream);
}

int launch_reduce_adam_gen(const float* slabs, int n_wg, int slab_stride,
                           int inp, int hid, int cpad, float* master,
                           unsigned short* bfmirror, float* m, float* v,
                           int* t_dev, float* loss_out, float lr, float beta1,
                           float beta2, float eps, unsigned short* wimg,
                           float* grads_out, unsigned* done_counter,
                           hipStream_t stream) {
  const GenGeometry g{inp, hid, cpad};
  if (!g.ok() || n_wg < 1 || slab_stride < g.min_slab_stride()) return -3;
  const int nparam = (int)g.nparam();
  int blocks = (nparam + 255) / 256;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(gen::reduce_adam_gen_kernel, dim3(blocks), dim3(256), 0,
                     stream, slabs, n_wg, slab_stride, nparam, inp, hid, cpad,
                     master, bfmirror, m, v, t_dev, loss_out, lr, beta1, beta2,
                     eps, wimg, grads_out, done_counter);
  return 0;
}

int launch_mlp_predict_gen(const float* X, int B, int draw, int inp, int hid,
                           int cls, const float* mean, const float* invstd,
                           const unsigned short* wimg, const float* master,
                           int* preds, float* probs, hipStream_t stream) {
  return dispatch_predict_gen<HEAD_XENT>(X, B, draw, inp, hid, cls, mean, invstd,
                                         wimg, master, preds, probs, stream);
}

int launch_mlp_predict_reg_gen(const float* X, int B, int draw, int inp, int hid,
                               int targets, const float* mean,
                               const float* invstd, const unsigned short* wimg,
                               const float* master, const float* y_mean,
                               const float* y_scale, float* out, int ldo,
                               hipStream_t stream) {
  if (ldo < targets) return -3;
  return dispatch_predict_gen<HEAD_REG>(X, B, draw, inp, hid, targets, mean,
                                        invstd, wimg, master,
                                        gen::RegAffine{y_mean, y_scale, ldo}, out,
                                        stream);
}

void launch_adam_step_gen(float* master, unsigned short* bfmirror,
                          const float* grads, float* m, float* v, int* t_dev,
                          int nparam, int inp, int hid, int cpad, float lr,
                          float beta1, float beta2, float eps,
                          unsigned short* wimg, hipStream_t stream) {
  int blocks = (nparam + 255) / 256;
  if (blocks > 512) blocks = 512;
  hipLaunchKernelGGL(gen::adam_step_gen_kernel, dim3(blocks), dim3(256), 0,
                     stream, master, bfmirror, grads, m, v, t_dev, nparam, inp,
                     hid, cpad, lr, beta1, beta2, eps, wimg);
  hipLaunchKernelGGL(gen::bump_t_kernel, dim3(1), dim3(1), 0, stream, t_dev);
}

}  // extern "C"
