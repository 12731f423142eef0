// LDS geometry and cooperative tile loaders of the generalized tabular
// kernels, shared by tabular_gen.hip (step, predict) and tabular_eval.hip
// (evaluation): the GG<> carve and the loaders that fill it. Device code
// only; what a kernel does with the tiles stays in the kernel.
#pragma once

#include <hip/hip_runtime.h>

#include "tabular_common.h"

namespace gen {

constexpr int A16(int x) { return (x + 15) & ~15; }
constexpr int IMAX(int a, int b) { return a > b ? a : b; }

// Geometry: LDS layout + tile bookkeeping, all from <HID, RT, CP>.
template <int HID_, int RT_, int CP_ = 16>
struct GG {
  static constexpr int HID = HID_;
  static constexpr int RT = RT_;        // batch rows per workgroup
  // k-tile over the input width; the widest hidden's W1T tile would
  // not fit double-buffered at TK=64, so it streams narrower tiles
  // (measured -14% at the hid=256 instantiation)
  static constexpr int TK = (HID_ >= 256) ? 32 : 64;
  static constexpr int CPAD = CP_;      // classes padded to MFMA tiles (16/32)
  static constexpr int NCT = CPAD / 16; // class tiles in the fwd2 head
  static_assert(CPAD == 16 || CPAD == 32, "classifier head: 16 or 32 classes");
  static constexpr int WAVES = 8;
  static constexpr int BLOCK = WAVES * 64;

  // LDS row strides (u16 elems), +8 keeps b128 alignment w/ distinct
  // bank slots per row (same scheme as tabular_kernels.hip XS/HS/TS/WS)
  static constexpr int XSS = TK + 8;    // Xs tile   [RT][XSS]
  static constexpr int XTS = RT + 8;    // XT tile   [TK][XTS]   (shares xbuf)
  static constexpr int W1S = TK + 8;    // W1T tile  [HID][W1S]
  static constexpr int HSS = HID + 8;   // Hs        [RT][HSS]
  static constexpr int HTS = RT + 8;    // HT        [HID][HTS]
  static constexpr int DLS = 40;        // DLs       [RT][40]   (K-pad to 32)
  static constexpr int DTS = RT + 8;    // DLT       [CPAD][DTS]
  static constexpr int DHS = RT + 8;    // DHT       [HID][DHS]
  static constexpr int W2S = 40;        // W2s       [HID][40]  (K-pad to 32)
  static constexpr int W2T = HID + 8;   // W2T       [CPAD][W2T]
  // per-row-tile partial sums (f32 elems): part [RT/16][PS], one row per
  // 16-row tile holding its db1 [HID], db2 [CPAD] and loss [1]
  static constexpr int PS = HID + CPAD + 1;

  // streamed-tile buffer sizes (u16 elems, ONE buffer each)
  static constexpr int XBUF1 = IMAX(RT * XSS, TK * XTS);
  static constexpr int W1B1 = HID * W1S;

  static constexpr int layout_total(int nxb) {
    int o = A16(nxb * XBUF1 * 2);
    o = A16(o + nxb * W1B1 * 2);
    o = A16(o + RT * HSS * 2);
    o = A16(o + HID * HTS * 2);
    o = A16(o + RT * DLS * 2);
    o = A16(o + CPAD * DTS * 2);
    o = A16(o + HID * DHS * 2);
    o = A16(o + HID * W2S * 2);
    o = A16(o + CPAD * W2T * 2);
    o = A16(o + (RT / 16) * PS * 4);
    o = A16(o + HID * 4);
    return A16(o + CPAD * 4);
  }

  // double-buffer the k-streamed tiles (Xs/W1T in fwd1, XT in dW1)
  // whenever the carve still fits in the CU's 160 KB: the next tile's
  // cooperative load then overlaps the current tile's MFMAs, hiding
  // the L2/HBM round trip that otherwise serializes each k step
  static constexpr bool DB = layout_total(2) <= 160 * 1024;
  static constexpr int NXB = DB ? 2 : 1;

  static constexpr int O_XB = 0;
  static constexpr int O_W1 = A16(O_XB + NXB * XBUF1 * 2);
  static constexpr int O_HS = A16(O_W1 + NXB * W1B1 * 2);
  static constexpr int O_HT = A16(O_HS + RT * HSS * 2);
  static constexpr int O_DL = A16(O_HT + HID * HTS * 2);
  static constexpr int O_DT = A16(O_DL + RT * DLS * 2);
  static constexpr int O_DH = A16(O_DT + CPAD * DTS * 2);
  static constexpr int O_2S = A16(O_DH + HID * DHS * 2);
  static constexpr int O_2T = A16(O_2S + HID * W2S * 2);
  static constexpr int O_PT = A16(O_2T + CPAD * W2T * 2);    // part [RT/16][PS] f32
  static constexpr int O_B1 = A16(O_PT + (RT / 16) * PS * 4);  // b1 stage [HID]
  static constexpr int O_B2 = A16(O_B1 + HID * 4);           // b2 stage [CPAD]
  static constexpr int TOTAL = A16(O_B2 + CPAD * 4);
  static_assert(TOTAL == layout_total(NXB), "layout helper out of sync");

  static constexpr int NT1 = (HID / 16) * (RT / 16);  // fwd1 / dH D tiles
  static constexpr int SLOTS = (NT1 + WAVES - 1) / WAVES;

  static_assert(HID % 16 == 0, "HID must be a multiple of 16");
  static_assert(RT % 32 == 0, "RT must be a multiple of 32");
  static_assert(TOTAL <= 160 * 1024, "LDS carve exceeds 160 KB");

  // What the per-tile partial rows cost over the three accumulators they
  // replaced (db1 [HID], db2 [CPAD] and four loss slots, each 16-aligned):
  // under 3,104 bytes everywhere (the whole of part at <64,128,32>), the
  // largest carve (<256,32,32>) stays under 151,064 bytes, every geometry
  // that double-buffered still does, and as many workgroups fit a CU's
  // 160 KB as before.
  static constexpr int PART_BYTES = (RT / 16) * PS * 4;
  static constexpr int PART_EXTRA = A16(PART_BYTES) - (HID * 4 + CPAD * 4 + 16);
  static_assert(PART_BYTES <= 3104 && PART_EXTRA <= 3104, "partial rows grew");
  static_assert(TOTAL <= 151064, "largest carve grew");
  static_assert(DB || layout_total(2) - PART_EXTRA > 160 * 1024,
                "partial rows cost a geometry its double buffer");
  static_assert((160 * 1024) / TOTAL == (160 * 1024) / (TOTAL - PART_EXTRA),
                "partial rows cost a workgroup per CU");

  char* smem_;
  u16 (*Hs)[HSS];
  u16 (*HT)[HTS];
  u16 (*DLs)[DLS];
  u16 (*DLT)[DTS];
  u16 (*DHT)[DHS];
  u16 (*W2s)[W2S];
  u16 (*W2Tt)[W2T];
  float (*part)[PS];
  float* b1s;
  float* b2s;

  __device__ __forceinline__ u16 (*Xs(int b))[XSS] {
    return (u16(*)[XSS])(smem_ + O_XB + b * XBUF1 * 2);
  }
  __device__ __forceinline__ u16 (*XT(int b))[XTS] {
    return (u16(*)[XTS])(smem_ + O_XB + b * XBUF1 * 2);
  }
  __device__ __forceinline__ u16 (*W1T(int b))[W1S] {
    return (u16(*)[W1S])(smem_ + O_W1 + b * W1B1 * 2);
  }

  __device__ __forceinline__ void carve(char* smem) {
    smem_ = smem;
    Hs = (u16(*)[HSS])(smem + O_HS);
    HT = (u16(*)[HTS])(smem + O_HT);
    DLs = (u16(*)[DLS])(smem + O_DL);
    DLT = (u16(*)[DTS])(smem + O_DT);
    DHT = (u16(*)[DHS])(smem + O_DH);
    W2s = (u16(*)[W2S])(smem + O_2S);
    W2Tt = (u16(*)[W2T])(smem + O_2T);
    part = (float(*)[PS])(smem + O_PT);
    b1s = (float*)(smem + O_B1);
    b2s = (float*)(smem + O_B2);
  }
};

// (packed global weight-image layout and its Adam-phase store:
// tabular_common.h wimg_w2s_off / wimg_w2t_off / wimg_write_gen)

// ---------------------------------------------------------------------------
// cooperative LDS loaders (all BLOCK threads)
// ---------------------------------------------------------------------------

// Xs tile: rows of this WG's chunk, k-columns [k0, k0+kv), zero tail
template <typename G>
__device__ __forceinline__ void load_xs_tile(G& L, int buf,
                                             const u16* __restrict__ Xbf,
                                             int inp, long long row0,
                                             long long Nvalid, int k0, int kv) {
  u16 (*Xs)[G::XSS] = L.Xs(buf);
  for (int i = threadIdx.x; i < G::RT * (G::TK / 8); i += G::BLOCK) {
    const int r = i / (G::TK / 8);
    const int jg = (i % (G::TK / 8)) * 8;
    bf16x8 v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (row0 + r < Nvalid && jg < kv) {
      v = *(const bf16x8*)&Xbf[(row0 + r) * inp + k0 + jg];
    }
    *(bf16x8*)&Xs[r][jg] = v;
  }
}

// XT tile: transposed image of the same chunk/k-tile (dW1's B operand)
template <typename G>
__device__ __forceinline__ void load_xt_tile(G& L, int buf,
                                             const u16* __restrict__ Xbf,
                                             int inp, long long row0,
                                             long long Nvalid, int k0, int kv) {
  u16 (*XT)[G::XTS] = L.XT(buf);
  for (int i = threadIdx.x; i < G::RT * (G::TK / 8); i += G::BLOCK) {
    const int r = i / (G::TK / 8);
    const int jg = (i % (G::TK / 8)) * 8;
    bf16x8 v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (row0 + r < Nvalid && jg < kv) {
      v = *(const bf16x8*)&Xbf[(row0 + r) * inp + k0 + jg];
    }
    #pragma unroll
    for (int j = 0; j < 8; ++j) XT[jg + j][r] = (u16)v[j];
  }
}

// W1T k-tile from the packed global image (row-major [HID][inp])
template <typename G>
__device__ __forceinline__ void load_w1t_tile(G& L, int buf,
                                              const u16* __restrict__ wimg,
                                              int inp, int k0, int kv) {
  u16 (*W1T)[G::W1S] = L.W1T(buf);
  for (int i = threadIdx.x; i < G::HID * (G::TK / 8); i += G::BLOCK) {
    const int h = i / (G::TK / 8);
    const int jg = (i % (G::TK / 8)) * 8;
    bf16x8 v = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (jg < kv) v = *(const bf16x8*)&wimg[h * inp + k0 + jg];
    *(bf16x8*)&W1T[h][jg] = v;
  }
}

// whole W2 images (small): W2s [HID][40] from [HID][32]; W2T [16][HID+8]
template <typename G>
__device__ __forceinline__ void load_w2_images(const G& L, const u16* __restrict__ wimg,
                                               int inp) {
  const u16* w2s = wimg + wimg_w2s_off(G::HID, inp);
  const u16* w2t = wimg + wimg_w2t_off(G::HID, inp);
  for (int i = threadIdx.x; i < G::HID * 4; i += G::BLOCK) {
    const int h = i / 4, jg = (i % 4) * 8;
    *(bf16x8*)&L.W2s[h][jg] = *(const bf16x8*)&w2s[h * 32 + jg];
  }
  for (int i = threadIdx.x; i < G::CPAD * (G::HID / 8); i += G::BLOCK) {
    const int c = i / (G::HID / 8), jg = (i % (G::HID / 8)) * 8;
    *(bf16x8*)&L.W2Tt[c][jg] = *(const bf16x8*)&w2t[c * G::HID + jg];
  }
}

}  // namespace gen
