// CDNA4 (gfx950 / MI355X) kernels for the default tabular hot path.
//
// Kernel set of SURVEY.md §2c (net-new designs; the reference
// unionai-oss/unionml is pure Python and has no kernels):
//   - standardize_fit / standardize_apply : per-column (x-mean)*invstd, fp32 -> bf16
//   - mlp_step        : fused fwd+bwd of the digits MLP
//                       (IN=64 -> HID=32 relu -> CLS=10 softmax/xent) adding
//                       fp32 grads + loss onto a zeroed buffer with global
//                       atomics. No training path launches it; only the
//                       kernel tests and benchmarks/probe_steps.py do.
//   - mlp_step_fused  : fwd+bwd + cross-workgroup slab reduction + Adam in
//                       ONE launch (the default single-GPU engine). With
//                       grads_out it stops after the reduction: that is the
//                       DP path and the benchmark's stepwise engine, where
//                       the RCCL all-reduce of the 2.6k-float grad buffer
//                       sits between it and adam_step
//   - adam_step       : single-block fused Adam on the flat fp32 master
//   - mlp_train_steps : single-GPU flagship — a persistent single-workgroup
//                       kernel running N optimizer steps in ONE launch with
//                       bf16 weights, fp32 master and Adam moments resident
//                       in LDS across steps; only minibatch rows stream from
//                       HBM. Zero per-step launches.
//   - mlp_predict     : fused standardize + fwd + argmax (serving hot path)
//
// Fragment-oriented design (2nd iteration, after PMC analysis — the first
// scalar-read version spent 59 % of wave cycles parked on LDS latency):
// every MFMA operand fragment is ONE ds_read_b128 or, where the K axis runs
// down the image's rows, TWO ds_read_b64_tr_b16. An MFMA fragment needs
// its K axis contiguous in the lane's registers, so the forward GEMMs and dH
// are oriented (plain or transposed output) such that both operands have a
// row-major LDS image whose rows run along K. The weight-grad GEMMs sum over
// the batch row, the ROW axis of the very same images (X, H, dLogits, dH):
// they read them with the transposed read (tr_read_k8 below), which hands
// a lane eight K-consecutive elements of one column. Every tile has ONE
// image. (Until r08 each of the four had a second, transposed copy written
// with 2-byte scatter stores: profiles/r08_lds_transposed_reads.md.)
//
//   H^T  = W1T @ B(Xs)        A=W1T[h][k_in]   B-img = Xs[row][in]
//   L^T  = W2T @ B(Hs)        A=W2T[c][k_h]    B-img = Hs[row][h]
//   dH^T = W2s @ B(DLs)       A=W2s[h][k_c]    B-img = DLs[row][c]
//   dW1^T= DH^T @ B(X^T)      A=tr(DHs[k_row][h])  B=tr(Xs[k_row][in])
//   dW2  = H^T  @ B(DL^T)     A=tr(Hs[k_row][h])   B=tr(DLs[k_row][c])
//
// MFMA: __builtin_amdgcn_mfma_f32_16x16x32_bf16 (gfx950 2xK form), fp32
// accumulate. Fragment mapping (verified on hardware by
// tests/test_gpu_kernels.py with asymmetric operands):
//   A[16x32]:  lane l holds A[l&15][(l>>4)*8 + i], i = 0..7
//   B[32x16]:  lane l holds B[(l>>4)*8 + i][l&15]
//   C/D[16x16]: lane l, reg r holds D[(l>>4)*4 + r][l&15]
//
// LDS row strides are multiples of 16 B (b128 alignment, guide §6 G17) with
// bank-slot-distinct row offsets (guide §6 G4); DHs, stored 8 bytes at a time
// and read only transposed, has 72-byte rows (conflict-free stores; computed
// bank figures: docs/kernels.md "LDS layout"). No fp32 division in device
// code (v_div_scale sequences dominated the first version) — v_rcp instead.
// All launches are stream-ordered and hipGraph-capturable (guide G9); step
// counters live in device memory so Adam bias correction is exact under
// graph replay.

#include <hip/hip_runtime.h>

#include "tabular_common.h"

// short names for the digits layout (defined once, in tabular_launch.h)
constexpr int IN = DIGITS_IN, HID = DIGITS_HID, CLS = DIGITS_CLS;
constexpr int CPAD = DIGITS_CPAD;   // CLS padded to one MFMA tile
#define ROWS 128         // batch rows per workgroup / per chunk
#define WAVES 8
#define BLOCK (WAVES * 64)

// LDS strides in bf16 elements (row-major [rows][stride]):
constexpr int XS = DIGITS_XS;   // Xs/W1T [*][72]  (144 B rows)
#define HS 40            // Hs/DLs [ROWS][40] (80 B rows)
#define DHS 36           // DHs [ROWS][36] (72 B rows: never read by rows)
constexpr int WS = DIGITS_WS;   // W2s/W2T [*][40] (80 B rows; K-padded zeros)

// ---------------------------------------------------------------------------
// standardize
// ---------------------------------------------------------------------------

// fast path (256 % D == 0): coalesced row-major accumulation — thread t
// owns column t%D and row-group t/D, so each iteration reads 256
// consecutive floats; per-column partials reduce in LDS and land in a
// double scratch via atomics; a tiny finalize kernel produces
// mean/invstd. (The column-per-workgroup variant below read the matrix
// with stride D — 181 µs for digits vs ~8 µs here.)
extern "C" __global__ void __launch_bounds__(256)
standardize_fit_fast_kernel(const float* __restrict__ X, long long N, int D,
                            double* __restrict__ scratch /* [2*D] zeroed */) {
  const int tid = threadIdx.x;
  const int col = tid % D;
  const int rg = tid / D;
  const int rpi = 256 / D;                 // rows per iteration per WG
  double s = 0.0, s2 = 0.0;
  for (long long r = (long long)blockIdx.x * rpi + rg; r < N;
       r += (long long)gridDim.x * rpi) {
    const double v = (double)X[r * D + col];
    s += v;
    s2 += v * v;
  }
  __shared__ double ls[256], ls2[256];
  ls[tid] = s;
  ls2[tid] = s2;
  __syncthreads();
  for (int off = 128; off >= D; off >>= 1) {
    if (tid < off && tid + off < 256) {
      ls[tid] += ls[tid + off];
      ls2[tid] += ls2[tid + off];
    }
    __syncthreads();
  }
  if (tid < D) {
    atomicAdd(&scratch[col], ls[tid]);
    atomicAdd(&scratch[D + col], ls2[tid]);
  }
}

extern "C" __global__ void __launch_bounds__(256)
standardize_fit_finalize_kernel(const double* __restrict__ scratch, long long N,
                                int D, float* __restrict__ mean,
                                float* __restrict__ invstd, float eps) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= D) return;
  const double m = scratch[col] / (double)N;
  const double var = scratch[D + col] / (double)N - m * m;
  mean[col] = (float)m;
  invstd[col] = (float)(1.0 / sqrt(var > 0.0 ? var + (double)eps : (double)eps));
}

extern "C" __global__ void __launch_bounds__(256)
standardize_fit_kernel(const float* __restrict__ X, long long N, int D,
                       float* __restrict__ mean, float* __restrict__ invstd,
                       float eps) {
  const int col = blockIdx.x;
  if (col >= D) return;
  double s = 0.0, s2 = 0.0;
  for (long long r = threadIdx.x; r < N; r += blockDim.x) {
    const double v = (double)X[r * D + col];
    s += v;
    s2 += v * v;
  }
  __shared__ double ls[256], ls2[256];
  ls[threadIdx.x] = s;
  ls2[threadIdx.x] = s2;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      ls[threadIdx.x] += ls[threadIdx.x + off];
      ls2[threadIdx.x] += ls2[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double m = ls[0] / (double)N;
    const double var = ls2[0] / (double)N - m * m;
    mean[col] = (float)m;
    invstd[col] = (float)(1.0 / sqrt(var > 0.0 ? var + (double)eps : (double)eps));
  }
}

// Dout >= D: output rows are Dout wide (extra columns untouched — the
// generalized kernels stage features into a zero-padded [N][INP] image)
extern "C" __global__ void __launch_bounds__(256)
standardize_apply_kernel(const float* __restrict__ X, long long n_elems, int D,
                         int Dout,
                         const float* __restrict__ mean,
                         const float* __restrict__ invstd,
                         u16* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_elems;
       i += (long long)gridDim.x * blockDim.x) {
    const int col = (int)(i % D);
    out[(i / D) * Dout + col] = f2bf((X[i] - mean[col]) * invstd[col]);
  }
}

// flat master/grads layout and the per-workgroup slab (tabular_launch.h)
constexpr int OFF_W1 = DIGITS_OFF_W1, OFF_B1 = DIGITS_OFF_B1;
constexpr int OFF_W2 = DIGITS_OFF_W2, OFF_B2 = DIGITS_OFF_B2;
constexpr int NPARAM = DIGITS_NPARAM, OFF_LOSS = NPARAM;
constexpr int SLAB = DIGITS_SLAB;

// ---------------------------------------------------------------------------
// dynamic-LDS carve shared by mlp_step / mlp_train_steps
// ---------------------------------------------------------------------------

#define ALIGN16(x) (((x) + 15) & ~15)
#define C_XS   0
#define C_HS   ALIGN16(C_XS  + ROWS * XS * 2)
#define C_DLS  ALIGN16(C_HS  + ROWS * HS * 2)
#define C_DHS  ALIGN16(C_DLS + ROWS * HS * 2)
#define C_W1T  ALIGN16(C_DHS + ROWS * DHS * 2)
#define C_W2S  ALIGN16(C_W1T + HID * XS * 2)
#define C_W2T  ALIGN16(C_W2S + HID * WS * 2)
#define C_DB1  ALIGN16(C_W2T + CPAD * WS * 2)
#define C_DB2  ALIGN16(C_DB1 + HID * 4)
#define C_LOSS ALIGN16(C_DB2 + CPAD * 4)
#define C_B1S  ALIGN16(C_LOSS + 16)
#define C_B2S  ALIGN16(C_B1S + HID * 4)
// per-wave bias-grad / loss partials of one chunk: [wave][HID + CPAD + 1]
#define NWAVE  (BLOCK / 64)
#define PART   (HID + CPAD + 1)
#define C_PART ALIGN16(C_B2S + CPAD * 4)
#define C_IMG_TOTAL ALIGN16(C_PART + NWAVE * PART * 4)
// steps kernel appends optimizer state after the images:
#define C_MASTER C_IMG_TOTAL
#define C_M    ALIGN16(C_MASTER + NPARAM * 4)
#define C_V    ALIGN16(C_M + NPARAM * 4)
#define C_STEPS_TOTAL ALIGN16(C_V + NPARAM * 4)

struct Lds {
  u16 (*Xs)[XS];
  u16 (*Hs)[HS];
  u16 (*DLs)[HS];
  u16 (*DHs)[DHS];
  u16 (*W1T)[XS];
  u16 (*W2s)[WS];
  u16 (*W2T)[WS];
  float* db1;
  float* db2;
  float* loss;
  float* b1s;   // bias prefetch (fwd chain must not stall on cold HBM)
  float* b2s;
  float* part;  // [NWAVE][PART]: db1 | db2 | loss, one row per wave
};

__device__ __forceinline__ Lds carve(char* smem) {
  Lds L;
  L.Xs = (u16(*)[XS])(smem + C_XS);
  L.Hs = (u16(*)[HS])(smem + C_HS);
  L.DLs = (u16(*)[HS])(smem + C_DLS);
  L.DHs = (u16(*)[DHS])(smem + C_DHS);
  L.W1T = (u16(*)[XS])(smem + C_W1T);
  L.W2s = (u16(*)[WS])(smem + C_W2S);
  L.W2T = (u16(*)[WS])(smem + C_W2T);
  L.db1 = (float*)(smem + C_DB1);
  L.db2 = (float*)(smem + C_DB2);
  L.loss = (float*)(smem + C_LOSS);
  L.b1s = (float*)(smem + C_B1S);
  L.b2s = (float*)(smem + C_B2S);
  L.part = (float*)(smem + C_PART);
  return L;
}

// packed weight-image staging: a persistent global buffer holding the
// THREE LDS images (W1T/W2s/W2T incl. their K-pads) back to back in
// exactly the LDS layout, so the training prologue is one straight
// vectorized copy instead of a per-element transposed gather. Writers:
// the Adam phases (in-kernel and adam_step) and the host on
// init/load_state_dict. Offsets: tabular_launch.h DIGITS_WIMG_*; the
// per-param store: tabular_common.h wimg_write.
//
// Two-phase form: a load loop compiles to load -> wait -> LDS store per
// trip, one cold global round trip each. issue_* puts every vector of this
// thread in flight and returns registers; store_* writes them to LDS after
// the caller has issued ALL its prologue loads, so the prologue waits once.
constexpr int WIMG_VECS = DIGITS_WIMG_N / 8;    // 528 vectors over 512 threads
constexpr int WIMG_TAIL = WIMG_VECS - BLOCK;    // second vector: threads 0..15
static_assert(WIMG_TAIL > 0 && WIMG_TAIL <= BLOCK, "two vectors per thread at most");

struct WimgRegs {
  bf16x8 v0, v1;
};

__device__ __forceinline__ void issue_weight_images_packed(
    WimgRegs& R, const u16* __restrict__ wimg) {
  const bf16x8* src = (const bf16x8*)wimg;
  const int tid = threadIdx.x;
  R.v0 = src[tid];
  // unconditional (threads past the tail re-read their first vector and
  // drop it): a load under a branch made the compiler wait on the spot
  R.v1 = src[tid < WIMG_TAIL ? BLOCK + tid : tid];
}

__device__ __forceinline__ void store_weight_images_packed(const WimgRegs& R,
                                                           const Lds& L) {
  bf16x8* dst = (bf16x8*)&L.W1T[0][0];   // W1T..W2T are contiguous in LDS
  const int tid = threadIdx.x;
  dst[tid] = R.v0;
  if (tid < WIMG_TAIL) dst[BLOCK + tid] = R.v1;
}

// prefetch biases into LDS alongside the other prologue loads — the
// previous launch's agent-scope acquire left L2 cold, so a lazy mid-GEMM
// b1/b2 read would serialize a full HBM round trip into the fwd chain.
// Two-phase as well: this thread's bias element travels in a register
// until the prologue's single wait.
__device__ __forceinline__ float issue_biases(const float* __restrict__ b1,
                                              const float* __restrict__ b2) {
  const int tid = threadIdx.x;
  // unconditional: threads without a bias element re-read b1[0], unused
  const float* p = tid < HID ? b1 + tid : tid < HID + CPAD ? b2 + (tid - HID) : b1;
  return *p;
}

// one word that every thread wants, as a VECTOR load of a uniform address
// (global_load_dword, no cache-policy bit). A plain read of a uniform
// address compiles to a scalar load, which sits on the scalar counter with
// the LDS traffic and gets a wait of its own; a relaxed wavefront-scope
// atomic load is never made scalar, costs nothing more than a plain load,
// and is counted with the other prologue loads.
template <typename T>
__device__ __forceinline__ T uniform_load(const T* p) {
  static_assert(sizeof(T) == 4, "one dword");
  typedef __attribute__((address_space(1))) const T gT;
  return __hip_atomic_load((gT*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

__device__ __forceinline__ void store_biases(float b, const Lds& L) {
  const int tid = threadIdx.x;
  if (tid < HID) L.b1s[tid] = b;
  else if (tid < HID + CPAD) L.b2s[tid - HID] = b;
}

// fill weight images (W1T/W2s/W2T incl. zero K-pads) from bf16 weight arrays
__device__ __forceinline__ void load_weight_images(const Lds& L,
                                                   const u16* __restrict__ W1bf,
                                                   const u16* __restrict__ W2bf) {
  const int tid = threadIdx.x;
  for (int i = tid; i < HID * IN; i += BLOCK) {       // W1T[h][k] = W1[k][h]
    const int h = i / IN, k = i % IN;
    L.W1T[h][k] = W1bf[k * HID + h];
  }
  for (int i = tid; i < HID * 32; i += BLOCK) {       // W2s[h][c], c-pad 16..31 = 0
    const int h = i / 32, c = i % 32;
    L.W2s[h][c] = (c < CPAD) ? W2bf[h * CPAD + c] : (u16)0;
  }
  for (int i = tid; i < CPAD * HID; i += BLOCK) {     // W2T[c][h] = W2[h][c]
    const int c = i / HID, h = i % HID;
    L.W2T[c][h] = W2bf[h * CPAD + c];
  }
}

// cooperative X-chunk load, two-phase like the packed images: thread t
// owns vector t and t + BLOCK of the chunk's ROWS x IN/8 vectors, plus the
// label of the row chunk_fwd_bwd gives it (wave*16 + lane%16; the four
// lane groups of a wave load the same value).
//
// Batch tail: a row at or beyond Nvalid loads from row Nvalid-1 instead
// (always in range: every caller has Nvalid >= 1) and the value is
// replaced after the wait, by zeros for X and by -1 for the label.
// Nothing at or beyond Nvalid is read. The loads are unconditional on
// purpose: a load under `if (row < Nvalid)` merged with a zero default
// made the compiler wait for it on the spot, one exposed round trip.
constexpr int X_VECS = ROWS * (IN / 8) / BLOCK;
static_assert(X_VECS * BLOCK == ROWS * (IN / 8), "whole vectors per thread");

struct XChunkRegs {
  bf16x8 v[X_VECS];
  bool vvalid[X_VECS];
  int label;    // as loaded; chunk_label() applies the tail rule
  bool valid;   // this thread's softmax row is a real batch row
};

__device__ __forceinline__ void issue_label(XChunkRegs& R,
                                            const int* __restrict__ y,
                                            long long row0, long long Nvalid) {
  const int tid = threadIdx.x;
  const long long row = row0 + (tid >> 6) * 16 + (tid & 15);
  R.valid = row < Nvalid;
  R.label = y[R.valid ? row : Nvalid - 1];
}

__device__ __forceinline__ void issue_x_chunk(XChunkRegs& R,
                                              const u16* __restrict__ Xbf,
                                              const int* __restrict__ y,
                                              long long row0, long long Nvalid) {
  const int tid = threadIdx.x;
  #pragma unroll
  for (int u = 0; u < X_VECS; ++u) {
    const int i = tid + u * BLOCK;
    const long long row = row0 + i / (IN / 8);
    const int c = (i % (IN / 8)) * 8;
    R.vvalid[u] = row < Nvalid;
    R.v[u] = *(const bf16x8*)&Xbf[(R.vvalid[u] ? row : Nvalid - 1) * IN + c];
  }
  issue_label(R, y, row0, Nvalid);
}

// the row's label, -1 for a row at or beyond Nvalid
__device__ __forceinline__ int chunk_label(const XChunkRegs& R) {
  return R.valid ? R.label : -1;
}

// Xs row-major, zero batch tail. It is the ONLY image of the chunk's X: fwd1
// reads it by rows, dW1 by transposed reads, so it stays live until every
// wave's dW1 is done.
__device__ __forceinline__ void store_x_chunk(const XChunkRegs& R, const Lds& L) {
  const int tid = threadIdx.x;
  #pragma unroll
  for (int u = 0; u < X_VECS; ++u) {
    const int i = tid + u * BLOCK;
    const int r = i / (IN / 8);
    const int c = (i % (IN / 8)) * 8;
    const bf16x8 v = R.vvalid[u] ? R.v[u] : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    *(bf16x8*)&L.Xs[r][c] = v;
  }
}

// zero DLs K-pad cols [CPAD,32) once per launch (never rewritten): 32 bytes
// per row, as two 16-byte stores; thread t takes half t&1 of row t>>1
__device__ __forceinline__ void zero_dl_pad(const Lds& L) {
  static_assert(2 * ROWS <= BLOCK && CPAD == 16 && (HS * 2) % 16 == 0, "one b128 store per thread");
  const int t = threadIdx.x;
  if (t < 2 * ROWS) *(bf16x8*)&L.DLs[t >> 1][CPAD + (t & 1) * 8] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
}

// four consecutive bf16 of one row-major LDS image row (8-byte aligned: the
// column is a multiple of 4 and the row strides are multiples of 16 bytes)
// as ONE 8-byte store, in place of four 2-byte ones
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
__device__ __forceinline__ void store_bf16x4(u16* p, const u16 (&x)[4]) {
  *(u32x2*)p = (u32x2){(unsigned)x[0] | ((unsigned)x[1] << 16),
                       (unsigned)x[2] | ((unsigned)x[3] << 16)};
}

struct ChunkAcc {
  f32x4 dW1;        // wave's dW1^T tile: h-tile = wave&1, in-tile = wave>>1
  f32x4 dW2;        // waves 0-1: dW2 tile (h-tile = wave)
};

// one 128-row chunk: fwd + bwd, accumulating weight grads in acc_io. b1/b2
// point at fp32 biases in LDS, 16-byte aligned, b2 padded to CPAD floats.
// label/valid describe this thread's softmax row (wrow + lr) and come from
// issue_x_chunk: the label was loaded with the chunk's X, so no global
// read sits inside the softmax chain.
//
// Bias grads and loss, two forms:
//   SINGLE = false (many chunks per step, mlp_train_steps_kernel): they are
//     accumulated in L.db1 / L.db2 / L.loss, which the caller zeroes per
//     step, and the function ends in a workgroup barrier after which the
//     chunk arrays may be refilled.
//   SINGLE = true (the step is this one chunk): the summing wave hands them
//     back in a register instead. Thread t = BIAS_SUM_T0 + i, i < PART, gets
//     in bias_sum entry i of db1 | db2 | loss (PART layout), every other
//     thread 0. L.db1 / L.db2 / L.loss are not touched, and there is NO
//     trailing barrier: each wave returns straight after its last MFMA, so
//     the caller must put a workgroup barrier before it reuses any chunk
//     array.
constexpr int BIAS_SUM_T0 = (NWAVE - 1) * 64;

template <bool SINGLE>
__device__ __forceinline__ void chunk_fwd_bwd(
    const Lds& L, const float* b1, const float* b2,
    const int label, const bool valid, float invBtot, ChunkAcc& acc_io,
    float& bias_sum) {
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, lr = l & 15;
  const int wrow = wave * 16;                       // this wave's 16-row block

  // this lane's bias values, ahead of everything that needs them: the eight
  // b1[mt*16 + lg*4 + r] as two 16-byte reads and the four b2[lg*4 + r] as
  // one (b2 holds CPAD floats, so the read is in range for every lg; the
  // pad is masked in head_logits_padded). They are issued with fwd1's
  // fragment reads and have long arrived where they are added; read where
  // they are used, each cost an LDS round trip inside the dependent chain.
  // The scheduling barriers keep the order bias reads, fragment reads,
  // MFMAs: left to the scheduler the bias reads sink below the MFMAs, next
  // to their adds.
  bf16x8 w1f[HID / 16][IN / 32], xf[IN / 32];
  f32x4 b1v[HID / 16];
  #pragma unroll
  for (int mt = 0; mt < HID / 16; ++mt) b1v[mt] = *(const f32x4*)&b1[mt * 16 + lg * 4];
  const f32x4 b2v = *(const f32x4*)&b2[lg * 4];
  __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
  for (int ks = 0; ks < IN / 32; ++ks) {
    xf[ks] = *(const bf16x8*)&L.Xs[wrow + lr][ks * 32 + lg * 8];
    #pragma unroll
    for (int mt = 0; mt < HID / 16; ++mt) {
      w1f[mt][ks] = *(const bf16x8*)&L.W1T[mt * 16 + lr][ks * 32 + lg * 8];
    }
  }
  __builtin_amdgcn_sched_barrier(0);

  // ---- fwd1: H^T = W1T @ B(Xs);  D: h = mt*16+lg*4+r, row = wrow+lr --------
  // hbits keeps the lane's eight H values: dH below needs exactly these
  // (same h, same row), so it does not read Hs back
  u16 hbits[HID / 16][4];
  f32x4 hacc[HID / 16];
  #pragma unroll
  for (int mt = 0; mt < HID / 16; ++mt) {
    hacc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int ks = 0; ks < IN / 32; ++ks) {
      hacc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w1f[mt][ks], xf[ks], hacc[mt], 0, 0, 0);
    }
  }
  #pragma unroll
  for (int mt = 0; mt < HID / 16; ++mt) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      float hv = hacc[mt][r] + b1v[mt][r];
      hv = hv > 0.f ? hv : 0.f;
      const u16 hb = f2bf(hv);
      hbits[mt][r] = hb;
    }
    store_bf16x4(&L.Hs[wrow + lr][mt * 16 + lg * 4], hbits[mt]);
  }
  // NO __syncthreads here: fwd2 reads only THIS wave's rows of Hs
  // (row = wrow+lr), written by lanes of the same wave — a wave-level
  // LDS drain is sufficient. (dW2's cross-wave reads of Hs are covered by
  // the barrier after dH below.)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- fwd2: L^T = W2T @ B(Hs);  D: c = lg*4+r, row = wrow+lr --------------
  {
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    const bf16x8 a = *(const bf16x8*)&L.W2T[lr][lg * 8];
    const bf16x8 b = *(const bf16x8*)&L.Hs[wrow + lr][lg * 8];
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[0], 0, 0, 0);

    const int row = wrow + lr;

    float logit[1][4], e[1][4];
    head_logits_padded(logit, acc, b2v, CLS, lg);
    const float m = head_row_max<1>(logit);
    const float s = head_exp_sum<1>(e, logit, m, CLS, lg);
    const float rs = fast_rcp(s);
    const float logs = __logf(s);
    float db2_acc[4];
    float loss_acc = 0.f;
    u16 dlbits[4];
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = lg * 4 + r;
      const float dl = valid ? (e[0][r] * rs - (c == label ? 1.f : 0.f)) * invBtot : 0.f;
      const u16 dlb = f2bf(dl);
      dlbits[r] = dlb;
      db2_acc[r] = dl;
      if (valid && c == label) loss_acc = -(logit[0][r] - m - logs) * invBtot;
    }
    store_bf16x4(&L.DLs[row][lg * 4], dlbits);
    // reduce db2/loss over the 16 row-lanes (lr bits) first, then ONE
    // plain store per (wave, class) into this wave's partial row: the
    // waves are summed in fixed order below, so the step is reproducible
    // bit for bit (float LDS atomics landed in arrival order). All five
    // reductions run first, with every lane active (DPP reads its row
    // neighbours' registers); the predicated stores follow in one block.
    #pragma unroll
    for (int r = 0; r < 4; ++r) db2_acc[r] = row_sum16(db2_acc[r]);
    loss_acc = row_sum16(loss_acc);
    // loss_acc now holds the 16-row sum within this lg quarter; fold
    // the four lg groups (lane bits 4,5) too, then one store per wave
    loss_acc = group_sum<16>(loss_acc);
    loss_acc = group_sum<32>(loss_acc);
    if (lr == 0) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) L.part[wave * PART + HID + lg * 4 + r] = db2_acc[r];
      if (l == 0) L.part[wave * PART + HID + CPAD] = loss_acc;
    }
  }
  // NO __syncthreads here either: dH reads only this wave's rows of
  // DLs. Cross-wave consumers (dW2 over all rows of Hs and DLs) wait at the
  // barrier after dH.
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // ---- dH^T = W2s @ B(DLs);  D: h = mt*16+lg*4+r, row = wrow+lr ------------
  {
    float db1_acc[HID / 16][4];
    #pragma unroll
    for (int mt = 0; mt < HID / 16; ++mt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      const bf16x8 a = *(const bf16x8*)&L.W2s[mt * 16 + lr][lg * 8];
      const bf16x8 b = *(const bf16x8*)&L.DLs[wrow + lr][lg * 8];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
      u16 dhbits[4];
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float hv = bf2f(hbits[mt][r]);   // == L.Hs[row][h], this lane's own store
        const float dh = hv > 0.f ? acc[r] : 0.f;
        dhbits[r] = f2bf(dh);
        db1_acc[mt][r] = dh;
      }
      // row-major, the lane's four consecutive h of its row as one store
      store_bf16x4(&L.DHs[wrow + lr][mt * 16 + lg * 4], dhbits);
    }
    // db1[h]: sum this row-block's contribution across the 16 lr lanes.
    // All eight reductions first, no branch between them, then the
    // predicated stores in one block.
    #pragma unroll
    for (int mt = 0; mt < HID / 16; ++mt) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) db1_acc[mt][r] = row_sum16(db1_acc[mt][r]);
    }
    if (lr == 0) {
      #pragma unroll
      for (int mt = 0; mt < HID / 16; ++mt) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          L.part[wave * PART + mt * 16 + lg * 4 + r] = db1_acc[mt][r];
        }
      }
    }
  }
  // DHs + per-wave partials complete; and every wave's Hs and DLs rows, which
  // dW2 reads across waves
  __syncthreads();

  // ---- db1/db2/loss += partials, waves in fixed order. The last wave does
  // it: it has no dW2 tile, so this stays off the longest wave's path ----
  bias_sum = 0.f;
  if (wave == NWAVE - 1 && l < PART) {
    float sum = 0.f;
    #pragma unroll
    for (int w = 0; w < NWAVE; ++w) sum += L.part[w * PART + l];
    if constexpr (SINGLE) {
      // what the accumulating form leaves in the zeroed LDS slot: 0 + sum
      // (kept as written: 0 + (-0) is +0)
      bias_sum = 0.f + sum;
    } else {
      if (l < HID) L.db1[l] += sum;
      else if (l < HID + CPAD) L.db2[l - HID] += sum;
      else L.loss[0] += sum;
    }
  }

  // ---- dW1^T += DH^T @ B(X^T): wave tile (ht = w&1, it = w>>1). K is the
  // batch row, the row axis of DHs and Xs: transposed reads (tr_read_k8,
  // tabular_common.h). Every lane of every wave gets here: EXEC is full. -----
  {
    const int ht = wave & 1, it = wave >> 1;
    // all the reads, then the MFMAs: left in one loop the compiler keeps each
    // k-step's reads behind the previous k-step's MFMA, four LDS round trips
    // in a row
    bf16x8 a[ROWS / 32], b[ROWS / 32];
    #pragma unroll
    for (int ks = 0; ks < ROWS / 32; ++ks) {
      a[ks] = tr_read_k8<DHS, ROWS / 32, HID / 16>(L.DHs, ks, ht, l);
      b[ks] = tr_read_k8<XS, ROWS / 32, IN / 16>(L.Xs, ks, it, l);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = acc_io.dW1;
    #pragma unroll
    for (int ks = 0; ks < ROWS / 32; ++ks) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], b[ks], acc, 0, 0, 0);
    }
    acc_io.dW1 = acc;
  }
  // ---- dW2 += H^T @ B(DL^T): waves 0-1 (h-tile = wave), transposed reads of
  // Hs and of DLs' class columns 0..15. The branch is on the wave index: all
  // 64 lanes take it or none does, so EXEC is full inside. -------------------
  if (wave < 2) {
    bf16x8 a[ROWS / 32], b[ROWS / 32];
    #pragma unroll
    for (int ks = 0; ks < ROWS / 32; ++ks) {
      a[ks] = tr_read_k8<HS, ROWS / 32, HID / 16>(L.Hs, ks, wave, l);
      b[ks] = tr_read_k8<HS, ROWS / 32, CPAD / 16>(L.DLs, ks, 0, l);
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = acc_io.dW2;
    #pragma unroll
    for (int ks = 0; ks < ROWS / 32; ++ks) {
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[ks], b[ks], acc, 0, 0, 0);
    }
    acc_io.dW2 = acc;
  }
  // chunk arrays free for reuse: Xs above all, which dW1 has just read and
  // the caller's next store_x_chunk refills
  if constexpr (!SINGLE) __syncthreads();
}

// flat grads/slab index of entry i of the PART layout (db1 | db2 | loss)
__device__ __forceinline__ int bias_sum_index(int i) {
  return i < HID ? OFF_B1 + i : i < HID + CPAD ? OFF_B2 + (i - HID) : OFF_LOSS;
}

// ---------------------------------------------------------------------------
// per-step kernel (multi-workgroup; grads via global atomics). Kept for the
// kernel tests and benchmarks/probe_steps.py: every training path, DP
// included, runs mlp_step_fused_kernel below.
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(BLOCK)
mlp_step_kernel(const u16* __restrict__ Xbf, const int* __restrict__ y, int B,
                const u16* __restrict__ W1bf, const u16* __restrict__ W2bf,
                const float* __restrict__ master,
                float* __restrict__ grads, float invBtot) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L = carve(smem);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, lr = l & 15;
  const long long row0 = (long long)blockIdx.x * ROWS;

  XChunkRegs xr;
  issue_x_chunk(xr, Xbf, y, row0, B);
  const float bias = issue_biases(master + OFF_B1, master + OFF_B2);
  zero_dl_pad(L);
  load_weight_images(L, W1bf, W2bf);
  store_x_chunk(xr, L);
  store_biases(bias, L);
  __syncthreads();

  ChunkAcc acc;
  acc.dW1 = (f32x4){0.f, 0.f, 0.f, 0.f};
  acc.dW2 = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bias_sum;
  chunk_fwd_bwd<true>(L, L.b1s, L.b2s, chunk_label(xr), xr.valid, invBtot, acc, bias_sum);

  {
    const int ht = wave & 1, it = wave >> 1;
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = ht * 16 + lg * 4 + r;          // D row = h index
      const int in = it * 16 + lr;                 // D col = input feature
      atomicAdd(&grads[OFF_W1 + in * HID + h], acc.dW1[r]);
    }
  }
  if (wave < 2) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = wave * 16 + lg * 4 + r;
      atomicAdd(&grads[OFF_W2 + h * CPAD + lr], acc.dW2[r]);
    }
  }
  // db1 / db2 / loss: the summing wave adds its register
  if (tid >= BIAS_SUM_T0 && tid < BIAS_SUM_T0 + PART) {
    atomicAdd(&grads[bias_sum_index(tid - BIAS_SUM_T0)], bias_sum);
  }
}

// ---------------------------------------------------------------------------
// fully-fused step kernel: fwd + bwd + cross-WG grad reduction + Adam in ONE
// launch. Each workgroup writes its complete partial-grad slab, signals it
// with the slab's epoch tag, waits until every slab of the launch carries
// this launch's tag, then sums ITS stripe of the parameters over all slabs
// and applies Adam to that stripe. The DP path needs the summed grads for
// RCCL: it runs this kernel in reduce-only mode (grads_out) and applies Adam
// afterwards with adam_step_kernel.
//
// The hand-off between the workgroups uses NO agent-scope fence (neither
// buffer_wbl2 nor buffer_inv): it is the write-through form of guide §6 G16,
// first row of the table of hand-offs measured with sc1 loads in place of
// the acquire (one lane of each storing workgroup signals with an sc1 flag
// store for all that workgroup's stores; the consumer polls the flags with
// sc1 loads; the other waves load after a workgroup barrier the polling wave
// joins; hipMalloc memory; one workgroup per CU; 4- and 16-byte stores,
// 4-byte loads). What makes it valid, and has to stay true after any edit:
//   (1) every store to slab memory is an sc1 store (xwg_store/xwg_store4,
//       tabular_common.h): written through, nothing left for a release;
//   (2) every storing wave drains its stores (s_waitcnt vmcnt(0)) and then
//       reaches the workgroup barrier BEFORE lane 0 stores the tag;
//   (3) the tag is stored and polled sc1;
//   (4) every load of a slab byte is an sc1 load (xwg_load) that sits
//       behind the poll and the barrier after it, and every OTHER load of the
//       kernel reads bytes no other workgroup writes in this launch: X and
//       the labels are never written; wimg / W1bf / W2bf and the biases in
//       master are written only in the Adam phase, which no workgroup enters
//       before ALL have published, i.e. after all have finished their
//       prologue loads; the prefetched master/m/v stripe is written only by
//       the workgroup that reads it; counter and t_dev are loaded by EVERY
//       thread (one plain vector load each, issued with the prologue loads)
//       and every wave has consumed its two words before it reaches the
//       FIRST barrier of its workgroup, hence before that workgroup
//       publishes; they are written by workgroup 0 as its last act, after
//       every workgroup has published and so has read them.
// Barriers, four per launch: after the prologue's LDS fills; after dH (DHs,
// Hs, DLs and the per-wave partials complete); the publish barrier of (2); and the
// one the polling wave joins once its poll has matched. Between the second
// and the third each wave goes from its last MFMA straight to its slab
// stores (chunk_fwd_bwd<true> ends in no barrier; the summing wave stores
// db1 / db2 / loss from a register).
// ---------------------------------------------------------------------------

// The stripe threads. Wave 0 is the hand-off wave and nothing else (it stores
// the tag, polls and joins the barrier); the stripe of the Adam-state prefetch
// and of the reduce loop belongs to waves 1 to 7: thread tid >= STRIPE_T0
// takes i = lo + (tid - STRIPE_T0), then every STRIPE_STEP-th. Both loops go
// through stripe_first, so a thread reads back exactly the pre[] entries it
// wrote. The stripe gets no longer for it: ceil(span / 448) == ceil(span / 512)
// for the spans of 1 to 5 workgroups (2609, 1305, 870, 653, 522), and from 6
// workgroups on it is one iteration.
constexpr int STRIPE_T0 = 64;
constexpr int STRIPE_STEP = BLOCK - STRIPE_T0;
__device__ __forceinline__ int stripe_first(int lo, int tid) { return lo + (tid - STRIPE_T0); }

extern "C" __global__ void __launch_bounds__(BLOCK)
mlp_step_fused_kernel(// the seven arguments the prologue's vector loads need
                      // come first: 14 dwords, inside the 16 that the build's
                      // kernel-argument preload delivers in registers at
                      // wave start (setup.py)
                      const u16* __restrict__ Xbf, const int* __restrict__ y,
                      int B,
                      u16* __restrict__ wimg,          // optional packed images
                      float* __restrict__ master,
                      unsigned* __restrict__ counter,  // launch-epoch counter (both modes)
                      int* __restrict__ t_dev,
                      const u16* __restrict__ W1bf, const u16* __restrict__ W2bf,
                      u16* __restrict__ bfmirror,
                      float* __restrict__ m, float* __restrict__ v,
                      float* __restrict__ slabs,    // [n_wg][SLAB]
                      float* __restrict__ loss_out,
                      float invBtot, float lr, float beta1, float beta2,
                      float eps,
                      // non-null: write summed grads (+loss) and skip
                      // Adam — the DP path's pre-collective kernel
                      float* __restrict__ grads_out) {
  // ---- prologue, phase 0: the kernel arguments. Left alone the compiler
  // fetches an argument just before its first use: a second batch (wimg,
  // master, counter, t_dev) stood between the X loads and the image loads,
  // and stragglers (invBtot, the Adam scalars) waited in the middle of the
  // softmax. An empty asm statement uses its operands, so their scalar
  // loads and ONE wait for them sit above it. The seven arguments of the
  // vector loads below are pinned here: preloaded (setup.py) they are in
  // registers already and nothing waits; in a build without the preload, or
  // on firmware without it (the kernel's compatibility entry), they arrive
  // in one scalar round trip. The other arguments are pinned behind the
  // vector loads, so that their round trip runs beside those. ---------------
  asm volatile("" :: "s"(Xbf), "s"(y), "s"(B), "s"(wimg), "s"(master), "s"(counter),
               "s"(t_dev));

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L = carve(smem);
  // L.loss slots: [0] unused here (the loss travels in a register),
  // [1] poll verdict (0 ok, 1 timed out), [2] and [3] the Adam bias
  // corrections on their way from waves 1 and 2 to the stripe threads
  unsigned* lossu = (unsigned*)L.loss;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, lr_ = l & 15;
  const long long row0 = (long long)blockIdx.x * ROWS;

  // ---- prologue, phase 1: EVERY global load goes out before the first
  // wait (after the launch-boundary invalidate each one is a cold round
  // trip, so they must overlap): X vectors + label, packed images, bias
  // element, and the epoch / step counters -----------------------------------
  XChunkRegs xr;
  WimgRegs wr;
#ifndef PROBE_SKIP_LOADS
  issue_x_chunk(xr, Xbf, y, row0, B);
  if (wimg) issue_weight_images_packed(wr, wimg);
#else
  issue_label(xr, y, row0, B);   // timing probe: X and the images stay out
#endif
  const float bias = issue_biases(master + OFF_B1, master + OFF_B2);
  // Read the epoch source BEFORE any workgroup of this launch can have
  // advanced it (the writer only writes after every WG has published, i.e.
  // after every wave of every WG has consumed this load: it is waited for
  // below, ahead of the first barrier). BOTH modes use the dedicated launch
  // counter, so mixing fused-Adam and reduce-only launches on one model
  // keeps epochs unique and monotonic; t_dev is read separately for Adam
  // bias correction only. EVERY thread loads both words (one uniform
  // address, one vector load in flight with the others): the values live in
  // a register of every thread, nothing waits on a scalar load of its own
  // and nothing travels through LDS.
  const unsigned counter_pre = uniform_load(counter);
  const unsigned t_pre = (unsigned)uniform_load(t_dev);
  // every other argument, the implicit grid size included: one scalar round
  // trip in the shadow of the vector loads above; no fetch of an argument
  // is left behind the first barrier
  const int n_wg = gridDim.x;
  asm volatile("" :: "s"(W1bf), "s"(W2bf), "s"(bfmirror), "s"(m), "s"(v), "s"(slabs),
               "s"(loss_out), "s"(invBtot), "s"(lr), "s"(beta1), "s"(beta2), "s"(eps),
               "s"(grads_out), "s"(n_wg));

  // ---- phase 2: LDS fills that need no load, then the loaded registers ----
  zero_dl_pad(L);
#ifndef PROBE_SKIP_LOADS
  if (wimg) store_weight_images_packed(wr, L);
  else load_weight_images(L, W1bf, W2bf);
  store_x_chunk(xr, L);
#endif
  store_biases(bias, L);
  // This launch's epoch, unique per launch (exactly one WG advances the
  // counter per launch). The asm uses it, so every wave has its counter
  // word before it can reach the barrier.
  const unsigned epoch = counter_pre + 1u;
  asm volatile("" :: "v"(epoch), "v"(t_pre));
  __syncthreads();

  ChunkAcc acc;
  acc.dW1 = (f32x4){0.f, 0.f, 0.f, 0.f};
  acc.dW2 = (f32x4){0.f, 0.f, 0.f, 0.f};
  float bias_sum = 0.f;
#ifndef PROBE_SKIP_FWDBWD
  // single-chunk form: no barrier at its end. Each wave goes from its last
  // MFMA straight to its slab stores below; the next workgroup barrier is
  // the publish barrier, and the chunk arrays are reused only behind it
  // (the Adam-state prefetch into Xs). Xs is read until each wave's dW1,
  // its second-to-last or last GEMM: the publish barrier is behind every
  // wave's dW1, so the prefetch cannot overwrite rows a slower wave still
  // has to read.
  chunk_fwd_bwd<true>(L, L.b1s, L.b2s, chunk_label(xr), xr.valid, invBtot, acc, bias_sum);
#endif

  // ---- write this WG's complete partial slab: write-through (sc1) stores,
  // no atomics. Condition (1) of the header: EVERY slab word goes out through
  // xwg_store / xwg_store4. ---------------------------------------------------
  float* slab = slabs + (long long)blockIdx.x * SLAB;
  {
    // the wave's dW1^T tile holds, per lane, the four consecutive floats
    // h = ht*16 + lg*4 + r of row `in`: ONE 16-byte sc1 store per lane (a
    // bulk publish re-issued as narrow sc1 stores costs one fabric write
    // per store, G16 pitfall 7). 16-byte aligned: in * HID + ht*16 + lg*4
    // is a multiple of 4 floats, and so are OFF_W1 and SLAB.
    static_assert(OFF_W1 % 4 == 0 && HID % 4 == 0 && SLAB % 4 == 0, "16-B dW1 stores");
    const int ht = wave & 1, it = wave >> 1;
    const int in = it * 16 + lr_;
    xwg_store4(slab, SLAB, OFF_W1 + in * HID + ht * 16 + lg * 4, acc.dW1);
  }
  if (wave < 2) {
    // dW2's registers are CPAD floats apart: the epilogue's natural 4-byte
    // sc1 stores (each store instruction still fills whole 64-byte rows)
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = wave * 16 + lg * 4 + r;
      xwg_store(&slab[OFF_W2 + h * CPAD + lr_], acc.dW2[r]);
    }
  }
  // db1 / db2 / loss: the summing wave stores its register
  if (tid >= BIAS_SUM_T0 && tid < BIAS_SUM_T0 + PART) {
    xwg_store(&slab[bias_sum_index(tid - BIAS_SUM_T0)], bias_sum);
  }

  // ---- signal + all-WG barrier (guide §6 G16, write-through form: sc1
  // payload, every storing wave drains, ONE lane stores the per-slab epoch
  // tag sc1). The tag is this launch's epoch counter_pre+1 — unique per
  // launch, so the scheme is robust to any grid size, graph replay, and
  // engine mixing; no reset. ---------------------------------------------------
  // Adam-state prefetch scratch (loads issued during the sweep below);
  // the chunk arrays are dead behind the publish barrier (every wave's dW1
  // reads of Xs are done there) — reuse Xs
  float* pre = (float*)L.Xs;
  const int span_pre = (NPARAM + 1 + n_wg - 1) / n_wg;
  const int lo_pre = blockIdx.x * span_pre;
  const bool use_pre =
      (grads_out == nullptr) && (3 * span_pre * 4 <= ROWS * XS * 2);
  const float t_new = (float)(t_pre + 1u);
  float corr1 = 0.f, corr2 = 0.f;   // Adam bias corrections (fused mode only)
#ifndef PROBE_SKIP_HANDSHAKE
  // Condition (2): EVERY storing wave waits until its write-through stores
  // have completed (inline asm, so no compiler pass can drop the wait), and
  // only behind the barrier, i.e. behind every wave's wait, does lane 0
  // signal for the whole workgroup. No release fence: nothing of the slab is
  // left dirty in L2 for one to write back.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) xwg_store((unsigned*)(slab + NPARAM + 1), epoch);   // (3)
  // No barrier between the tag store and the polls: nothing reads what the
  // tag store orders. Lane 0 sits in the polling wave itself, the other
  // waves only work on their own Adam stripe until the barrier behind the
  // poll, and another workgroup sees the tag whenever it arrives.

  // Two roles until that barrier. Wave 0 is the hand-off wave and nothing
  // else: from the tag store it goes straight to its first poll, with no
  // load of its own to wait for. Waves 1 to 7 do two things WHILE the sweep
  // waits. They prefetch this WG's Adam-state stripe (master/m/v) into LDS —
  // these are only ever written by this same WG's stripe in the reduce
  // phase, so plain loads ahead of the poll are safe (condition (4)), and it
  // pulls an HBM round trip out of the reduce chain. And two of them compute
  // the Adam bias corrections, two full pow expansions whose only inputs
  // (beta1, beta2, t_pre) every thread has held since the prologue: wave 1
  // corr1, wave 2 corr2, one chain each, so that the pair takes the time of
  // one (both chains in every stripe wave outlast the poll and hold the
  // barrier up). The stripe's first loads go out, the arithmetic runs while
  // they are in flight, and the empty asm pins it here (left alone the
  // compiler sinks the pure arithmetic to its use, behind the last barrier
  // and in front of the first slab load). The values cross the barrier in
  // L.loss[2] and [3]. Reduce-only launches need no correction and compute
  // none.
  if (wave != 0) {
    const int hi_pre = min(lo_pre + span_pre, NPARAM);
    int i = stripe_first(lo_pre, tid);
    const bool first = use_pre && i < hi_pre;
    float p0 = 0.f, m0 = 0.f, v0 = 0.f;
    if (first) {
      p0 = master[i];
      m0 = m[i];
      v0 = v[i];
    }
    if (!grads_out && wave <= 2) {
#ifdef PROBE_CONST_CORR
      const float c = wave == 1 ? 10.f : 1000.f;   // timing probe: no pow
#else
      const float c = adam_bias_corr_one(wave == 1 ? beta1 : beta2, t_new);
#endif
      asm volatile("" :: "v"(c));
      if (l == 0) L.loss[1 + wave] = c;
    }
    if (first) {
      const int j = i - lo_pre;
      pre[j] = p0;
      pre[span_pre + j] = m0;
      pre[2 * span_pre + j] = v0;
    }
    if (use_pre) {
      for (i += STRIPE_STEP; i < hi_pre; i += STRIPE_STEP) {
        const int j = i - lo_pre;
        pre[j] = master[i];
        pre[span_pre + j] = m[i];
        pre[2 * span_pre + j] = v[i];
      }
    }
  } else {
    // relaxed PARALLEL sweep: lane j polls tags j, j+64, ... (G16: never
    // poll with an acquire). One vector gather per poll round — one
    // memory round trip after the last publish, independent of n_wg
    // (the serial lane-0 sweep this replaces cost ~500 cyc per WG and
    // dominated the handshake at large grids).
    unsigned spins = 0;
    bool ok = true;
    for (int w = l; w < n_wg; w += 64) {
      for (;;) {
        const unsigned tag = xwg_load(
            (const unsigned*)(slabs + (long long)w * SLAB + NPARAM + 1));
        if (tag == epoch) break;
        __builtin_amdgcn_s_sleep(2);
        if (++spins > 100000000u) { ok = false; break; }
      }
      if (!ok) break;
    }
#ifdef PROBE_COUNT_POLLS
    {
      // counting probe: the wave's poll rounds (its slowest lane's), binned
      // 1 .. 13 and 14+ in the spare words behind slab 0's tag
      unsigned rounds = spins + 1u;
      #pragma unroll
      for (int o = 32; o > 0; o >>= 1) rounds = max(rounds, (unsigned)__shfl_xor((int)rounds, o));
      if (l == 0 && blockIdx.x == 0) {
        atomicAdd((unsigned*)(slabs + NPARAM + 2) + (min(rounds, 14u) - 1u), 1u);
      }
    }
#endif
    const unsigned long long bad = __ballot(!ok);
    // No agent acquire: every slab load below is an sc1 load, which does
    // not look into this CU's L1, so there is no stale line to invalidate
    // (condition (4)). The wavefront-scope fence emits no instruction; it
    // keeps the compiler from moving those loads above the poll.
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (l == 0) lossu[1] = bad ? 1u : 0u;
  }
  // the polling wave joins this barrier only after its poll has matched:
  // the other waves' slab loads all sit behind it
  __syncthreads();
  if (lossu[1] != 0u) {             // timed out: poison the loss, keep going
    if (tid == 0 && blockIdx.x == 0) *loss_out = __builtin_nanf("");
    return;
  }
#endif  // PROBE_SKIP_HANDSHAKE

#ifdef PROBE_SKIP_REDUCE
  if (tid == 0 && blockIdx.x == 0) {
    *counter = epoch;
    if (!grads_out) *t_dev = (int)(t_pre + 1u);
  }
  return;
#endif
  // ---- every WG reduces its own param stripe + applies Adam ----------------
#ifdef PROBE_SKIP_HANDSHAKE
  // timing probe without the hand-off window: the corrections at their use
  if (!grads_out) adam_bias_corr(beta1, beta2, t_new, corr1, corr2);
#else
  if (!grads_out) corr1 = L.loss[2], corr2 = L.loss[3];
#endif
  const int span = (NPARAM + 1 + n_wg - 1) / n_wg;
  const int lo = blockIdx.x * span;
  const int hi = min(lo + span, NPARAM + 1);
  for (int i = stripe_first(lo, tid); wave != 0 && i < hi; i += STRIPE_STEP) {
    // Eight chains: chain k sums the slabs w = k, k+8, k+16, ... in that
    // order; the remainder (n_wg % 8 slabs) goes into chain 0; then the
    // chains are folded pairwise. That order is pinned bit for bit. What is
    // free is how many loads are in flight: each batch below issues ALL its
    // loads before its first add (a batch is one memory round trip, and a
    // written-through slab word is in no L2), 16 slabs at a time, then 8,
    // then the remainder's up to 7 in one batch as well. The remainder
    // loads unconditionally, past the grid's end the last slab once more,
    // and only the ADD is predicated (adding a zero instead could turn a
    // -0 sum into +0). Every slab word through xwg_load (sc1, past the
    // L1): condition (4).
    float gc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int w = 0;
    for (; w + 16 <= n_wg; w += 16) {
      float a[16];
      #pragma unroll
      for (int k = 0; k < 16; ++k) a[k] = xwg_load(&slabs[(long long)(w + k) * SLAB + i]);
      #pragma unroll
      for (int k = 0; k < 16; ++k) gc[k & 7] += a[k];
    }
    for (; w + 8 <= n_wg; w += 8) {
      float a[8];
      #pragma unroll
      for (int k = 0; k < 8; ++k) a[k] = xwg_load(&slabs[(long long)(w + k) * SLAB + i]);
      #pragma unroll
      for (int k = 0; k < 8; ++k) gc[k] += a[k];
    }
    if (w < n_wg) {
      float a[7];
      #pragma unroll
      for (int k = 0; k < 7; ++k) {
        a[k] = xwg_load(&slabs[(long long)min(w + k, n_wg - 1) * SLAB + i]);
      }
      #pragma unroll
      for (int k = 0; k < 7; ++k) {
        if (w + k < n_wg) gc[0] += a[k];
      }
    }
    const float g0 = gc[0], g1 = gc[1], g2 = gc[2], g3 = gc[3];
    const float g4 = gc[4], g5 = gc[5], g6 = gc[6], g7 = gc[7];
    const float g = ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7));
    if (grads_out) {            // reduce-only: hand the summed grads (+loss
      grads_out[i] = g;         // at NPARAM) to the RCCL all-reduce
      continue;
    }
    if (i == NPARAM) {
      *loss_out = g;
      continue;
    }
    const int j = i - lo;
    float p = use_pre ? pre[j] : master[i];
    float mi = use_pre ? pre[span_pre + j] : m[i];
    float vi = use_pre ? pre[2 * span_pre + j] : v[i];
    adam_update(p, mi, vi, g, lr, beta1, beta2, eps, corr1, corr2);
    m[i] = mi;
    v[i] = vi;
    master[i] = p;
    const u16 wb = f2bf(p);
    bfmirror[i] = wb;
    if (wimg) wimg_write(wimg, i, wb);
  }
  if (tid == 0 && blockIdx.x == 0) {
    *counter = epoch;
    if (!grads_out) *t_dev = (int)t_new;
  }
}

// ---------------------------------------------------------------------------
// fused Adam (per-step DP path) — single block, device step counter
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(256)
adam_step_kernel(float* __restrict__ master, u16* __restrict__ bfmirror,
                 const float* __restrict__ grads, float* __restrict__ m,
                 float* __restrict__ v, int* __restrict__ t_dev,
                 float lr, float beta1, float beta2, float eps,
                 u16* __restrict__ wimg) {
  __shared__ float corr1, corr2;
  // 4 strided elements per thread and iteration, all their loads issued
  // before the first use, so the g/m/v/master reads overlap instead of
  // serializing one HBM round trip per element (the serial version measured
  // 6.7 us for 2.6k params: pure latency)
  constexpr int U = 4, STEP = 256 * U;
  float g[U], mi_[U], vi_[U], p_[U];
  auto load_batch = [&](int base) {
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * 256;
      if (i < NPARAM) {
        g[u] = grads[i];
        mi_[u] = m[i];
        vi_[u] = v[i];
        p_[u] = master[i];
      }
    }
  };
  // Thread 0's chain (the step counter's round trip, two pow expansions, the
  // LDS write) stands in front of the barrier. Every thread's first batch of
  // loads goes out before it, thread 0's behind its counter load, so the
  // chain runs beside them instead of in front of them.
  int t = 0;
  if (threadIdx.x == 0) t = *t_dev + 1;
  int base = (int)threadIdx.x;
  load_batch(base);
  if (threadIdx.x == 0) {
    *t_dev = t;
    adam_bias_corr(beta1, beta2, (float)t, corr1, corr2);
  }
  __syncthreads();
  for (;;) {
    #pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = base + u * 256;
      if (i < NPARAM) {
        float p = p_[u], mi = mi_[u], vi = vi_[u];
        adam_update(p, mi, vi, g[u], lr, beta1, beta2, eps, corr1, corr2);
        m[i] = mi;
        v[i] = vi;
        master[i] = p;
        const u16 wb = f2bf(p);
        bfmirror[i] = wb;
        if (wimg) wimg_write(wimg, i, wb);
      }
    }
    base += STEP;
    if (base >= NPARAM) break;
    load_batch(base);
  }
}

// ---------------------------------------------------------------------------
// persistent multi-step kernel: ONE workgroup, optimizer state in LDS
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(BLOCK, 1)
mlp_train_steps_kernel(const u16* __restrict__ Xbf,  // [N][IN] staged bf16
                       const int* __restrict__ y,    // [N]
                       long long N, int B, int n_steps,
                       float* __restrict__ master,   // HBM fp32 in/out
                       u16* __restrict__ bfmirror,   // HBM bf16 out
                       float* __restrict__ m,        // HBM in/out
                       float* __restrict__ v,        // HBM in/out
                       int* __restrict__ t_dev,
                       float* __restrict__ loss_out, // last-step loss
                       float lr, float beta1, float beta2, float eps) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L = carve(smem);
  float* master_s = (float*)(smem + C_MASTER);
  float* m_s = (float*)(smem + C_M);
  float* v_s = (float*)(smem + C_V);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, ln = l & 15;

  // ---- optimizer state + weight images into LDS -----------------------------
  for (int i = tid; i < NPARAM; i += BLOCK) {
    master_s[i] = master[i];
    m_s[i] = m[i];
    v_s[i] = v[i];
  }
  __syncthreads();
  // weight images from the fp32 master (single source of truth)
  for (int i = tid; i < HID * IN; i += BLOCK) {
    const int h = i / IN, k = i % IN;
    L.W1T[h][k] = f2bf(master_s[OFF_W1 + k * HID + h]);
  }
  for (int i = tid; i < HID * 32; i += BLOCK) {
    const int h = i / 32, c = i % 32;
    L.W2s[h][c] = (c < CPAD) ? f2bf(master_s[OFF_W2 + h * CPAD + c]) : (u16)0;
  }
  for (int i = tid; i < CPAD * HID; i += BLOCK) {
    const int c = i / HID, h = i % HID;
    L.W2T[c][h] = f2bf(master_s[OFF_W2 + h * CPAD + c]);
  }
  zero_dl_pad(L);
  const int t0 = *t_dev;
  float b1t = __powf(beta1, (float)t0), b2t = __powf(beta2, (float)t0);
  __syncthreads();

  const int batches = (int)(N / B);
  const int chunks = B / ROWS;
  const float invB = fast_rcp((float)B);

  for (int s = 0; s < n_steps; ++s) {
    const long long base = (long long)(s % batches) * B;

    if (tid < HID) L.db1[tid] = 0.f;
    if (tid < CPAD) L.db2[tid] = 0.f;
    if (tid == 0) L.loss[0] = 0.f;

    ChunkAcc acc;
    acc.dW1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    acc.dW2 = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < chunks; ++ch) {
      const long long row0 = base + (long long)ch * ROWS;
      XChunkRegs xr;   // the chunk's X vectors and label in one round trip
      issue_x_chunk(xr, Xbf, y, row0, N);
      store_x_chunk(xr, L);
      __syncthreads();
      float unused;
      chunk_fwd_bwd<false>(L, master_s + OFF_B1, master_s + OFF_B2, chunk_label(xr),
                           xr.valid, invB, acc, unused);
    }

    // ---- fused in-LDS Adam --------------------------------------------------
    b1t *= beta1;
    b2t *= beta2;
    const float corr1 = adam_corr(b1t);
    const float corr2 = adam_corr(b2t);

    auto adam_at = [&](int i, float g) {
      adam_update(master_s[i], m_s[i], v_s[i], g, lr, beta1, beta2, eps, corr1, corr2);
    };

    {
      const int ht = wave & 1, it = wave >> 1;
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = ht * 16 + lg * 4 + r;
        const int in = it * 16 + ln;
        const int idx = OFF_W1 + in * HID + h;
        adam_at(idx, acc.dW1[r]);
        L.W1T[h][in] = f2bf(master_s[idx]);
      }
    }
    if (wave < 2) {
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int h = wave * 16 + lg * 4 + r;
        const int idx = OFF_W2 + h * CPAD + ln;
        adam_at(idx, acc.dW2[r]);
        const u16 wb = f2bf(master_s[idx]);
        L.W2s[h][ln] = wb;
        L.W2T[ln][h] = wb;
      }
    }
    if (wave == 2) {
      if (l < HID) {
        adam_at(OFF_B1 + l, L.db1[l]);
      } else if (l < HID + CPAD) {
        adam_at(OFF_B2 + (l - HID), L.db2[l - HID]);
      }
    }
    __syncthreads();   // weights updated before next step's fwd
  }

  // ---- write state back to HBM ----------------------------------------------
  if (tid == 0) {
    *t_dev = t0 + n_steps;
    *loss_out = L.loss[0];
  }
  for (int i = tid; i < NPARAM; i += BLOCK) {
    master[i] = master_s[i];
    m[i] = m_s[i];
    v[i] = v_s[i];
    bfmirror[i] = f2bf(master_s[i]);
  }
}

// ---------------------------------------------------------------------------
// fused predict: standardize + fwd + argmax (serving hot path).
// Uses the same transposed-output fragment scheme (logits arrive as L^T,
// so the class axis lives in registers/lane-groups and the row-argmax is a
// 2-level shuffle).
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(BLOCK)
mlp_predict_kernel(const float* __restrict__ X, int B,
                   const float* __restrict__ mean,
                   const float* __restrict__ invstd,
                   const u16* __restrict__ W1bf, const u16* __restrict__ W2bf,
                   const float* __restrict__ master,
                   int* __restrict__ preds,
                   float* __restrict__ probs /* optional [B][CLS] */) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const Lds L = carve(smem);

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int l = tid & 63;
  const int lg = l >> 4, lr = l & 15;
  const long long row0 = (long long)blockIdx.x * ROWS;
  const int wrow = wave * 16;

  // standardize on load (fp32 -> bf16); only Xs needed (no bwd)
  for (int i = tid; i < ROWS * IN; i += BLOCK) {
    const int r = i / IN, c = i % IN;
    const float v =
        (row0 + r < B) ? (X[(row0 + r) * IN + c] - mean[c]) * invstd[c] : 0.f;
    L.Xs[r][c] = f2bf(v);
  }
  load_weight_images(L, W1bf, W2bf);
  __syncthreads();

  const float* b1 = master + OFF_B1;
  const float* b2 = master + OFF_B2;

  // fwd1: H^T = W1T @ B(Xs) -> write Hs only
  #pragma unroll
  for (int mt = 0; mt < HID / 16; ++mt) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    #pragma unroll
    for (int ks = 0; ks < IN / 32; ++ks) {
      const bf16x8 a = *(const bf16x8*)&L.W1T[mt * 16 + lr][ks * 32 + lg * 8];
      const bf16x8 b = *(const bf16x8*)&L.Xs[wrow + lr][ks * 32 + lg * 8];
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int h = mt * 16 + lg * 4 + r;
      float hv = acc[r] + b1[h];
      L.Hs[wrow + lr][h] = f2bf(hv > 0.f ? hv : 0.f);
    }
  }
  __syncthreads();

  // fwd2: L^T = W2T @ B(Hs); argmax/softmax over the class axis
  {
    f32x4 acc[1] = {{0.f, 0.f, 0.f, 0.f}};
    const bf16x8 a = *(const bf16x8*)&L.W2T[lr][lg * 8];
    const bf16x8 b = *(const bf16x8*)&L.Hs[wrow + lr][lg * 8];
    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[0], 0, 0, 0);

    const int row = wrow + lr;
    float best;
    int bcol;
    float logit[1][4];
    head_logits<1>(logit, acc, b2, CLS, lg);
    head_argmax<1>(logit, CLS, lg, best, bcol);
    if (lg == 0 && row0 + row < B) preds[row0 + row] = bcol;
    if (probs != nullptr) {
      float e[1][4];
      const float rs = fast_rcp(head_exp_sum<1>(e, logit, best, CLS, lg));
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int c = lg * 4 + r;
        if (c < CLS && row0 + row < B) {
          probs[(row0 + row) * CLS + c] = e[0][r] * rs;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// row_sum16 self-test: one wave per row of x [n][64]. Lane l writes the
// DPP helper's result to out[row][l][0] and the plain __shfl_xor
// butterfly's (the form row_sum16 replaced, kept only here) to
// out[row][l][1]; the two must agree bit for bit.
// ---------------------------------------------------------------------------

extern "C" __global__ void __launch_bounds__(64)
reduce_selftest_kernel(const float* __restrict__ x, int n,
                       float* __restrict__ out) {
  const int row = blockIdx.x;
  const int l = threadIdx.x;
  if (row >= n) return;                      // whole wave, never a partial one
  const float v = x[(long long)row * 64 + l];
  const float dpp = row_sum16(v);
  float bfly = v;
  bfly += __shfl_xor(bfly, 1, 64);
  bfly += __shfl_xor(bfly, 2, 64);
  bfly += __shfl_xor(bfly, 4, 64);
  bfly += __shfl_xor(bfly, 8, 64);
  out[((long long)row * 64 + l) * 2 + 0] = dpp;
  out[((long long)row * 64 + l) * 2 + 1] = bfly;
}

// ---------------------------------------------------------------------------
// host launchers (extern "C"; stream-ordered, capture-safe)
// ---------------------------------------------------------------------------

extern "C" {

void launch_standardize_fit(const float* X, long long N, int D, float* mean,
                            float* invstd, float eps, double* scratch,
                            hipStream_t stream) {
  if (scratch != nullptr && D <= 256 && 256 % D == 0) {
    const int rpi = 256 / D;
    // one WG per ~64 KB of input: small inputs stay atomic-light (each
    // extra WG costs 2 serialized fp64 atomics PER COLUMN — 750 WGs on a
    // [3000,64] fit measured 753 µs vs 10 µs at 12 WGs), large inputs
    // still fan out to 1024 WGs (>8 XCDs) for bandwidth
    long long blocks_ll = (N * (long long)D * 4) / 65536;
    int blocks = (int)(blocks_ll < 1 ? 1 : (blocks_ll > 1024 ? 1024 : blocks_ll));
    {
      const int max_useful = (int)((N + rpi - 1) / rpi);
      if (blocks > max_useful) blocks = max_useful;
    }
    hipLaunchKernelGGL(standardize_fit_fast_kernel, dim3(blocks), dim3(256), 0,
                       stream, X, N, D, scratch);
    hipLaunchKernelGGL(standardize_fit_finalize_kernel,
                       dim3((D + 255) / 256), dim3(256), 0, stream, scratch, N,
                       D, mean, invstd, eps);
    return;
  }
  hipLaunchKernelGGL(standardize_fit_kernel, dim3(D), dim3(256), 0, stream,
                     X, N, D, mean, invstd, eps);
}

void launch_standardize_apply(const float* X, long long N, int D, int Dout,
                              const float* mean, const float* invstd,
                              unsigned short* out, hipStream_t stream) {
  const long long n = N * D;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(standardize_apply_kernel, dim3(blocks), dim3(256), 0, stream,
                     X, n, D, Dout, mean, invstd, out);
}

int launch_mlp_step(const unsigned short* Xbf, const int* y, int B,
                    const unsigned short* W1bf, const unsigned short* W2bf,
                    const float* master, float* grads, float invBtot,
                    hipStream_t stream) {
  if (B < 1) return -3;
  if (ensure_dynamic_lds<mlp_step_kernel>(C_IMG_TOTAL) != 0) return -2;
  const int blocks = (B + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(mlp_step_kernel, dim3(blocks), dim3(BLOCK), C_IMG_TOTAL,
                     stream, Xbf, y, B, W1bf, W2bf, master, grads, invBtot);
  return 0;
}

int launch_mlp_step_fused(const unsigned short* Xbf, const int* y, int B,
                          const unsigned short* W1bf, const unsigned short* W2bf,
                          float* master, unsigned short* bfmirror, float* m,
                          float* v, int* t_dev, float* slabs, unsigned* counter,
                          float* loss_out, float invBtot, float lr, float beta1,
                          float beta2, float eps, int max_slabs, float* grads_out,
                          unsigned short* wimg, hipStream_t stream) {
  if (B < 1) return -3;
  const int blocks = (B + ROWS - 1) / ROWS;
  if (blocks > max_slabs) return -1;
  if (ensure_dynamic_lds<mlp_step_fused_kernel>(C_IMG_TOTAL) != 0) return -2;
  hipLaunchKernelGGL(mlp_step_fused_kernel, dim3(blocks), dim3(BLOCK), C_IMG_TOTAL,
                     stream, Xbf, y, B, wimg, master, counter, t_dev, W1bf, W2bf,
                     bfmirror, m, v, slabs, loss_out, invBtot, lr, beta1, beta2, eps,
                     grads_out);
  return 0;
}

int launch_mlp_train_steps(const unsigned short* Xbf, const int* y, long long N,
                           int B, int n_steps, float* master,
                           unsigned short* bfmirror, float* m, float* v,
                           int* t_dev, float* loss_out, float lr, float beta1,
                           float beta2, float eps, hipStream_t stream) {
  if (B < 1 || N < 1 || n_steps < 0) return -3;   // before N % B divides
  if (B % ROWS != 0 || N % B != 0) return -1;     // caller falls back
  if (ensure_dynamic_lds<mlp_train_steps_kernel>(C_STEPS_TOTAL) != 0) return -2;
  hipLaunchKernelGGL(mlp_train_steps_kernel, dim3(1), dim3(BLOCK), C_STEPS_TOTAL,
                     stream, Xbf, y, N, B, n_steps, master, bfmirror, m, v,
                     t_dev, loss_out, lr, beta1, beta2, eps);
  return 0;
}

int launch_mlp_predict(const float* X, int B, const float* mean,
                       const float* invstd, const unsigned short* W1bf,
                       const unsigned short* W2bf, const float* master,
                       int* preds, float* probs, hipStream_t stream) {
  if (B < 1) return -3;
  if (ensure_dynamic_lds<mlp_predict_kernel>(C_IMG_TOTAL) != 0) return -2;
  const int blocks = (B + ROWS - 1) / ROWS;
  hipLaunchKernelGGL(mlp_predict_kernel, dim3(blocks), dim3(BLOCK), C_IMG_TOTAL,
                     stream, X, B, mean, invstd, W1bf, W2bf, master, preds, probs);
  return 0;
}

void launch_adam_step(float* master, unsigned short* bfmirror, const float* grads,
                      float* m, float* v, int* t_dev, float lr, float beta1,
                      float beta2, float eps, unsigned short* wimg,
                      hipStream_t stream) {
  hipLaunchKernelGGL(adam_step_kernel, dim3(1), dim3(256), 0, stream,
                     master, bfmirror, grads, m, v, t_dev, lr, beta1, beta2, eps,
                     wimg);
}

void launch_reduce_selftest(const float* x, int n, float* out,
                            hipStream_t stream) {
  if (n <= 0) return;
  hipLaunchKernelGGL(reduce_selftest_kernel, dim3(n), dim3(64), 0, stream, x, n,
                     out);
}

}  // extern "C"
