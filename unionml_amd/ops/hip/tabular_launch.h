// Host-visible interface of the tabular kernels: the digits-geometry
// layout constants, the generalized kernels' instantiation table and padded
// geometry, and every extern "C" launcher, declared ONCE. Both kernel files
// and the torch bindings include this header, so a launcher whose
// definition drifts from its declaration is a compile error instead of a
// silently mis-ordered argument list.
//
// The constants carry a DIGITS_ prefix: short names such as IN or HID
// clash with macros of other headers and with the generalized kernels'
// template parameters.
#pragma once

#include <climits>

#include <hip/hip_runtime_api.h>

// digits MLP: IN=64 -> HID=32 relu -> CLS=10 softmax (CLS padded to one
// MFMA tile)
constexpr int DIGITS_IN = 64;
constexpr int DIGITS_HID = 32;
constexpr int DIGITS_CLS = 10;
constexpr int DIGITS_CPAD = 16;

// flat master/grads layout (floats):
//   [0, 2048)     W1 [IN][HID]
//   [2048, 2080)  b1 [HID]
//   [2080, 2592)  W2 [HID][CPAD]  (cols >= CLS stay zero)
//   [2592, 2608)  b2 [CPAD]
//   [2608]        loss (grads buffer only)
constexpr int DIGITS_OFF_W1 = 0;
constexpr int DIGITS_OFF_B1 = DIGITS_IN * DIGITS_HID;
constexpr int DIGITS_OFF_W2 = DIGITS_OFF_B1 + DIGITS_HID;
constexpr int DIGITS_OFF_B2 = DIGITS_OFF_W2 + DIGITS_HID * DIGITS_CPAD;
constexpr int DIGITS_NPARAM = DIGITS_OFF_B2 + DIGITS_CPAD;
// per-workgroup gradient slab: NPARAM + loss + epoch tag, padded to a
// 16-float multiple
constexpr int DIGITS_SLAB = (DIGITS_NPARAM + 2 + 15) / 16 * 16;

// packed weight image: the three LDS images W1T [HID][XS], W2s [HID][WS],
// W2T [CPAD][WS] back to back, strides in bf16 elements
constexpr int DIGITS_XS = 72;
constexpr int DIGITS_WS = 40;
constexpr int DIGITS_WIMG_W1T = 0;
constexpr int DIGITS_WIMG_W2S = DIGITS_HID * DIGITS_XS;
constexpr int DIGITS_WIMG_W2T = DIGITS_WIMG_W2S + DIGITS_HID * DIGITS_WS;
constexpr int DIGITS_WIMG_N = DIGITS_WIMG_W2T + DIGITS_CPAD * DIGITS_WS;

static_assert(DIGITS_NPARAM == 2608 && DIGITS_SLAB == 2624 &&
                  DIGITS_WIMG_N == 4224,
              "digits layout changed: staged buffers and checkpoints depend on it");

// ---- generalized kernels (tabular_gen.hip): table and geometry ---------------

// Every compiled <HID, RT, CPAD> instantiation of the generalized step
// kernel, one row each, for both heads. PREDICT marks the row whose RT the
// predict kernel is compiled at too: the larger RT of its (HID, CPAD). The
// step dispatch matches (hid, rt, cpad) exactly, the predict dispatch
// (hid, cpad). ops/reference.py GEN_INSTANTIATIONS is the Python copy; a
// test holds the two equal.
//   X(HID, RT, CPAD, PREDICT)
#define TABULAR_GEN_INSTANTIATIONS(X) \
  X(32, 128, 16, 1)                   \
  X(32, 64, 16, 0)                    \
  X(64, 128, 16, 1)                   \
  X(64, 64, 16, 0)                    \
  X(128, 64, 16, 1)                   \
  X(128, 32, 16, 0)                   \
  X(256, 32, 16, 1)                   \
  X(32, 128, 32, 1)                   \
  X(64, 128, 32, 1)                   \
  X(128, 64, 32, 1)                   \
  X(256, 32, 32, 1)

// Padded geometry of the generalized kernels as the host sees it (the
// Python copy is reference.Geometry): the flat master/grads layout
//   W1 [inp][hid] | b1 [hid] | W2 [hid][cpad] | b2 [cpad] | loss (grads only)
// and the packed weight image W1T [hid][inp] | W2s [hid][32] | W2T [cpad][hid].
// Sizes are 64-bit here; the kernels index with int, so ok() refuses a
// geometry whose slab row or image does not fit one.
struct GenGeometry {
  long long inp, hid, cpad;   // staged input width, compiled hidden, padded outputs

  // classes or targets (1..32) padded to one or two MFMA tiles
  static constexpr int cpad_for(long long n_out) { return n_out <= 16 ? 16 : 32; }

  constexpr long long off_w1() const { return 0; }
  constexpr long long off_b1() const { return inp * hid; }
  constexpr long long off_w2() const { return off_b1() + hid; }
  constexpr long long off_b2() const { return off_w2() + hid * cpad; }
  constexpr long long nparam() const { return off_b2() + cpad; }
  // a workgroup's slab row: nparam + loss + epoch tag
  constexpr long long min_slab_stride() const { return nparam() + 2; }
  constexpr long long wimg_w2s() const { return hid * inp; }
  constexpr long long wimg_w2t() const { return wimg_w2s() + hid * 32; }
  constexpr long long wimg_n() const { return wimg_w2t() + cpad * hid; }

  constexpr bool ok() const {
    return inp >= 32 && inp % 32 == 0 && inp <= INT_MAX && hid >= 1 &&
           hid <= INT_MAX && (cpad == 16 || cpad == 32) &&
           min_slab_stride() <= INT_MAX && wimg_n() <= INT_MAX;
  }
};

constexpr GenGeometry DIGITS_AS_GEN{DIGITS_IN, DIGITS_HID, DIGITS_CPAD};
static_assert(DIGITS_AS_GEN.ok() && DIGITS_AS_GEN.off_b1() == DIGITS_OFF_B1 &&
                  DIGITS_AS_GEN.off_w2() == DIGITS_OFF_W2 &&
                  DIGITS_AS_GEN.off_b2() == DIGITS_OFF_B2 &&
                  DIGITS_AS_GEN.nparam() == DIGITS_NPARAM,
              "the digits flat layout is the generalized one at 64x32x16");
// four of the geometries tests/oracle64.py runs, as reference.Geometry
// computes them (tests/test_tabular_gen_cpu.py holds Geometry to the same
// literals and to the rest of the set):
//   {inp, hid, cpad} -> off_b1, off_w2, off_b2, nparam, image W2T offset, size
constexpr bool gen_geometry_is(GenGeometry g, long long off_b1, long long off_w2,
                               long long off_b2, long long nparam,
                               long long wimg_w2t, long long wimg_n) {
  return g.ok() && g.off_b1() == off_b1 && g.off_w2() == off_w2 &&
         g.off_b2() == off_b2 && g.nparam() == nparam &&
         g.min_slab_stride() == nparam + 2 && g.wimg_w2s() == off_b1 &&
         g.wimg_w2t() == wimg_w2t && g.wimg_n() == wimg_n;
}
static_assert(
    gen_geometry_is({32, 32, 16}, 1024, 1056, 1568, 1584, 2048, 2560) &&
        gen_geometry_is({32, 32, 32}, 1024, 1056, 2080, 2112, 2048, 3072) &&
        gen_geometry_is({224, 128, 32}, 28672, 28800, 32896, 32928, 32768, 36864) &&
        gen_geometry_is({96, 256, 16}, 24576, 24832, 28928, 28944, 32768, 36864),
    "GenGeometry and reference.Geometry disagree");
static_assert(!GenGeometry{1LL << 23, 256, 16}.ok() && !GenGeometry{48, 32, 16}.ok() &&
                  !GenGeometry{32, 32, 24}.ok() && GenGeometry{1LL << 20, 256, 32}.ok(),
              "ok() refuses what an int cannot index and unpadded widths");

// ---- evaluation (tabular_eval.hip): record layout ---------------------------

// A workgroup's partial row and a metrics record share one layout (fp32
// entries). Classifier: [LOSS] mean of -log softmax(z)[y], [CORRECT] the
// rows with argmax == y, an int32 stored as its bits. Regression: [LOSS]
// mean of 0.5 * sum_c (z - y)^2, [FIRST_MSE + c] the mean of (z - y)^2 of
// column c < cpad in standardized units (pad columns exactly 0). The
// partial rows hold the same entries as unnormalised fp32 sums.
constexpr int EVAL_REC_LOSS = 0;
constexpr int EVAL_REC_CORRECT = 1;
constexpr int EVAL_REC_CLS_N = 2;
constexpr int EVAL_REC_FIRST_MSE = 1;
constexpr int eval_rec_reg_n(int cpad) { return EVAL_REC_FIRST_MSE + cpad; }

// Raise a kernel's dynamic-LDS limit to `bytes`: 0, or -2 when the runtime
// refuses. Done once per process and kernel (the flag is per instantiation),
// as the launchers always did; per-device setup is not attempted.
template <auto Kernel>
int ensure_dynamic_lds(int bytes) {
  static bool done = false;
  if (!done) {
    done = hipFuncSetAttribute((const void*)Kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               bytes) == hipSuccess;
  }
  return done ? 0 : -2;
}

extern "C" {

// ---- tabular_kernels.hip ---------------------------------------------------

void launch_standardize_fit(const float* X, long long N, int D, float* mean,
                            float* invstd, float eps, double* scratch,
                            hipStream_t stream);
void launch_standardize_apply(const float* X, long long N, int D, int Dout,
                              const float* mean, const float* invstd,
                              unsigned short* out, hipStream_t stream);
// Return codes of the int launchers: 0 launched; -2 the dynamic-LDS
// attribute failed; -3 arguments outside what the kernels take (a batch
// below one row, or, for the generalized family, no instantiation for the
// geometry); -1 is per launcher, below.
int launch_mlp_step(const unsigned short* Xbf, const int* y, int B,
                    const unsigned short* W1bf, const unsigned short* W2bf,
                    const float* master, float* grads, float invBtot,
                    hipStream_t stream);
// -1: more workgroups than slab rows
int launch_mlp_step_fused(const unsigned short* Xbf, const int* y, int B,
                          const unsigned short* W1bf, const unsigned short* W2bf,
                          float* master, unsigned short* bfmirror, float* m,
                          float* v, int* t_dev, float* slabs, unsigned* counter,
                          float* loss_out, float invBtot, float lr, float beta1,
                          float beta2, float eps, int max_slabs, float* grads_out,
                          unsigned short* wimg, hipStream_t stream);
// -1: shape constraints unmet (caller falls back)
int launch_mlp_train_steps(const unsigned short* Xbf, const int* y, long long N,
                           int B, int n_steps, float* master,
                           unsigned short* bfmirror, float* m, float* v,
                           int* t_dev, float* loss_out, float lr, float beta1,
                           float beta2, float eps, hipStream_t stream);
int launch_mlp_predict(const float* X, int B, const float* mean,
                       const float* invstd, const unsigned short* W1bf,
                       const unsigned short* W2bf, const float* master,
                       int* preds, float* probs, hipStream_t stream);
void launch_adam_step(float* master, unsigned short* bfmirror, const float* grads,
                      float* m, float* v, int* t_dev, float lr, float beta1,
                      float beta2, float eps, unsigned short* wimg,
                      hipStream_t stream);
// x [n][64] fp32, one wave per row -> out [n][64][2]: the in-row sum of 16
// by the kernels' DPP helper, and by the plain shuffle butterfly
void launch_reduce_selftest(const float* x, int n, float* out,
                            hipStream_t stream);

// ---- tabular_gen.hip (any geometry) -----------------------------------------

// -1: more workgroups than slab rows
int launch_mlp_step_gen(const unsigned short* Xbf, const int* y, int B, int inp,
                        int hid, int cls, int rt, const unsigned short* wimg,
                        const float* master, float* slabs, int slab_stride,
                        int max_slabs, float invBtot, hipStream_t stream);
int launch_reduce_adam_gen(const float* slabs, int n_wg, int slab_stride,
                           int inp, int hid, int cpad, float* master,
                           unsigned short* bfmirror, float* m, float* v,
                           int* t_dev, float* loss_out, float lr, float beta1,
                           float beta2, float eps, unsigned short* wimg,
                           float* grads_out, unsigned* done_counter,
                           hipStream_t stream);
int launch_mlp_predict_gen(const float* X, int B, int draw, int inp, int hid,
                           int cls, const float* mean, const float* invstd,
                           const unsigned short* wimg, const float* master,
                           int* preds, float* probs, hipStream_t stream);
void launch_adam_step_gen(float* master, unsigned short* bfmirror,
                          const float* grads, float* m, float* v, int* t_dev,
                          int nparam, int inp, int hid, int cpad, float lr,
                          float beta1, float beta2, float eps,
                          unsigned short* wimg, hipStream_t stream);

// regression head (squared error over 1..32 targets): same slabs, same
// return codes. Yt [B][cpad] fp32 standardized targets, pad columns zero,
// 16-byte aligned; out [B][ldo] fp32, ldo >= targets, receives
// z * y_scale + y_mean in the first `targets` columns.
int launch_mlp_step_reg_gen(const unsigned short* Xbf, const float* Yt, int B,
                            int inp, int hid, int targets, int rt,
                            const unsigned short* wimg, const float* master,
                            float* slabs, int slab_stride, int max_slabs,
                            float invBtot, hipStream_t stream);
int launch_mlp_predict_reg_gen(const float* X, int B, int draw, int inp, int hid,
                               int targets, const float* mean,
                               const float* invstd, const unsigned short* wimg,
                               const float* master, const float* y_mean,
                               const float* y_scale, float* out, int ldo,
                               hipStream_t stream);

// ---- tabular_eval.hip (forward-only metrics, any geometry) -------------------

// rows per workgroup of the evaluation kernel for a padded (hid, cpad): the
// RT of the table's predict row; 0 when there is none
int eval_rows_per_wg(int hid, int cpad);
// Two launches: the metrics kernel (one partial row per workgroup into
// part [part_rows][part_stride]) and the finish kernel, which writes one
// record to hist[min(*slot, cap - 1)] (rows of hist_stride floats) and
// advances *slot. -1: fewer partial rows than workgroups; -3 also for a
// part or hist row narrower than the record, or cap < 1.
int launch_mlp_eval_gen(const unsigned short* Xbf, const int* y, int B, int inp,
                        int hid, int cls, const unsigned short* wimg,
                        const float* master, float* part, int part_rows,
                        int part_stride, float* hist, int hist_stride, int cap,
                        int* slot, hipStream_t stream);
int launch_mlp_eval_reg_gen(const unsigned short* Xbf, const float* Yt, int B,
                            int inp, int hid, int targets,
                            const unsigned short* wimg, const float* master,
                            float* part, int part_rows, int part_stride,
                            float* hist, int hist_stride, int cap, int* slot,
                            hipStream_t stream);

}  // extern "C"
