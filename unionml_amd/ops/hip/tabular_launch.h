// Host-visible interface of the tabular kernels: the digits-geometry
// layout constants and every extern "C" launcher, declared ONCE. Both
// kernel files and the torch bindings include this header, so a launcher
// whose definition drifts from its declaration is a compile error instead
// of a silently mis-ordered argument list.
//
// The constants carry a DIGITS_ prefix: short names such as IN or HID
// clash with macros of other headers and with the generalized kernels'
// template parameters.
#pragma once

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

extern "C" {

// ---- tabular_kernels.hip ---------------------------------------------------

void launch_standardize_fit(const float* X, long long N, int D, float* mean,
                            float* invstd, float eps, double* scratch,
                            hipStream_t stream);
void launch_standardize_apply(const float* X, long long N, int D, int Dout,
                              const float* mean, const float* invstd,
                              unsigned short* out, hipStream_t stream);
void launch_mlp_step(const unsigned short* Xbf, const int* y, int B,
                     const unsigned short* W1bf, const unsigned short* W2bf,
                     const float* master, float* grads, float invBtot,
                     hipStream_t stream);
// -1: more workgroups than slab rows, -2: LDS attribute failed
int launch_mlp_step_fused(const unsigned short* Xbf, const int* y, int B,
                          const unsigned short* W1bf, const unsigned short* W2bf,
                          float* master, unsigned short* bfmirror, float* m,
                          float* v, int* t_dev, float* slabs, unsigned* counter,
                          float* loss_out, float invBtot, float lr, float beta1,
                          float beta2, float eps, int max_slabs, float* grads_out,
                          unsigned short* wimg, hipStream_t stream);
// -1: shape constraints unmet (caller falls back), -2: LDS attribute failed
int launch_mlp_train_steps(const unsigned short* Xbf, const int* y, long long N,
                           int B, int n_steps, float* master,
                           unsigned short* bfmirror, float* m, float* v,
                           int* t_dev, float* loss_out, float lr, float beta1,
                           float beta2, float eps, hipStream_t stream);
void launch_mlp_predict(const float* X, int B, const float* mean,
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

// -1: more workgroups than slab rows, -2: LDS attribute failed,
// -3: no instantiation for the geometry
int launch_mlp_step_gen(const unsigned short* Xbf, const int* y, int B, int inp,
                        int hid, int cls, int rt, const unsigned short* wimg,
                        const float* master, float* slabs, int slab_stride,
                        int max_slabs, float invBtot, hipStream_t stream);
void launch_reduce_adam_gen(const float* slabs, int n_wg, int slab_stride,
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

}  // extern "C"
