// Torch bindings for the CDNA4 tabular hot-path kernels
// (tabular_kernels.hip, tabular_gen.hip; launchers and layout constants:
// tabular_launch.h). All launches go to the current torch stream so they
// compose with torch.cuda.graphs capture and RCCL work.

#include <climits>

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "tabular_launch.h"

namespace {

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void check(const torch::Tensor& t, torch::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dtype, name, " has wrong dtype");
}

const unsigned short* bf16_ptr(const torch::Tensor& t) {
  return reinterpret_cast<const unsigned short*>(t.data_ptr());
}

unsigned short* bf16_mut_ptr(const torch::Tensor& t) {
  return reinterpret_cast<unsigned short*>(t.data_ptr());
}

// optional tensor -> checked data pointer, or null when absent
template <typename T>
T* opt_ptr(const c10::optional<torch::Tensor>& t, torch::ScalarType dtype,
           const char* name, int64_t min_numel = 0) {
  if (!t.has_value()) return nullptr;
  check(*t, dtype, name);
  TORCH_CHECK(t->numel() >= min_numel, name, " too small: needs ", min_numel,
              " elements");
  return reinterpret_cast<T*>(t->data_ptr());
}

// the specialized kernels' packed weight image has one fixed size
unsigned short* digits_wimg_ptr(const c10::optional<torch::Tensor>& wimg) {
  TORCH_CHECK(!wimg.has_value() || wimg->numel() == DIGITS_WIMG_N,
              "wimg must be the packed ", DIGITS_WIMG_N, "-elem image buffer");
  return opt_ptr<unsigned short>(wimg, torch::kBFloat16, "wimg");
}

// Adam state as every optimizer entry point takes it
struct AdamState {
  float* master;
  unsigned short* bfmirror;
  float* m;
  float* v;
  int* t_dev;
};

AdamState adam_state(const torch::Tensor& master, const torch::Tensor& bfmirror,
                     const torch::Tensor& m, const torch::Tensor& v,
                     const torch::Tensor& t_dev, int64_t nparam) {
  check(master, torch::kFloat32, "master");
  check(bfmirror, torch::kBFloat16, "bfmirror");
  check(m, torch::kFloat32, "m");
  check(v, torch::kFloat32, "v");
  check(t_dev, torch::kInt32, "t_dev");
  TORCH_CHECK(master.numel() >= nparam && bfmirror.numel() >= nparam &&
                  m.numel() >= nparam && v.numel() >= nparam && t_dev.numel() >= 1,
              "Adam state too small: master/bfmirror/m/v need ", nparam,
              " elements, t_dev one");
  return {master.data_ptr<float>(), bf16_mut_ptr(bfmirror), m.data_ptr<float>(),
          v.data_ptr<float>(), t_dev.data_ptr<int>()};
}

int gen_nparam(int64_t inp, int64_t hid, int64_t cpad) {
  return (int)(inp * hid + hid + hid * cpad + cpad);
}

}  // namespace

void standardize_fit(torch::Tensor X, torch::Tensor mean, torch::Tensor invstd,
                     double eps) {
  check(X, torch::kFloat32, "X");
  check(mean, torch::kFloat32, "mean");
  check(invstd, torch::kFloat32, "invstd");
  const int D = (int)X.size(1);
  TORCH_CHECK(mean.numel() == D && invstd.numel() == D, "mean/invstd size mismatch");
  double* scratch_ptr = nullptr;
  torch::Tensor scratch;
  if (D <= 256 && 256 % D == 0) {
    scratch = torch::zeros({2 * D}, mean.options().dtype(torch::kFloat64));
    scratch_ptr = scratch.data_ptr<double>();
  }
  launch_standardize_fit(X.data_ptr<float>(), X.size(0), D, mean.data_ptr<float>(),
                         invstd.data_ptr<float>(), (float)eps, scratch_ptr,
                         current_stream());
}

void standardize_apply(torch::Tensor X, torch::Tensor mean, torch::Tensor invstd,
                       torch::Tensor out_bf16) {
  check(X, torch::kFloat32, "X");
  check(out_bf16, torch::kBFloat16, "out");
  TORCH_CHECK(out_bf16.dim() == 2 && out_bf16.size(0) == X.size(0) &&
                  out_bf16.size(1) >= X.size(1),
              "out must be [N][Dout] with Dout >= D");
  launch_standardize_apply(X.data_ptr<float>(), X.size(0), (int)X.size(1),
                           (int)out_bf16.size(1), mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), bf16_mut_ptr(out_bf16),
                           current_stream());
}

void mlp_step(torch::Tensor Xbf, torch::Tensor y, torch::Tensor W1bf,
              torch::Tensor W2bf, torch::Tensor master, torch::Tensor grads,
              double invBtot) {
  check(Xbf, torch::kBFloat16, "Xbf");
  check(y, torch::kInt32, "y");
  check(W1bf, torch::kBFloat16, "W1bf");
  check(W2bf, torch::kBFloat16, "W2bf");
  check(master, torch::kFloat32, "master");
  check(grads, torch::kFloat32, "grads");
  TORCH_CHECK(Xbf.size(1) == DIGITS_IN, "IN must be ", DIGITS_IN);
  TORCH_CHECK(W1bf.numel() == DIGITS_IN * DIGITS_HID &&
                  W2bf.numel() == DIGITS_HID * DIGITS_CPAD,
              "weight shapes");
  TORCH_CHECK(grads.numel() >= DIGITS_NPARAM + 1, "grads must hold ",
              DIGITS_NPARAM, " params + loss");
  launch_mlp_step(bf16_ptr(Xbf), y.data_ptr<int>(), (int)Xbf.size(0),
                  bf16_ptr(W1bf), bf16_ptr(W2bf), master.data_ptr<float>(),
                  grads.data_ptr<float>(), (float)invBtot, current_stream());
}

bool mlp_step_fused(torch::Tensor Xbf, torch::Tensor y, torch::Tensor W1bf,
                    torch::Tensor W2bf, torch::Tensor master, torch::Tensor bfmirror,
                    torch::Tensor m, torch::Tensor v, torch::Tensor t_dev,
                    torch::Tensor slabs, torch::Tensor counter,
                    torch::Tensor loss_out, double invBtot, double lr,
                    double beta1, double beta2, double eps,
                    c10::optional<torch::Tensor> grads_out = c10::nullopt,
                    c10::optional<torch::Tensor> wimg = c10::nullopt) {
  check(Xbf, torch::kBFloat16, "Xbf");
  check(y, torch::kInt32, "y");
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, DIGITS_NPARAM);
  check(slabs, torch::kFloat32, "slabs");
  check(counter, torch::kUInt32, "counter");
  check(loss_out, torch::kFloat32, "loss_out");
  TORCH_CHECK(Xbf.size(1) == DIGITS_IN, "IN must be ", DIGITS_IN);
  TORCH_CHECK(slabs.dim() == 2 && slabs.size(1) == DIGITS_SLAB, "slabs must be [n][",
              DIGITS_SLAB, "]");
  const int rc = launch_mlp_step_fused(
      bf16_ptr(Xbf), y.data_ptr<int>(), (int)Xbf.size(0), bf16_ptr(W1bf),
      bf16_ptr(W2bf), st.master, st.bfmirror, st.m, st.v, st.t_dev,
      slabs.data_ptr<float>(), (unsigned*)counter.data_ptr(),
      loss_out.data_ptr<float>(), (float)invBtot, (float)lr, (float)beta1,
      (float)beta2, (float)eps, (int)slabs.size(0),
      opt_ptr<float>(grads_out, torch::kFloat32, "grads_out", DIGITS_NPARAM + 1),
      digits_wimg_ptr(wimg), current_stream());
  TORCH_CHECK(rc != -2, "mlp_step_fused: hipFuncSetAttribute(LDS) failed");
  return rc == 0;
}

bool mlp_train_steps(torch::Tensor Xbf, torch::Tensor y, int64_t batch,
                     int64_t n_steps, torch::Tensor master, torch::Tensor bfmirror,
                     torch::Tensor m, torch::Tensor v, torch::Tensor t_dev,
                     torch::Tensor loss_out, double lr, double beta1, double beta2,
                     double eps) {
  check(Xbf, torch::kBFloat16, "Xbf");
  check(y, torch::kInt32, "y");
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, DIGITS_NPARAM);
  check(loss_out, torch::kFloat32, "loss_out");
  TORCH_CHECK(Xbf.size(1) == DIGITS_IN, "IN must be ", DIGITS_IN);
  const int rc = launch_mlp_train_steps(
      bf16_ptr(Xbf), y.data_ptr<int>(), Xbf.size(0), (int)batch, (int)n_steps,
      st.master, st.bfmirror, st.m, st.v, st.t_dev, loss_out.data_ptr<float>(),
      (float)lr, (float)beta1, (float)beta2, (float)eps, current_stream());
  TORCH_CHECK(rc != -2, "mlp_train_steps: hipFuncSetAttribute(LDS) failed");
  return rc == 0;   // false -> shape constraints unmet, caller falls back
}

void mlp_predict(torch::Tensor X, torch::Tensor mean, torch::Tensor invstd,
                 torch::Tensor W1bf, torch::Tensor W2bf, torch::Tensor master,
                 torch::Tensor preds, c10::optional<torch::Tensor> probs) {
  check(X, torch::kFloat32, "X");
  check(preds, torch::kInt32, "preds");
  TORCH_CHECK(X.size(1) == DIGITS_IN, "IN must be ", DIGITS_IN);
  launch_mlp_predict(X.data_ptr<float>(), (int)X.size(0), mean.data_ptr<float>(),
                     invstd.data_ptr<float>(), bf16_ptr(W1bf), bf16_ptr(W2bf),
                     master.data_ptr<float>(), preds.data_ptr<int>(),
                     opt_ptr<float>(probs, torch::kFloat32, "probs"),
                     current_stream());
}

void adam_step(torch::Tensor master, torch::Tensor bfmirror, torch::Tensor grads,
               torch::Tensor m, torch::Tensor v, torch::Tensor t_dev, double lr,
               double beta1, double beta2, double eps,
               c10::optional<torch::Tensor> wimg = c10::nullopt) {
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, DIGITS_NPARAM);
  check(grads, torch::kFloat32, "grads");
  launch_adam_step(st.master, st.bfmirror, grads.data_ptr<float>(), st.m, st.v,
                   st.t_dev, (float)lr, (float)beta1, (float)beta2, (float)eps,
                   digits_wimg_ptr(wimg), current_stream());
}

torch::Tensor reduce_selftest(torch::Tensor x) {
  check(x, torch::kFloat32, "x");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == 64, "x must be [n][64]");
  TORCH_CHECK(x.size(0) <= INT_MAX, "too many rows");
  torch::Tensor out = torch::empty({x.size(0), 64, 2}, x.options());
  launch_reduce_selftest(x.data_ptr<float>(), (int)x.size(0),
                         out.data_ptr<float>(), current_stream());
  return out;
}

// ---------------------------------------------------------------------------
// generalized-geometry (any in_features/hidden/classes) entry points
// ---------------------------------------------------------------------------

bool mlp_step_gen(torch::Tensor Xbf, torch::Tensor y, int64_t hid, int64_t cls,
                  int64_t rt, torch::Tensor wimg, torch::Tensor master,
                  torch::Tensor slabs, double invBtot) {
  check(Xbf, torch::kBFloat16, "Xbf");
  check(y, torch::kInt32, "y");
  check(wimg, torch::kBFloat16, "wimg");
  check(master, torch::kFloat32, "master");
  check(slabs, torch::kFloat32, "slabs");
  const int inp = (int)Xbf.size(1);
  const int cpad = cls <= 16 ? 16 : 32;
  const int nparam = gen_nparam(inp, hid, cpad);
  TORCH_CHECK(inp % 32 == 0, "staged input width must be a multiple of 32");
  TORCH_CHECK(master.numel() >= nparam, "master too small for geometry");
  TORCH_CHECK(wimg.numel() >= (int64_t)hid * inp + hid * 32 + cpad * hid,
              "wimg too small for geometry");
  TORCH_CHECK(slabs.dim() == 2 && slabs.size(1) >= nparam + 2,
              "slabs must be [n][>= nparam+2]");
  const int rc = launch_mlp_step_gen(
      bf16_ptr(Xbf), y.data_ptr<int>(), (int)Xbf.size(0), inp, (int)hid,
      (int)cls, (int)rt, bf16_ptr(wimg), master.data_ptr<float>(),
      slabs.data_ptr<float>(), (int)slabs.size(1), (int)slabs.size(0),
      (float)invBtot, current_stream());
  TORCH_CHECK(rc != -2, "mlp_step_gen: hipFuncSetAttribute(LDS) failed");
  TORCH_CHECK(rc != -3, "mlp_step_gen: unsupported geometry (hid=", hid,
              " inp=", inp, " cls=", cls, " rt=", rt, ")");
  return rc == 0;  // false -> more WGs than slab rows, caller re-sizes
}

void reduce_adam_gen(torch::Tensor slabs, int64_t n_wg, int64_t inp, int64_t hid,
                     int64_t cpad, torch::Tensor master, torch::Tensor bfmirror,
                     torch::Tensor m, torch::Tensor v, torch::Tensor t_dev,
                     torch::Tensor counter, torch::Tensor loss_out, double lr,
                     double beta1, double beta2, double eps,
                     c10::optional<torch::Tensor> wimg = c10::nullopt,
                     c10::optional<torch::Tensor> grads_out = c10::nullopt) {
  check(counter, torch::kUInt32, "counter");
  check(slabs, torch::kFloat32, "slabs");
  check(loss_out, torch::kFloat32, "loss_out");
  TORCH_CHECK(cpad == 16 || cpad == 32, "cpad must be 16 or 32");
  const int nparam = gen_nparam(inp, hid, cpad);
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, nparam);
  TORCH_CHECK(slabs.dim() == 2 && slabs.size(1) >= nparam + 2, "slab stride");
  TORCH_CHECK(n_wg >= 1 && n_wg <= slabs.size(0), "n_wg out of range");
  launch_reduce_adam_gen(
      slabs.data_ptr<float>(), (int)n_wg, (int)slabs.size(1), (int)inp, (int)hid,
      (int)cpad, st.master, st.bfmirror, st.m, st.v, st.t_dev,
      loss_out.data_ptr<float>(), (float)lr, (float)beta1, (float)beta2,
      (float)eps, opt_ptr<unsigned short>(wimg, torch::kBFloat16, "wimg"),
      opt_ptr<float>(grads_out, torch::kFloat32, "grads_out", nparam + 1),
      (unsigned*)counter.data_ptr(), current_stream());
}

void mlp_predict_gen(torch::Tensor X, int64_t inp, int64_t hid, int64_t cls,
                     torch::Tensor mean, torch::Tensor invstd, torch::Tensor wimg,
                     torch::Tensor master, torch::Tensor preds,
                     c10::optional<torch::Tensor> probs) {
  check(X, torch::kFloat32, "X");
  check(wimg, torch::kBFloat16, "wimg");
  check(master, torch::kFloat32, "master");
  check(preds, torch::kInt32, "preds");
  TORCH_CHECK(mean.numel() == X.size(1) && invstd.numel() == X.size(1),
              "mean/invstd must match raw feature width");
  const int rc = launch_mlp_predict_gen(
      X.data_ptr<float>(), (int)X.size(0), (int)X.size(1), (int)inp, (int)hid,
      (int)cls, mean.data_ptr<float>(), invstd.data_ptr<float>(), bf16_ptr(wimg),
      master.data_ptr<float>(), preds.data_ptr<int>(),
      opt_ptr<float>(probs, torch::kFloat32, "probs"), current_stream());
  TORCH_CHECK(rc == 0, "mlp_predict_gen: unsupported geometry or LDS failure");
}

void adam_step_gen(torch::Tensor master, torch::Tensor bfmirror,
                   torch::Tensor grads, torch::Tensor m, torch::Tensor v,
                   torch::Tensor t_dev, int64_t inp, int64_t hid, int64_t cpad,
                   double lr, double beta1, double beta2, double eps,
                   c10::optional<torch::Tensor> wimg = c10::nullopt) {
  check(grads, torch::kFloat32, "grads");
  TORCH_CHECK(cpad == 16 || cpad == 32, "cpad must be 16 or 32");
  const int nparam = gen_nparam(inp, hid, cpad);
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, nparam);
  launch_adam_step_gen(st.master, st.bfmirror, grads.data_ptr<float>(), st.m,
                       st.v, st.t_dev, nparam, (int)inp, (int)hid, (int)cpad,
                       (float)lr, (float)beta1, (float)beta2, (float)eps,
                       opt_ptr<unsigned short>(wimg, torch::kBFloat16, "wimg"),
                       current_stream());
}

// ---------------------------------------------------------------------------
// regression head of the generalized kernels (squared error, 1..32 targets)
// ---------------------------------------------------------------------------

bool mlp_step_reg_gen(torch::Tensor Xbf, torch::Tensor Yt, int64_t hid,
                      int64_t targets, int64_t rt, torch::Tensor wimg,
                      torch::Tensor master, torch::Tensor slabs, double invBtot) {
  check(Xbf, torch::kBFloat16, "Xbf");
  check(Yt, torch::kFloat32, "Yt");
  check(wimg, torch::kBFloat16, "wimg");
  check(master, torch::kFloat32, "master");
  check(slabs, torch::kFloat32, "slabs");
  TORCH_CHECK(targets >= 1 && targets <= 32, "targets must be 1..32");
  TORCH_CHECK(Xbf.dim() == 2 && Xbf.size(0) >= 1, "Xbf must be [B][inp], B >= 1");
  const int inp = (int)Xbf.size(1);
  const int cpad = targets <= 16 ? 16 : 32;
  const int nparam = gen_nparam(inp, hid, cpad);
  TORCH_CHECK(inp % 32 == 0, "staged input width must be a multiple of 32");
  // the kernel reads a row's targets as aligned 16-byte groups of a
  // [B][cpad] matrix (TabularMLPRegressor.stage_targets builds it)
  TORCH_CHECK(Yt.dim() == 2 && Yt.size(0) == Xbf.size(0) && Yt.size(1) == cpad,
              "Yt must be [B][", cpad, "] standardized targets, zero-padded");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(Yt.data_ptr()) % 16 == 0,
              "Yt must be 16-byte aligned");
  TORCH_CHECK(master.numel() >= nparam, "master too small for geometry");
  TORCH_CHECK(wimg.numel() >= (int64_t)hid * inp + hid * 32 + cpad * hid,
              "wimg too small for geometry");
  TORCH_CHECK(slabs.dim() == 2 && slabs.size(1) >= nparam + 2,
              "slabs must be [n][>= nparam+2]");
  const int rc = launch_mlp_step_reg_gen(
      bf16_ptr(Xbf), Yt.data_ptr<float>(), (int)Xbf.size(0), inp, (int)hid,
      (int)targets, (int)rt, bf16_ptr(wimg), master.data_ptr<float>(),
      slabs.data_ptr<float>(), (int)slabs.size(1), (int)slabs.size(0),
      (float)invBtot, current_stream());
  TORCH_CHECK(rc != -2, "mlp_step_reg_gen: hipFuncSetAttribute(LDS) failed");
  TORCH_CHECK(rc != -3, "mlp_step_reg_gen: unsupported geometry (hid=", hid,
              " inp=", inp, " targets=", targets, " rt=", rt, ")");
  return rc == 0;  // false -> more WGs than slab rows, caller re-sizes
}

void mlp_predict_reg_gen(torch::Tensor X, int64_t inp, int64_t hid,
                         int64_t targets, torch::Tensor mean,
                         torch::Tensor invstd, torch::Tensor wimg,
                         torch::Tensor master, torch::Tensor y_mean,
                         torch::Tensor y_scale, torch::Tensor out) {
  check(X, torch::kFloat32, "X");
  check(mean, torch::kFloat32, "mean");
  check(invstd, torch::kFloat32, "invstd");
  check(wimg, torch::kBFloat16, "wimg");
  check(master, torch::kFloat32, "master");
  check(y_mean, torch::kFloat32, "y_mean");
  check(y_scale, torch::kFloat32, "y_scale");
  check(out, torch::kFloat32, "out");
  TORCH_CHECK(targets >= 1 && targets <= 32, "targets must be 1..32");
  const int cpad = targets <= 16 ? 16 : 32;
  TORCH_CHECK(X.dim() == 2 && X.size(0) >= 1 && X.size(1) <= inp,
              "X must be [B][<= inp], B >= 1");
  TORCH_CHECK(mean.numel() == X.size(1) && invstd.numel() == X.size(1),
              "mean/invstd must match raw feature width");
  TORCH_CHECK(master.numel() >= gen_nparam(inp, hid, cpad),
              "master too small for geometry");
  TORCH_CHECK(wimg.numel() >= hid * inp + hid * 32 + cpad * hid,
              "wimg too small for geometry");
  TORCH_CHECK(y_mean.numel() == targets && y_scale.numel() == targets,
              "y_mean/y_scale must hold one entry per target");
  TORCH_CHECK(out.dim() == 2 && out.size(0) >= X.size(0) && out.size(1) >= targets,
              "out must be [>= B][>= targets]");
  const int rc = launch_mlp_predict_reg_gen(
      X.data_ptr<float>(), (int)X.size(0), (int)X.size(1), (int)inp, (int)hid,
      (int)targets, mean.data_ptr<float>(), invstd.data_ptr<float>(),
      bf16_ptr(wimg), master.data_ptr<float>(), y_mean.data_ptr<float>(),
      y_scale.data_ptr<float>(), out.data_ptr<float>(), (int)out.size(1),
      current_stream());
  TORCH_CHECK(rc == 0, "mlp_predict_reg_gen: unsupported geometry or LDS failure");
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  // specialized (digits) layout numbers the host side stages buffers with
  m.attr("WIMG_N") = DIGITS_WIMG_N;   // packed weight image, bf16 elements
  m.attr("SLAB") = DIGITS_SLAB;       // gradient slab stride, floats
  m.attr("XS") = DIGITS_XS;           // image row stride of W1T
  m.attr("WS") = DIGITS_WS;           // image row stride of W2s / W2T
  m.def("standardize_fit", &standardize_fit, "column mean/invstd (CDNA4)");
  m.def("standardize_apply", &standardize_apply, "(x-mean)*invstd -> bf16 (CDNA4)");
  m.def("mlp_step", &mlp_step, "fused MLP fwd+bwd step (CDNA4 MFMA)");
  m.def("mlp_step_fused", &mlp_step_fused,
        "fully-fused step: fwd+bwd + cross-WG slab reduction + Adam in one "
        "launch; with grads_out, reduce-only (the DP pre-collective kernel)",
        py::arg("Xbf"), py::arg("y"), py::arg("W1bf"), py::arg("W2bf"),
        py::arg("master"), py::arg("bfmirror"), py::arg("m"), py::arg("v"),
        py::arg("t_dev"), py::arg("slabs"), py::arg("counter"),
        py::arg("loss_out"), py::arg("invBtot"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("grads_out") = c10::nullopt,
        py::arg("wimg") = c10::nullopt);
  m.def("mlp_train_steps", &mlp_train_steps,
        "persistent multi-step training kernel (weights+Adam resident in LDS)");
  m.def("mlp_predict", &mlp_predict, "fused standardize+fwd+argmax (CDNA4 MFMA)");
  m.def("adam_step", &adam_step, "fused Adam on flat master params (CDNA4)",
        py::arg("master"), py::arg("bfmirror"), py::arg("grads"), py::arg("m"),
        py::arg("v"), py::arg("t_dev"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("wimg") = c10::nullopt);
  m.def("reduce_selftest", &reduce_selftest,
        "x [n][64] -> [n][64][2]: in-row sums of 16 by the DPP helper and by "
        "the shuffle butterfly (must be bit-equal)",
        py::arg("x"));
  m.def("mlp_step_gen", &mlp_step_gen,
        "generalized fused step: any (in,hid,cls) geometry; double-buffered "
        "K-tiled MFMA fwd+bwd producing per-WG gradient slabs",
        py::arg("Xbf"), py::arg("y"), py::arg("hid"), py::arg("cls"),
        py::arg("rt"), py::arg("wimg"), py::arg("master"), py::arg("slabs"),
        py::arg("invBtot"));
  m.def("reduce_adam_gen", &reduce_adam_gen,
        "wide-grid slab reduction + fused Adam (grads_out: reduce-only, the "
        "DP pre-collective mode)",
        py::arg("slabs"), py::arg("n_wg"), py::arg("inp"), py::arg("hid"),
        py::arg("cpad"), py::arg("master"), py::arg("bfmirror"), py::arg("m"),
        py::arg("v"), py::arg("t_dev"), py::arg("counter"), py::arg("loss_out"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("wimg") = c10::nullopt, py::arg("grads_out") = c10::nullopt);
  m.def("mlp_predict_gen", &mlp_predict_gen,
        "generalized fused standardize+fwd+argmax",
        py::arg("X"), py::arg("inp"), py::arg("hid"), py::arg("cls"),
        py::arg("mean"), py::arg("invstd"), py::arg("wimg"), py::arg("master"),
        py::arg("preds"), py::arg("probs") = c10::nullopt);
  m.def("adam_step_gen", &adam_step_gen,
        "generalized fused Adam (runtime param count; DP path)",
        py::arg("master"), py::arg("bfmirror"), py::arg("grads"), py::arg("m"),
        py::arg("v"), py::arg("t_dev"), py::arg("inp"), py::arg("hid"),
        py::arg("cpad"), py::arg("lr"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("wimg") = c10::nullopt);
  m.def("mlp_step_reg_gen", &mlp_step_reg_gen,
        "generalized fused step with the regression head: squared error "
        "over 1..32 standardized targets Yt [B][cpad]; same slabs as "
        "mlp_step_gen",
        py::arg("Xbf"), py::arg("Yt"), py::arg("hid"), py::arg("targets"),
        py::arg("rt"), py::arg("wimg"), py::arg("master"), py::arg("slabs"),
        py::arg("invBtot"));
  m.def("mlp_predict_reg_gen", &mlp_predict_reg_gen,
        "generalized fused standardize+fwd with the regression head: "
        "out[b][t] = z * y_scale[t] + y_mean[t]",
        py::arg("X"), py::arg("inp"), py::arg("hid"), py::arg("targets"),
        py::arg("mean"), py::arg("invstd"), py::arg("wimg"), py::arg("master"),
        py::arg("y_mean"), py::arg("y_scale"), py::arg("out"));
}
