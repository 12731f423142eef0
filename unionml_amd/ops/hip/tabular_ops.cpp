// Torch bindings for the CDNA4 tabular hot-path kernels
// (tabular_kernels.hip, tabular_gen.hip, tabular_eval.hip, tabular_shuffle.hip;
// launchers and layout constants: tabular_launch.h, tabular_shuffle.h). All launches go to the current torch
// stream so they compose with torch.cuda.graphs capture and RCCL work.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include "tabular_launch.h"
#include "tabular_shuffle.h"

namespace {

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void check(const torch::Tensor& t, torch::ScalarType dtype, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device tensor");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dtype, name, " has wrong dtype");
}

// check() plus a least (or, with exact, the only) element count
void check_n(const torch::Tensor& t, torch::ScalarType dtype, const char* name,
             int64_t numel, bool exact = false) {
  check(t, dtype, name);
  TORCH_CHECK(exact ? t.numel() == numel : t.numel() >= numel, name, " must hold ",
              exact ? "exactly " : "at least ", numel, " elements, has ", t.numel());
}

// the kernels load 16-byte vectors from these
void check_aligned16(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0, name,
              " must be 16-byte aligned");
}

// a [B][cols] matrix, 1 <= B <= max_rows -> B (cols 0: any width 1..INT_MAX).
// max_rows is INT_MAX where the launcher takes int B, INT64_MAX where it
// takes long long N.
int64_t check_rows(const torch::Tensor& t, torch::ScalarType dtype, const char* name,
                   int64_t cols = 0, int64_t max_rows = INT_MAX) {
  check(t, dtype, name);
  TORCH_CHECK(t.dim() == 2 && t.size(0) >= 1 && t.size(0) <= max_rows &&
                  t.size(1) >= 1 && t.size(1) <= INT_MAX &&
                  (cols == 0 || t.size(1) == cols),
              name, " must be [1 <= B <= ", max_rows, "][",
              cols ? std::to_string(cols) : std::string("1 <= width <= INT_MAX"),
              "], is ", t.sizes());
  return t.size(0);
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
  check_n(*t, dtype, name, min_numel);
  return reinterpret_cast<T*>(t->data_ptr());
}

// optional class probabilities [>= B][cls], dense
float* probs_ptr(const c10::optional<torch::Tensor>& probs, int B, int64_t cls) {
  TORCH_CHECK(!probs.has_value() || (probs->dim() == 2 && probs->size(0) >= B &&
                                     probs->size(1) == cls),
              "probs must be [>= ", B, "][", cls, "]");
  return opt_ptr<float>(probs, torch::kFloat32, "probs");
}

// feature standardizer of a raw [N][D] matrix
void check_scaler(const torch::Tensor& mean, const torch::Tensor& invstd, int64_t D) {
  check_n(mean, torch::kFloat32, "mean", D, true);
  check_n(invstd, torch::kFloat32, "invstd", D, true);
}

// gradient slabs [n][stride >= min_stride] (exact: the digits stride)
void check_slabs(const torch::Tensor& slabs, int64_t min_stride, bool exact = false) {
  check(slabs, torch::kFloat32, "slabs");
  TORCH_CHECK(slabs.dim() == 2 && slabs.size(0) <= INT_MAX &&
                  slabs.size(1) <= INT_MAX &&
                  (exact ? slabs.size(1) == min_stride : slabs.size(1) >= min_stride),
              "slabs must be [n][", exact ? "" : ">= ", min_stride, "], is ",
              slabs.sizes());
}

// ---- the digits state --------------------------------------------------------

// the specialized kernels' packed weight image has one fixed size
unsigned short* digits_wimg_ptr(const c10::optional<torch::Tensor>& wimg) {
  TORCH_CHECK(!wimg.has_value() || wimg->numel() == DIGITS_WIMG_N,
              "wimg must be the packed ", DIGITS_WIMG_N, "-elem image buffer");
  if (wimg.has_value()) check_aligned16(*wimg, "wimg");
  return opt_ptr<unsigned short>(wimg, torch::kBFloat16, "wimg");
}

// a staged digits batch: Xbf [B][64] bf16 and one int32 label per row -> B
int64_t digits_batch(const torch::Tensor& Xbf, const torch::Tensor& y,
                     int64_t max_rows = INT_MAX) {
  const int64_t B = check_rows(Xbf, torch::kBFloat16, "Xbf", DIGITS_IN, max_rows);
  check_aligned16(Xbf, "Xbf");
  check_n(y, torch::kInt32, "y", B, true);
  return B;
}

// the bf16 weight views and the fp32 master every specialized kernel reads
void digits_weights(const torch::Tensor& W1bf, const torch::Tensor& W2bf,
                    const torch::Tensor& master) {
  check_n(W1bf, torch::kBFloat16, "W1bf", DIGITS_IN * DIGITS_HID, true);
  check_n(W2bf, torch::kBFloat16, "W2bf", DIGITS_HID * DIGITS_CPAD, true);
  check_n(master, torch::kFloat32, "master", DIGITS_NPARAM);
}

// what a specialized launcher returned -> the binding's result
bool digits_launched(int rc, const char* fn) {
  TORCH_CHECK(rc != -2, fn, ": hipFuncSetAttribute(LDS) failed");
  TORCH_CHECK(rc != -3, fn, ": arguments outside the kernel's range");
  return rc == 0;   // false (-1): the caller re-sizes or falls back
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
  check_n(master, torch::kFloat32, "master", nparam);
  check_n(bfmirror, torch::kBFloat16, "bfmirror", nparam);
  check_n(m, torch::kFloat32, "m", nparam);
  check_n(v, torch::kFloat32, "v", nparam);
  check_n(t_dev, torch::kInt32, "t_dev", 1);
  return {master.data_ptr<float>(), bf16_mut_ptr(bfmirror), m.data_ptr<float>(),
          v.data_ptr<float>(), t_dev.data_ptr<int>()};
}

// ---- the generalized family ----------------------------------------------------

// the padded geometry (inp, hid, cpad), refused when the kernels could not
// index it; gen_geometry_for: the same from n_out classes or targets
GenGeometry gen_geometry(int64_t inp, int64_t hid, int64_t cpad) {
  TORCH_CHECK(cpad == 16 || cpad == 32, "cpad must be 16 or 32");
  const GenGeometry g{inp, hid, cpad};
  TORCH_CHECK(g.ok(), "unsupported geometry: inp=", inp, " must be a positive ",
              "multiple of 32, hid=", hid, " positive, and nparam and the weight ",
              "image must fit an int");
  return g;
}

GenGeometry gen_geometry_for(int64_t inp, int64_t hid, int64_t n_out,
                             const char* what) {
  TORCH_CHECK(n_out >= 1 && n_out <= 32, what, " must be 1..32");
  return gen_geometry(inp, hid, GenGeometry::cpad_for(n_out));
}

// the packed image and the master the step and the predict kernels read
void gen_weights(const GenGeometry& g, const torch::Tensor& wimg,
                 const torch::Tensor& master) {
  check_n(wimg, torch::kBFloat16, "wimg", g.wimg_n());
  check_aligned16(wimg, "wimg");
  check_n(master, torch::kFloat32, "master", g.nparam());
}

// what the two helpers below return: the call's geometry and batch rows
struct GenCall {
  GenGeometry g;
  int B;
};

// A generalized step's arguments, either head: all but the per-row targets,
// which the head's binding holds to B.
GenCall gen_step_args(const torch::Tensor& Xbf, int64_t hid, int64_t n_out,
                      const char* n_out_name, int64_t rt,
                      const torch::Tensor& wimg, const torch::Tensor& master,
                      const torch::Tensor& slabs) {
  const int B = (int)check_rows(Xbf, torch::kBFloat16, "Xbf");
  check_aligned16(Xbf, "Xbf");
  const GenGeometry g = gen_geometry_for(Xbf.size(1), hid, n_out, n_out_name);
  TORCH_CHECK(rt >= 1 && rt <= INT_MAX, "rt must be a compiled rows-per-workgroup");
  gen_weights(g, wimg, master);
  check_slabs(slabs, g.min_slab_stride());
  return {g, B};
}

// what a generalized launcher returned -> the binding's result
bool gen_launched(int rc, const char* fn, const GenCall& a, int64_t n_out,
                  int64_t rt = 0) {
  TORCH_CHECK(rc != -2, fn, ": hipFuncSetAttribute(LDS) failed");
  TORCH_CHECK(rc != -3, fn, ": unsupported geometry (hid=", a.g.hid,
              " inp=", a.g.inp, " outputs=", n_out, " rt=", rt, ")");
  return rc == 0;  // false -> more WGs than slab rows, caller re-sizes
}

// A generalized predict's arguments, either head: all but the outputs.
GenCall gen_predict_args(const torch::Tensor& X, int64_t inp, int64_t hid,
                         int64_t n_out, const char* n_out_name,
                         const torch::Tensor& mean, const torch::Tensor& invstd,
                         const torch::Tensor& wimg, const torch::Tensor& master) {
  const int B = (int)check_rows(X, torch::kFloat32, "X");
  const GenGeometry g = gen_geometry_for(inp, hid, n_out, n_out_name);
  TORCH_CHECK(X.size(1) <= inp, "X must be [B][<= inp=", inp, "], is ", X.sizes());
  check_scaler(mean, invstd, X.size(1));
  gen_weights(g, wimg, master);
  return {g, B};
}

}  // namespace

void standardize_fit(torch::Tensor X, torch::Tensor mean, torch::Tensor invstd,
                     double eps) {
  check_rows(X, torch::kFloat32, "X", 0, INT64_MAX);   // long long N below
  const int D = (int)X.size(1);
  check_scaler(mean, invstd, D);
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
  check_rows(X, torch::kFloat32, "X", 0, INT64_MAX);   // long long N below
  check_scaler(mean, invstd, X.size(1));
  check(out_bf16, torch::kBFloat16, "out");
  TORCH_CHECK(out_bf16.dim() == 2 && out_bf16.size(0) == X.size(0) &&
                  out_bf16.size(1) >= X.size(1) && out_bf16.size(1) <= INT_MAX,
              "out must be [N][Dout] with Dout >= D");
  launch_standardize_apply(X.data_ptr<float>(), X.size(0), (int)X.size(1),
                           (int)out_bf16.size(1), mean.data_ptr<float>(),
                           invstd.data_ptr<float>(), bf16_mut_ptr(out_bf16),
                           current_stream());
}

void mlp_step(torch::Tensor Xbf, torch::Tensor y, torch::Tensor W1bf,
              torch::Tensor W2bf, torch::Tensor master, torch::Tensor grads,
              double invBtot) {
  const int B = (int)digits_batch(Xbf, y);
  digits_weights(W1bf, W2bf, master);
  check_n(grads, torch::kFloat32, "grads", DIGITS_NPARAM + 1);
  const int rc = launch_mlp_step(bf16_ptr(Xbf), y.data_ptr<int>(), B,
                                 bf16_ptr(W1bf), bf16_ptr(W2bf),
                                 master.data_ptr<float>(), grads.data_ptr<float>(),
                                 (float)invBtot, current_stream());
  digits_launched(rc, "mlp_step");
}

bool mlp_step_fused(torch::Tensor Xbf, torch::Tensor y, torch::Tensor W1bf,
                    torch::Tensor W2bf, torch::Tensor master, torch::Tensor bfmirror,
                    torch::Tensor m, torch::Tensor v, torch::Tensor t_dev,
                    torch::Tensor slabs, torch::Tensor counter,
                    torch::Tensor loss_out, double invBtot, double lr,
                    double beta1, double beta2, double eps,
                    c10::optional<torch::Tensor> grads_out = c10::nullopt,
                    c10::optional<torch::Tensor> wimg = c10::nullopt) {
  const int B = (int)digits_batch(Xbf, y);
  digits_weights(W1bf, W2bf, master);
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, DIGITS_NPARAM);
  check_slabs(slabs, DIGITS_SLAB, true);
  check_n(counter, torch::kUInt32, "counter", 1);
  check_n(loss_out, torch::kFloat32, "loss_out", 1);
  const int rc = launch_mlp_step_fused(
      bf16_ptr(Xbf), y.data_ptr<int>(), B, bf16_ptr(W1bf), bf16_ptr(W2bf),
      st.master, st.bfmirror, st.m, st.v, st.t_dev, slabs.data_ptr<float>(),
      (unsigned*)counter.data_ptr(), loss_out.data_ptr<float>(), (float)invBtot,
      (float)lr, (float)beta1, (float)beta2, (float)eps, (int)slabs.size(0),
      opt_ptr<float>(grads_out, torch::kFloat32, "grads_out", DIGITS_NPARAM + 1),
      digits_wimg_ptr(wimg), current_stream());
  return digits_launched(rc, "mlp_step_fused");   // false: more WGs than slab rows
}

bool mlp_train_steps(torch::Tensor Xbf, torch::Tensor y, int64_t batch,
                     int64_t n_steps, torch::Tensor master, torch::Tensor bfmirror,
                     torch::Tensor m, torch::Tensor v, torch::Tensor t_dev,
                     torch::Tensor loss_out, double lr, double beta1, double beta2,
                     double eps) {
  const int64_t N = digits_batch(Xbf, y, INT64_MAX);   // the launcher takes long long
  // before the launcher's N % batch
  TORCH_CHECK(batch >= 1 && batch <= INT_MAX, "batch must be 1..INT_MAX, is ", batch);
  TORCH_CHECK(n_steps >= 0 && n_steps <= INT_MAX, "n_steps must be 0..INT_MAX, is ",
              n_steps);
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, DIGITS_NPARAM);
  check_n(loss_out, torch::kFloat32, "loss_out", 1);
  const int rc = launch_mlp_train_steps(
      bf16_ptr(Xbf), y.data_ptr<int>(), N, (int)batch, (int)n_steps, st.master,
      st.bfmirror, st.m, st.v, st.t_dev, loss_out.data_ptr<float>(), (float)lr,
      (float)beta1, (float)beta2, (float)eps, current_stream());
  return digits_launched(rc, "mlp_train_steps");   // false: shape constraints unmet
}

void mlp_predict(torch::Tensor X, torch::Tensor mean, torch::Tensor invstd,
                 torch::Tensor W1bf, torch::Tensor W2bf, torch::Tensor master,
                 torch::Tensor preds, c10::optional<torch::Tensor> probs) {
  const int B = (int)check_rows(X, torch::kFloat32, "X", DIGITS_IN);
  check_scaler(mean, invstd, DIGITS_IN);
  digits_weights(W1bf, W2bf, master);
  check_n(preds, torch::kInt32, "preds", B);
  const int rc = launch_mlp_predict(
      X.data_ptr<float>(), B, mean.data_ptr<float>(), invstd.data_ptr<float>(),
      bf16_ptr(W1bf), bf16_ptr(W2bf), master.data_ptr<float>(),
      preds.data_ptr<int>(), probs_ptr(probs, B, DIGITS_CLS), current_stream());
  digits_launched(rc, "mlp_predict");
}

void adam_step(torch::Tensor master, torch::Tensor bfmirror, torch::Tensor grads,
               torch::Tensor m, torch::Tensor v, torch::Tensor t_dev, double lr,
               double beta1, double beta2, double eps,
               c10::optional<torch::Tensor> wimg = c10::nullopt) {
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, DIGITS_NPARAM);
  check_n(grads, torch::kFloat32, "grads", DIGITS_NPARAM);
  launch_adam_step(st.master, st.bfmirror, grads.data_ptr<float>(), st.m, st.v,
                   st.t_dev, (float)lr, (float)beta1, (float)beta2, (float)eps,
                   digits_wimg_ptr(wimg), current_stream());
}

torch::Tensor reduce_selftest(torch::Tensor x) {
  check_rows(x, torch::kFloat32, "x", 64);
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
  const GenCall a = gen_step_args(Xbf, hid, cls, "cls", rt, wimg, master, slabs);
  check_n(y, torch::kInt32, "y", a.B, true);
  const int rc = launch_mlp_step_gen(
      bf16_ptr(Xbf), y.data_ptr<int>(), a.B, (int)a.g.inp, (int)hid, (int)cls,
      (int)rt, bf16_ptr(wimg), master.data_ptr<float>(), slabs.data_ptr<float>(),
      (int)slabs.size(1), (int)slabs.size(0), (float)invBtot, current_stream());
  return gen_launched(rc, "mlp_step_gen", a, cls, rt);
}

void reduce_adam_gen(torch::Tensor slabs, int64_t n_wg, int64_t inp, int64_t hid,
                     int64_t cpad, torch::Tensor master, torch::Tensor bfmirror,
                     torch::Tensor m, torch::Tensor v, torch::Tensor t_dev,
                     torch::Tensor counter, torch::Tensor loss_out, double lr,
                     double beta1, double beta2, double eps,
                     c10::optional<torch::Tensor> wimg = c10::nullopt,
                     c10::optional<torch::Tensor> grads_out = c10::nullopt) {
  const GenGeometry g = gen_geometry(inp, hid, cpad);
  check_n(counter, torch::kUInt32, "counter", 1);
  check_n(loss_out, torch::kFloat32, "loss_out", 1);
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, g.nparam());
  check_slabs(slabs, g.min_slab_stride());
  TORCH_CHECK(n_wg >= 1 && n_wg <= slabs.size(0), "n_wg must be 1..", slabs.size(0),
              " (the slab rows), is ", n_wg);
  const int rc = launch_reduce_adam_gen(
      slabs.data_ptr<float>(), (int)n_wg, (int)slabs.size(1), (int)inp, (int)hid,
      (int)cpad, st.master, st.bfmirror, st.m, st.v, st.t_dev,
      loss_out.data_ptr<float>(), (float)lr, (float)beta1, (float)beta2,
      (float)eps,
      opt_ptr<unsigned short>(wimg, torch::kBFloat16, "wimg", g.wimg_n()),
      opt_ptr<float>(grads_out, torch::kFloat32, "grads_out", g.nparam() + 1),
      (unsigned*)counter.data_ptr(), current_stream());
  TORCH_CHECK(rc == 0, "reduce_adam_gen: unsupported geometry");
}

void mlp_predict_gen(torch::Tensor X, int64_t inp, int64_t hid, int64_t cls,
                     torch::Tensor mean, torch::Tensor invstd, torch::Tensor wimg,
                     torch::Tensor master, torch::Tensor preds,
                     c10::optional<torch::Tensor> probs) {
  const GenCall a =
      gen_predict_args(X, inp, hid, cls, "cls", mean, invstd, wimg, master);
  check_n(preds, torch::kInt32, "preds", a.B);
  const int rc = launch_mlp_predict_gen(
      X.data_ptr<float>(), a.B, (int)X.size(1), (int)inp, (int)hid, (int)cls,
      mean.data_ptr<float>(), invstd.data_ptr<float>(), bf16_ptr(wimg),
      master.data_ptr<float>(), preds.data_ptr<int>(), probs_ptr(probs, a.B, cls),
      current_stream());
  gen_launched(rc, "mlp_predict_gen", a, cls);
}

void adam_step_gen(torch::Tensor master, torch::Tensor bfmirror,
                   torch::Tensor grads, torch::Tensor m, torch::Tensor v,
                   torch::Tensor t_dev, int64_t inp, int64_t hid, int64_t cpad,
                   double lr, double beta1, double beta2, double eps,
                   c10::optional<torch::Tensor> wimg = c10::nullopt) {
  const GenGeometry g = gen_geometry(inp, hid, cpad);
  check_n(grads, torch::kFloat32, "grads", g.nparam());
  const AdamState st = adam_state(master, bfmirror, m, v, t_dev, g.nparam());
  launch_adam_step_gen(
      st.master, st.bfmirror, grads.data_ptr<float>(), st.m, st.v, st.t_dev,
      (int)g.nparam(), (int)inp, (int)hid, (int)cpad, (float)lr, (float)beta1,
      (float)beta2, (float)eps,
      opt_ptr<unsigned short>(wimg, torch::kBFloat16, "wimg", g.wimg_n()),
      current_stream());
}

// ---------------------------------------------------------------------------
// regression head of the generalized kernels (squared error, 1..32 targets)
// ---------------------------------------------------------------------------

bool mlp_step_reg_gen(torch::Tensor Xbf, torch::Tensor Yt, int64_t hid,
                      int64_t targets, int64_t rt, torch::Tensor wimg,
                      torch::Tensor master, torch::Tensor slabs, double invBtot) {
  const GenCall a =
      gen_step_args(Xbf, hid, targets, "targets", rt, wimg, master, slabs);
  // the kernel reads a row's targets as aligned 16-byte groups of a
  // [B][cpad] matrix (TabularMLPRegressor.stage_targets builds it)
  check(Yt, torch::kFloat32, "Yt");
  TORCH_CHECK(Yt.dim() == 2 && Yt.size(0) == a.B && Yt.size(1) == a.g.cpad,
              "Yt must be [", a.B, "][", a.g.cpad,
              "] standardized targets, zero-padded");
  check_aligned16(Yt, "Yt");
  const int rc = launch_mlp_step_reg_gen(
      bf16_ptr(Xbf), Yt.data_ptr<float>(), a.B, (int)a.g.inp, (int)hid,
      (int)targets, (int)rt, bf16_ptr(wimg), master.data_ptr<float>(),
      slabs.data_ptr<float>(), (int)slabs.size(1), (int)slabs.size(0),
      (float)invBtot, current_stream());
  return gen_launched(rc, "mlp_step_reg_gen", a, targets, rt);
}

void mlp_predict_reg_gen(torch::Tensor X, int64_t inp, int64_t hid,
                         int64_t targets, torch::Tensor mean,
                         torch::Tensor invstd, torch::Tensor wimg,
                         torch::Tensor master, torch::Tensor y_mean,
                         torch::Tensor y_scale, torch::Tensor out) {
  const GenCall a =
      gen_predict_args(X, inp, hid, targets, "targets", mean, invstd, wimg, master);
  check_n(y_mean, torch::kFloat32, "y_mean", targets, true);
  check_n(y_scale, torch::kFloat32, "y_scale", targets, true);
  check(out, torch::kFloat32, "out");
  TORCH_CHECK(out.dim() == 2 && out.size(0) >= a.B && out.size(1) >= targets &&
                  out.size(1) <= INT_MAX,
              "out must be [>= ", a.B, "][>= ", targets, "]");
  const int rc = launch_mlp_predict_reg_gen(
      X.data_ptr<float>(), a.B, (int)X.size(1), (int)inp, (int)hid, (int)targets,
      mean.data_ptr<float>(), invstd.data_ptr<float>(), bf16_ptr(wimg),
      master.data_ptr<float>(), y_mean.data_ptr<float>(),
      y_scale.data_ptr<float>(), out.data_ptr<float>(), (int)out.size(1),
      current_stream());
  gen_launched(rc, "mlp_predict_reg_gen", a, targets);
}

// ---------------------------------------------------------------------------
// device-side evaluation (tabular_eval.hip): forward-only metrics
// ---------------------------------------------------------------------------

namespace {

// An evaluation's arguments, either head: all but the per-row targets. rec
// is the record width of the head at this geometry.
GenCall gen_eval_args(const torch::Tensor& Xbf, int64_t hid, int64_t n_out,
                      const char* n_out_name, bool reg, const torch::Tensor& wimg,
                      const torch::Tensor& master, const torch::Tensor& part,
                      const torch::Tensor& hist, const torch::Tensor& slot) {
  const int B = (int)check_rows(Xbf, torch::kBFloat16, "Xbf");
  check_aligned16(Xbf, "Xbf");
  const GenGeometry g = gen_geometry_for(Xbf.size(1), hid, n_out, n_out_name);
  const int rt = eval_rows_per_wg((int)std::min<int64_t>(hid, INT_MAX), (int)g.cpad);
  TORCH_CHECK(rt > 0, "unsupported geometry: no evaluation kernel for hid=", hid,
              " cpad=", g.cpad);
  gen_weights(g, wimg, master);
  const int64_t rec = reg ? eval_rec_reg_n((int)g.cpad) : EVAL_REC_CLS_N;
  const int64_t n_wg = ((int64_t)B + rt - 1) / rt;
  check(part, torch::kFloat32, "part");
  TORCH_CHECK(part.dim() == 2 && part.size(0) >= n_wg && part.size(0) <= INT_MAX &&
                  part.size(1) >= rec && part.size(1) <= INT_MAX,
              "part must be [>= ", n_wg, "][>= ", rec, "], is ", part.sizes());
  check(hist, torch::kFloat32, "hist");
  TORCH_CHECK(hist.dim() == 2 && hist.size(0) >= 1 && hist.size(0) <= INT_MAX &&
                  hist.size(1) >= rec && hist.size(1) <= INT_MAX,
              "hist must be [cap >= 1][>= ", rec, "], is ", hist.sizes());
  check_n(slot, torch::kInt32, "slot", 1);
  return {g, B};
}

}  // namespace

void mlp_eval_gen(torch::Tensor Xbf, torch::Tensor y, int64_t hid, int64_t cls,
                  torch::Tensor wimg, torch::Tensor master, torch::Tensor part,
                  torch::Tensor hist, torch::Tensor slot) {
  const GenCall a =
      gen_eval_args(Xbf, hid, cls, "cls", false, wimg, master, part, hist, slot);
  check_n(y, torch::kInt32, "y", a.B, true);
  const int rc = launch_mlp_eval_gen(
      bf16_ptr(Xbf), y.data_ptr<int>(), a.B, (int)a.g.inp, (int)hid, (int)cls,
      bf16_ptr(wimg), master.data_ptr<float>(), part.data_ptr<float>(),
      (int)part.size(0), (int)part.size(1), hist.data_ptr<float>(),
      (int)hist.size(1), (int)hist.size(0), slot.data_ptr<int>(), current_stream());
  TORCH_CHECK(rc != -1, "mlp_eval_gen: fewer partial rows than workgroups");
  gen_launched(rc, "mlp_eval_gen", a, cls);
}

void mlp_eval_reg_gen(torch::Tensor Xbf, torch::Tensor Yt, int64_t hid,
                      int64_t targets, torch::Tensor wimg, torch::Tensor master,
                      torch::Tensor part, torch::Tensor hist, torch::Tensor slot) {
  const GenCall a = gen_eval_args(Xbf, hid, targets, "targets", true, wimg, master,
                                  part, hist, slot);
  check(Yt, torch::kFloat32, "Yt");
  TORCH_CHECK(Yt.dim() == 2 && Yt.size(0) == a.B && Yt.size(1) == a.g.cpad,
              "Yt must be [", a.B, "][", a.g.cpad,
              "] standardized targets, zero-padded");
  check_aligned16(Yt, "Yt");
  const int rc = launch_mlp_eval_reg_gen(
      bf16_ptr(Xbf), Yt.data_ptr<float>(), a.B, (int)a.g.inp, (int)hid,
      (int)targets, bf16_ptr(wimg), master.data_ptr<float>(),
      part.data_ptr<float>(), (int)part.size(0), (int)part.size(1),
      hist.data_ptr<float>(), (int)hist.size(1), (int)hist.size(0),
      slot.data_ptr<int>(), current_stream());
  TORCH_CHECK(rc != -1, "mlp_eval_reg_gen: fewer partial rows than workgroups");
  gen_launched(rc, "mlp_eval_reg_gen", a, targets);
}

// ---------------------------------------------------------------------------
// shuffled epochs (tabular_shuffle.hip): gather the staged rows by the keyed
// permutation of tabular_shuffle.h
// ---------------------------------------------------------------------------

namespace {

// the bytes a contiguous tensor occupies
struct Span {
  const char* name;
  uintptr_t lo, hi;
};

Span span_of(const torch::Tensor& t, const char* name) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(t.data_ptr());
  return {name, lo, lo + (uintptr_t)t.numel() * (uintptr_t)t.element_size()};
}

void check_disjoint(const Span& a, const Span& b) {
  TORCH_CHECK(a.hi <= b.lo || b.hi <= a.lo, a.name, " and ", b.name,
              " must not share storage");
}

// A shuffle's arguments, either head: all but the per-row targets. -> N
struct ShuffleCall {
  int64_t N;
  unsigned seed;
  int* perm_out;
};

ShuffleCall shuffle_args(const torch::Tensor& Xbf, const torch::Tensor& y,
                         const char* y_name, const torch::Tensor& Xs,
                         const torch::Tensor& ys, const char* ys_name,
                         const torch::Tensor& t_dev, int64_t seed,
                         const c10::optional<torch::Tensor>& perm_out) {
  const int64_t N = check_rows(Xbf, torch::kBFloat16, "Xbf");
  const int64_t inp = Xbf.size(1);
  TORCH_CHECK(inp % 32 == 0, "Xbf must be [N][inp], inp a multiple of 32, is ",
              Xbf.sizes());
  check_aligned16(Xbf, "Xbf");
  check(Xs, torch::kBFloat16, "Xs");
  TORCH_CHECK(Xs.dim() == 2 && Xs.size(0) >= N && Xs.size(1) == inp,
              "Xs must be [>= ", N, "][", inp, "], is ", Xs.sizes());
  check_aligned16(Xs, "Xs");
  check_n(t_dev, torch::kInt32, "t_dev", 1);
  TORCH_CHECK(seed >= 0 && seed <= (int64_t)UINT32_MAX,
              "seed must be in [0, 2^32), is ", seed);
  int* perm = opt_ptr<int>(perm_out, torch::kInt32, "perm_out", N);
  // the kernel reads a source row while another wave writes a destination
  // row: no destination may alias a source or another destination
  std::vector<Span> src{span_of(Xbf, "Xbf"), span_of(y, y_name),
                        span_of(t_dev, "t_dev")};
  std::vector<Span> dst{span_of(Xs, "Xs"), span_of(ys, ys_name)};
  if (perm_out.has_value()) dst.push_back(span_of(*perm_out, "perm_out"));
  for (size_t i = 0; i < dst.size(); ++i) {
    for (const Span& s : src) check_disjoint(s, dst[i]);
    for (size_t j = i + 1; j < dst.size(); ++j) check_disjoint(dst[i], dst[j]);
  }
  return {N, (unsigned)seed, perm};
}

}  // namespace

void shuffle_rows(torch::Tensor Xbf, torch::Tensor y, torch::Tensor Xs,
                  torch::Tensor ys, torch::Tensor t_dev, int64_t seed,
                  c10::optional<torch::Tensor> perm_out = c10::nullopt) {
  check_rows(Xbf, torch::kBFloat16, "Xbf");   // N, before the targets' counts
  check_n(y, torch::kInt32, "y", Xbf.size(0), true);
  check_n(ys, torch::kInt32, "ys", Xbf.size(0));
  const ShuffleCall a = shuffle_args(Xbf, y, "y", Xs, ys, "ys", t_dev, seed, perm_out);
  const int rc = launch_shuffle_rows(
      bf16_ptr(Xbf), y.data_ptr<int>(), bf16_mut_ptr(Xs), ys.data_ptr<int>(),
      a.perm_out, t_dev.data_ptr<int>(), a.seed, a.N, (int)Xbf.size(1),
      current_stream());
  TORCH_CHECK(rc == 0, "shuffle_rows: arguments outside the kernel's range");
}

void shuffle_rows_reg(torch::Tensor Xbf, torch::Tensor Yt, torch::Tensor Xs,
                      torch::Tensor Yts, torch::Tensor t_dev, int64_t seed,
                      c10::optional<torch::Tensor> perm_out = c10::nullopt) {
  const int64_t N = check_rows(Xbf, torch::kBFloat16, "Xbf");
  check(Yt, torch::kFloat32, "Yt");
  TORCH_CHECK(Yt.dim() == 2 && Yt.size(0) == N &&
                  (Yt.size(1) == 16 || Yt.size(1) == 32),
              "Yt must be [", N, "][cpad = 16 or 32] staged targets, is ", Yt.sizes());
  check_aligned16(Yt, "Yt");
  check(Yts, torch::kFloat32, "Yts");
  TORCH_CHECK(Yts.dim() == 2 && Yts.size(0) >= N && Yts.size(1) == Yt.size(1),
              "Yts must be [>= ", N, "][", Yt.size(1), "], is ", Yts.sizes());
  check_aligned16(Yts, "Yts");
  const ShuffleCall a =
      shuffle_args(Xbf, Yt, "Yt", Xs, Yts, "Yts", t_dev, seed, perm_out);
  const int rc = launch_shuffle_rows_reg(
      bf16_ptr(Xbf), Yt.data_ptr<float>(), bf16_mut_ptr(Xs), Yts.data_ptr<float>(),
      a.perm_out, t_dev.data_ptr<int>(), a.seed, a.N, (int)Xbf.size(1),
      (int)Yt.size(1), current_stream());
  TORCH_CHECK(rc == 0, "shuffle_rows_reg: arguments outside the kernel's range");
}

// The permutation as the HOST compiles tabular_shuffle.h: src[i] for every
// i < N, an int32 CPU tensor. No device involved; tests hold it equal to
// reference.shuffle_perm and to the kernel's perm_out.
torch::Tensor shuffle_perm_host(int64_t N, int64_t seed, int64_t t) {
  TORCH_CHECK(N >= 1 && N <= INT_MAX, "N must be 1..INT_MAX, is ", N);
  TORCH_CHECK(seed >= 0 && seed <= (int64_t)UINT32_MAX,
              "seed must be in [0, 2^32), is ", seed);
  TORCH_CHECK(t >= INT_MIN && t <= INT_MAX, "t must fit an int32, is ", t);
  torch::Tensor out = torch::empty({N}, torch::dtype(torch::kInt32));
  const ShufflePerm perm((unsigned)N, (unsigned)seed, (unsigned)(int)t);
  int* p = out.data_ptr<int>();
  for (int64_t i = 0; i < N; ++i) p[i] = (int)perm((unsigned)i);
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("shuffle_rows", &shuffle_rows,
        "Xs[i] = Xbf[src], ys[i] = y[src] (int32 labels), src = P(i; N, seed, "
        "t_dev[0]) the keyed permutation; perm_out[i] = src when given",
        py::arg("Xbf"), py::arg("y"), py::arg("Xs"), py::arg("ys"),
        py::arg("t_dev"), py::arg("seed"), py::arg("perm_out") = c10::nullopt);
  m.def("shuffle_rows_reg", &shuffle_rows_reg,
        "shuffle_rows over staged regression targets Yt [N][cpad] fp32",
        py::arg("Xbf"), py::arg("Yt"), py::arg("Xs"), py::arg("Yts"),
        py::arg("t_dev"), py::arg("seed"), py::arg("perm_out") = c10::nullopt);
  m.def("shuffle_perm_host", &shuffle_perm_host,
        "the keyed permutation of [0, N) evaluated on the host, int32 [N]",
        py::arg("N"), py::arg("seed"), py::arg("t"));
  // evaluation record layout (tabular_launch.h EVAL_REC_*), fp32 entries
  m.attr("EVAL_REC_LOSS") = EVAL_REC_LOSS;
  m.attr("EVAL_REC_CORRECT") = EVAL_REC_CORRECT;      // int32 bits
  m.attr("EVAL_REC_CLS_N") = EVAL_REC_CLS_N;          // classifier record width
  m.attr("EVAL_REC_FIRST_MSE") = EVAL_REC_FIRST_MSE;  // regression: + column
  m.def("eval_rec_reg_n", [](int64_t cpad) { return eval_rec_reg_n((int)cpad); },
        "regression record width at a padded target count", py::arg("cpad"));
  m.def("eval_rows_per_wg",
        [](int64_t hid, int64_t cpad) { return eval_rows_per_wg((int)hid, (int)cpad); },
        "rows per workgroup of the evaluation kernel (0: none compiled)",
        py::arg("hid"), py::arg("cpad"));
  m.def("mlp_eval_gen", &mlp_eval_gen,
        "forward-only classifier metrics: loss sum and correct count per "
        "workgroup into part, then one record (mean loss, correct count) "
        "into hist[min(slot, cap-1)]; slot advances",
        py::arg("Xbf"), py::arg("y"), py::arg("hid"), py::arg("cls"),
        py::arg("wimg"), py::arg("master"), py::arg("part"), py::arg("hist"),
        py::arg("slot"));
  m.def("mlp_eval_reg_gen", &mlp_eval_reg_gen,
        "forward-only regression metrics: loss and per-column squared error "
        "per workgroup into part, then one record (mean loss, column MSE in "
        "standardized units) into hist[min(slot, cap-1)]; slot advances",
        py::arg("Xbf"), py::arg("Yt"), py::arg("hid"), py::arg("targets"),
        py::arg("wimg"), py::arg("master"), py::arg("part"), py::arg("hist"),
        py::arg("slot"));
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
