"""The tabular HIP kernels against the plain fp64 oracle (tests/oracle64.py).

Every mlp_step_gen / mlp_predict_gen instantiation is launched directly
(rt= picks the rows-per-workgroup variant TabularMLP would only choose at
large batches), with NON-ZERO biases, at the batch sizes around a
workgroup's row count. Bounds are either derived (loss, argmax slack,
summation, moments, standardizer) or measured IN THE SAME TEST on the
bf16-mirroring reference (ops/reference.py) against the oracle, never on
the kernel under test. The case list lives in oracle64.py, where
tests/test_oracle64_cpu.py checks its conditions on the CPU.

Run with -s to see every measured ratio (docs/kernels.md, "Numerics vs
fp64", records the largest per kernel)."""

import numpy as np
import pytest
import torch

import oracle64 as o64
from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import Geometry

pytestmark = pytest.mark.gpu

F64 = torch.float64
LR, EPS = 1e-3, 1e-8


def f32(x: float) -> float:
    """x as the kernels receive it (the bindings cast scalars to float)"""
    return float(np.float32(x))


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def gpu_clf(case, dev):
    """A TabularMLP carrying the case's weights AND non-zero biases"""
    from unionml_amd.ops.tabular import TabularMLP

    inf, hid, cls = case.shape
    clf = TabularMLP(in_features=inf, hidden=hid, classes=cls, device=dev, seed=case.seed)
    clf.master.copy_(case.master.to(dev))
    clf.bfmirror.copy_(clf.master.bfloat16())
    clf._build_wimg()
    assert torch.equal(clf.bfmirror.cpu(), case.bfmirror)
    return clf


# ---------------------------------------------------------------------------
# step kernels
# ---------------------------------------------------------------------------


def check_step(name, case, grads_k):
    """Per-case assertions on a step kernel's flat grads (+loss): exact-zero
    pads, per-segment error within twice the reference's own (floor one
    bf16 ulp), loss within its derived bound."""
    g = case.g
    grads_k = grads_k.cpu()
    assert torch.isfinite(grads_k).all(), "unwritten or non-finite gradient entries"
    assert (grads_k[: g.nparam][o64.pad_mask(g)] == 0).all(), "padded parameter leaked gradient"

    grads64, _, H, _ = o64.step64(g, case.Xbf, case.y, case.W1bf, case.W2bf,
                                  case.master, case.invB)
    err_r = o64.segment_errors(g, o64.reference_step(case), grads64)
    err_k = o64.segment_errors(g, grads_k, grads64)
    failures = []
    for s in o64.SEGMENTS:
        (e_k, emax_k), (e_r, emax_r) = err_k[s], err_r[s]
        print(f"RATIO step {name} {s}: e_k={e_k:.3e} e_r={e_r:.3e} e_k/e_r={e_k / e_r:.3f} "
              f"emax_k={emax_k:.3e} emax_r={emax_r:.3e} emax_k/emax_r={emax_k / emax_r:.3f}")
        if not e_k <= max(2 * e_r, o64.BF16_ULP):
            failures.append(f"{s}: e_k={e_k:.3e} > max(2*{e_r:.3e}, 2^-8)")
        if not emax_k <= max(2 * emax_r, o64.BF16_ULP):
            failures.append(f"{s}: emax_k={emax_k:.3e} > max(2*{emax_r:.3e}, 2^-8)")
    assert not failures, f"{name}: " + "; ".join(failures)

    bound = o64.loss_bound(H, case.W2bf, g, case.invB)
    dloss = abs(float(grads_k[g.nparam].double() - grads64[g.nparam]))
    print(f"RATIO loss {name}: |dloss|={dloss:.3e} bound={bound:.3e}")
    assert dloss <= bound, f"{name}: loss off by {dloss:.3e} > {bound:.3e}"


def run_gen_step(ext, dev, case, rt):
    """mlp_step_gen at an explicit rows-per-workgroup, then the reduce-only
    slab sum. Slabs start as NaN: every entry the reduction reads must have
    been stored by the step kernel in this launch."""
    clf = gpu_clf(case, dev)
    g = clf.g
    n_wg = (case.B + rt - 1) // rt
    slabs = torch.full((n_wg, g.slab_stride), float("nan"), device=dev)
    counter = torch.zeros(1, dtype=torch.uint32, device=dev)
    grads = torch.full((g.nparam + 1,), float("nan"), device=dev)
    loss_out = torch.zeros(1, device=dev)
    master0 = clf.master.clone()
    ok = ext.mlp_step_gen(case.Xbf.to(dev), case.y.to(dev), g.hid, g.classes, rt,
                          clf.wimg, clf.master, slabs, case.invB)
    assert ok
    ext.reduce_adam_gen(slabs, n_wg, g.inp, g.hid, g.cpad, clf.master, clf.bfmirror,
                        clf.m, clf.v, clf.t_dev, counter, loss_out, LR, 0.9, 0.999, EPS,
                        wimg=clf.wimg, grads_out=grads)
    torch.cuda.synchronize()
    assert int(clf.t_dev.item()) == 0 and int(counter.item()) == 0
    assert torch.equal(clf.master, master0)
    return grads


GEN_STEP = o64.gen_step_cases()


@pytest.mark.parametrize("cid,inst,shape,B,seed", GEN_STEP, ids=[c[0] for c in GEN_STEP])
def test_gen_step_vs_oracle(ext, dev, cid, inst, shape, B, seed):
    """Every step instantiation <HID,RT,CPAD>, launched directly."""
    case = o64.make_case(shape, B, seed)
    o64.check_instantiation(inst, shape)
    check_step(cid, case, run_gen_step(ext, dev, case, inst[1]))


SPEC_STEP = o64.spec_step_cases()


@pytest.mark.parametrize("kernel", ["mlp_step", "mlp_step_fused"])
@pytest.mark.parametrize("cid,shape,B,seed", SPEC_STEP, ids=[c[0] for c in SPEC_STEP])
def test_spec_step_vs_oracle(ext, dev, kernel, cid, shape, B, seed):
    """The specialized 64x32x10 kernels: the atomic-accumulating mlp_step
    and the fused step in reduce-only (grads_out=) mode."""
    case = o64.make_case(shape, B, seed)
    clf = gpu_clf(case, dev)
    g = clf.g
    Xbf, y = case.Xbf.to(dev), case.y.to(dev)
    if kernel == "mlp_step":
        grads = torch.zeros(g.nparam + 1, device=dev)
        ext.mlp_step(Xbf, y, clf.W1bf, clf.W2bf, clf.master, grads, case.invB)
    else:
        grads = torch.full((g.nparam + 1,), float("nan"), device=dev)
        clf._ensure_slabs((B + o64.SPEC_RT - 1) // o64.SPEC_RT)
        loss_out = torch.zeros(1, device=dev)
        ok = ext.mlp_step_fused(
            Xbf, y, clf.W1bf, clf.W2bf, clf.master, clf.bfmirror, clf.m, clf.v,
            clf.t_dev, clf.slabs, clf.counter, loss_out, case.invB, LR, 0.9, 0.999, EPS,
            grads_out=grads, wimg=clf.wimg,
        )
        assert ok
    torch.cuda.synchronize()
    assert int(clf.t_dev.item()) == 0
    check_step(f"{kernel}-{cid}", case, grads)


# ---------------------------------------------------------------------------
# predict kernels
# ---------------------------------------------------------------------------

SENTINEL = -7.0
GUARD_ROWS = 3


def run_predict(ext, dev, clf, X):
    """preds/probs with GUARD_ROWS sentinel rows behind [B][cls]"""
    g = clf.g
    B = X.shape[0]
    preds = torch.full((B + GUARD_ROWS,), int(SENTINEL), dtype=torch.int32, device=dev)
    probs = torch.full((B + GUARD_ROWS, g.classes), SENTINEL, device=dev)
    if g.is_specialized:
        ext.mlp_predict(X, clf.mean, clf.invstd, clf.W1bf, clf.W2bf, clf.master, preds, probs)
    else:
        ext.mlp_predict_gen(X, g.inp, g.hid, g.classes, clf.mean, clf.invstd, clf.wimg,
                            clf.master, preds, probs)
    torch.cuda.synchronize()
    preds, probs = preds.cpu(), probs.cpu()
    assert (preds[B:] == int(SENTINEL)).all() and (probs[B:] == SENTINEL).all(), \
        "wrote past [B][cls]"
    return preds[:B], probs[:B]


PREDICT = o64.predict_cases()


@pytest.mark.parametrize("cid,inst,shape,B,seed", PREDICT, ids=[c[0] for c in PREDICT])
def test_predict_vs_oracle(ext, dev, cid, inst, shape, B, seed):
    """Every predict instantiation and the specialized predict kernel."""
    case = o64.make_case(shape, B, seed)
    if inst is not None:
        o64.check_instantiation(inst, shape)
    clf = gpu_clf(case, dev)
    g = clf.g
    ext.standardize_fit(case.Xfit.to(dev), clf.mean, clf.invstd, 1e-5)
    preds_k, p_k = run_predict(ext, dev, clf, case.X.to(dev))

    mean, invstd = clf.mean.cpu(), clf.invstd.cpu()
    logits, p64, H = o64.predict64(g, case.X, mean, invstd, case.W1bf, case.W2bf, case.master)
    _, p_r = ref.mlp_predict_g(g, case.X, mean, invstd, case.W1bf, case.W2bf, case.master,
                               return_probs=True)
    d_k = float((p_k.double() - p64).abs().max())
    d_r = float((p_r.double() - p64).abs().max())
    print(f"RATIO predict {cid}: dp_k={d_k:.3e} dp_r={d_r:.3e} dp_k/dp_r={d_k / d_r:.3f}")
    assert d_k <= max(2 * d_r, 1e-6), f"{cid}: dp_k={d_k:.3e} > max(2*{d_r:.3e}, 1e-6)"
    assert float((p_k.double().sum(dim=1) - 1).abs().max()) <= 1e-5

    clear = o64.clear_rows(logits, H, case.W2bf, g)
    excluded = 1.0 - float(clear.double().mean())
    assert excluded <= o64.MAX_EXCLUDED, f"{cid}: margin rule excludes {excluded:.3f}"
    want = logits.argmax(dim=1)
    bad = (preds_k.long() != want) & clear
    assert not bad.any(), f"{cid}: {int(bad.sum())} clear-margin argmax mismatches"


TIE_SHAPES = [(64, 32, 10), (70, 50, 7), (100, 64, 26)]


@pytest.mark.parametrize("shape", TIE_SHAPES, ids=o64.shape_id)
def test_predict_ties_pick_lowest_class(ext, dev, shape):
    """head_argmax promises the lowest class on a tie. All weights and b2
    zero: every logit ties, prediction 0, probability 1/cls. On the
    26-class head, b2 raised equally on classes 3 and 19 (one in each MFMA
    class tile): prediction 3."""
    rt = 128
    case = o64.make_case(shape, rt + 1, seed=2)
    seg = o64.real_segments(case.g, case.master)
    for s in ("W1", "W2", "b2"):
        seg[s].zero_()                      # b1 stays non-zero: H != 0, logits still 0
    case.bfmirror = case.master.bfloat16()
    clf = gpu_clf(case, dev)
    cls = clf.g.classes
    ext.standardize_fit(case.Xfit.to(dev), clf.mean, clf.invstd, 1e-5)
    preds, probs = run_predict(ext, dev, clf, case.X.to(dev))
    assert (preds == 0).all()
    assert float((probs.double() - 1.0 / cls).abs().max()) <= 1e-6

    if cls == 26:
        seg["b2"][3] = 1.5
        seg["b2"][19] = 1.5
        case.bfmirror = case.master.bfloat16()
        clf = gpu_clf(case, dev)
        ext.standardize_fit(case.Xfit.to(dev), clf.mean, clf.invstd, 1e-5)
        preds, probs = run_predict(ext, dev, clf, case.X.to(dev))
        assert (preds == 3).all()
        assert torch.equal(probs[:, 3], probs[:, 19])


# ---------------------------------------------------------------------------
# the slab reduction alone
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n_wg", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("shape", [(1, 1, 2), (784, 256, 10)], ids=o64.shape_id)
def test_reduce_gen_sum_vs_fp64(ext, dev, shape, n_wg):
    """reduce_adam_gen with grads_out=: the unrolled-by-4 slab loop and its
    remainder, on a tiny geometry and on one whose nparam (> 512*256) wraps
    the grid-stride loop. Values over 8 decades, mixed signs; the error is
    bounded elementwise by gamma_n * sum|x| (fp32 summation of n terms)."""
    g = Geometry(*shape)
    if shape[0] == 784:
        assert g.nparam > 512 * 256
    gen = torch.Generator().manual_seed(n_wg)
    mag = 10.0 ** (torch.rand(n_wg, g.slab_stride, generator=gen) * 8.0 - 4.0)
    sign = torch.where(torch.rand(n_wg, g.slab_stride, generator=gen) < 0.5, -1.0, 1.0)
    x = (mag * sign).float()
    slabs = x.to(dev)
    z = lambda: torch.zeros(g.nparam, device=dev)  # noqa: E731
    master, m, v = z() + 0.25, z() + 0.5, z() + 0.75
    bfmirror = master.bfloat16()
    t_dev = torch.full((1,), 5, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.uint32, device=dev)
    loss_out = torch.full((1,), SENTINEL, device=dev)
    grads = torch.full((g.nparam + 1 + GUARD_ROWS,), SENTINEL, device=dev)
    for _ in range(2):   # twice: the done-counter must be back at 0 each time
        ext.reduce_adam_gen(slabs, n_wg, g.inp, g.hid, g.cpad, master, bfmirror, m, v,
                            t_dev, counter, loss_out, LR, 0.9, 0.999, EPS, grads_out=grads)
        torch.cuda.synchronize()
        assert int(counter.item()) == 0
    assert int(t_dev.item()) == 5
    assert (master == 0.25).all() and (m == 0.5).all() and (v == 0.75).all()
    grads = grads.cpu()
    assert (grads[g.nparam + 1:] == SENTINEL).all()
    xd = x.double()[:, : g.nparam + 1]
    err = (grads[: g.nparam + 1].double() - xd.sum(dim=0)).abs()
    bound = o64.gamma(n_wg) * xd.abs().sum(dim=0)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"RATIO reduce {o64.shape_id(shape)} n_wg={n_wg}: max err/bound={worst:.3f}")
    assert (err <= bound).all()


# ---------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------

ADAM_STEPS = 12
# rho_k <= ADAM_RHO_MARGIN * rho_ref, rho = max_i |delta - delta_64| / lr
ADAM_RHO_MARGIN = 4.0
# The one bound NOT taken from the reference. adam_bias_corr computes
# beta^t with the fp32 fast pow; at beta2 = 0.999 the error of beta2^t
# (about half an fp32 ulp of 1) is divided by 1 - beta2^t ~ t * 1e-3, so the
# step is off by a few 1e-6 of its size at t = 2..6, where the 4 * rho_ref
# bound (~1e-6) fails; from t = 7 on, and with betas (0.8, 0.95), it holds.
# Computing the power exactly (fp64 binary exponentiation) brought every
# step within 1.5 * rho_ref but cost a measurable 0.06 us on the 9.03 us
# fused benchmark step, so the kernel stays as it is and these steps are
# held to the measured rho_k (worst of the three kernels) with a 2x margin.
# docs/kernels.md, "Numerics vs fp64", has the full table.
ADAM_POW_RHO_MEASURED = {2: 3.70e-6, 3: 3.21e-6, 4: 2.99e-6, 5: 2.33e-6, 6: 1.62e-6}


def adam_rho_bound(betas, t, rho_ref):
    bound = ADAM_RHO_MARGIN * rho_ref
    if betas == (0.9, 0.999):
        bound = max(bound, 2.0 * ADAM_POW_RHO_MEASURED.get(t, 0.0))
    return bound


def rho(p_new, p_old, d64):
    return float(((p_new.double() - p_old.double()) - d64).abs().max()) / f32(LR)


class AdamRun:
    """Drives one of the three Adam entry points over a gradient sequence."""

    def __init__(self, ext, dev, kernel, shape):
        from unionml_amd.ops.tabular import TabularMLP

        self.ext, self.dev, self.kernel = ext, dev, kernel
        self.clf = TabularMLP(*shape, device=dev, seed=0)
        self.clf.master.zero_()
        self.clf.bfmirror.zero_()
        self.clf._build_wimg()
        g = self.g = self.clf.g
        self.grads = torch.zeros(g.nparam + 1, device=dev)
        if kernel == "reduce_adam_gen":
            self.slabs = torch.zeros(1, g.slab_stride, device=dev)
            self.counter = torch.zeros(1, dtype=torch.uint32, device=dev)
            self.loss_out = torch.zeros(1, device=dev)

    def step(self, gr, loss, betas):
        c, g, ext = self.clf, self.g, self.ext
        state = (c.master, c.bfmirror)
        if self.kernel == "adam_step":
            self.grads[: g.nparam].copy_(gr)
            ext.adam_step(*state, self.grads, c.m, c.v, c.t_dev, LR, *betas, EPS, wimg=c.wimg)
        elif self.kernel == "adam_step_gen":
            self.grads[: g.nparam].copy_(gr)
            ext.adam_step_gen(*state, self.grads, c.m, c.v, c.t_dev, g.inp, g.hid, g.cpad,
                              LR, *betas, EPS, wimg=c.wimg)
        else:
            self.slabs[0, : g.nparam].copy_(gr)
            self.slabs[0, g.nparam] = loss
            ext.reduce_adam_gen(self.slabs, 1, g.inp, g.hid, g.cpad, *state, c.m, c.v,
                                c.t_dev, self.counter, self.loss_out, LR, *betas, EPS,
                                wimg=c.wimg)
        torch.cuda.synchronize()
        if self.kernel == "reduce_adam_gen":
            assert int(self.counter.item()) == 0
            assert float(self.loss_out.item()) == f32(loss)


ADAM_KERNELS = o64.ADAM_KERNELS


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)], ids=["default", "b0.8-0.95"])
@pytest.mark.parametrize("kernel,shape", ADAM_KERNELS, ids=[k for k, _ in ADAM_KERNELS])
def test_adam_vs_oracle(ext, dev, kernel, shape, betas):
    """Twelve steps from zero state with a FRESH gradient each step
    (1e-6..10, some exact zeros), so the betas matter; every state tensor
    checked after every step. The oracle and the fp32 torch reference get
    the scalars as the kernel does, rounded to fp32."""
    run = AdamRun(ext, dev, kernel, shape)
    clf, g = run.clf, run.g
    n = g.nparam
    grads, always_zero = o64.adam_gradients(n, ADAM_STEPS, seed=17)
    b1, b2 = f32(betas[0]), f32(betas[1])
    lr, eps = f32(LR), f32(EPS)
    p64, m64, v64 = o64.adam64(torch.zeros(n), grads, lr, b1, b2, eps)
    env = o64.moment_envelopes(grads, b1, b2)

    p_r, mir_r = torch.zeros(n), torch.zeros(n, dtype=torch.bfloat16)
    m_r, v_r = torch.zeros(n), torch.zeros(n)
    prev_k, prev_64 = torch.zeros(n), torch.zeros(n, dtype=F64)
    failures = []
    for t in range(1, ADAM_STEPS + 1):
        gr = grads[t - 1]
        run.step(gr.to(dev), 0.125 * t, betas)
        prev_r = p_r.clone()
        ref.adam_step_g(g, p_r, mir_r, gr, m_r, v_r, t, lr, b1, b2, eps)

        assert int(clf.t_dev.item()) == t
        p_k, m_k, v_k = clf.master.cpu(), clf.m.cpu(), clf.v.cpu()
        # moments: 4 t 2^-24 of the same recurrence on |g| (resp. g^2)
        tol = 4 * t * 2.0 ** -24
        assert ((m_k.double() - m64[t - 1]).abs() <= tol * env[t - 1][0]).all(), f"m at t={t}"
        assert ((v_k.double() - v64[t - 1]).abs() <= tol * env[t - 1][1]).all(), f"v at t={t}"
        for name, x in (("master", p_k), ("m", m_k), ("v", v_k)):
            assert (x[always_zero] == 0).all(), f"{name} moved without a gradient at t={t}"
        assert torch.equal(clf.bfmirror.cpu(), p_k.bfloat16()), f"bfmirror at t={t}"
        incremental = clf.wimg.clone()
        clf._build_wimg()
        assert torch.equal(incremental, clf.wimg), f"wimg at t={t}"

        d64 = p64[t - 1] - prev_64
        rho_k, rho_r = rho(p_k, prev_k, d64), rho(p_r, prev_r, d64)
        print(f"RATIO adam {kernel} betas={betas} t={t}: rho_k={rho_k:.3e} "
              f"rho_ref={rho_r:.3e} rho_k/rho_ref={rho_k / rho_r:.2f}")
        bound = adam_rho_bound(betas, t, rho_r)
        if not rho_k <= bound:
            failures.append(f"t={t}: rho_k={rho_k:.3e} > {bound:.3e} (rho_ref={rho_r:.3e})")
        prev_k, prev_64 = p_k, p64[t - 1]
    assert not failures, f"{kernel} {betas}: " + "; ".join(failures)


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)], ids=["default", "b0.8-0.95"])
@pytest.mark.parametrize("kernel,shape", ADAM_KERNELS, ids=[k for k, _ in ADAM_KERNELS])
def test_adam_moments_are_the_written_formula(ext, dev, kernel, shape, betas):
    """m and v bit for bit against the formulas adam_update (tabular_common.h)
    states, m' = fma(1-b1, g, rn(b1 m)) and v' = fma(g, rn((1-b2) g), rn(b2 v)),
    evaluated on the host by oracle64.adam_moments32 from the state the
    kernel itself left after the previous step. Every Adam entry point must
    compile to this one arithmetic (two of them did not; docs/kernels.md,
    "Determinism"). Exempt are the entries whose host fma may be
    double-rounded, at most MAX_MIDPOINT_SHARE of a tensor (on these seeds:
    none, tests/test_oracle64_cpu.py). master is not held bit for bit:
    v_rcp_f32 and v_sqrt_f32 are approximate, test_adam_vs_oracle bounds it."""
    run = AdamRun(ext, dev, kernel, shape)
    clf, n = run.clf, run.g.nparam
    grads, _ = o64.adam_gradients(n, o64.ADAM_MOMENT_STEPS, seed=o64.ADAM_GRAD_SEED)
    b1, b2 = f32(betas[0]), f32(betas[1])
    m_prev, v_prev = torch.zeros(n), torch.zeros(n)
    exempted = 0
    for t, gr in enumerate(grads, start=1):
        run.step(gr.to(dev), 0.125 * t, betas)
        assert int(clf.t_dev.item()) == t
        m_k, v_k = clf.m.cpu(), clf.v.cpu()
        m_w, v_w, ex_m, ex_v = o64.adam_moments32(m_prev, v_prev, gr, b1, b2)
        for name, got, want, ex in (("m", m_k, m_w, ex_m), ("v", v_k, v_w, ex_v)):
            share = float(ex.double().mean())
            assert share <= o64.MAX_MIDPOINT_SHARE, f"{name} t={t}: {share:.2e} exempt"
            exempted += int(ex.sum())
            bad = (got != want) & ~ex
            assert not bad.any(), (
                f"{kernel} {name} t={t}: {int(bad.sum())} of {n} entries differ from the "
                f"formula, first at {int(bad.nonzero()[0])}")
        m_prev, v_prev = m_k, v_k
    print(f"RATIO adam-moments {kernel} betas={betas}: {exempted} midpoint entries exempted "
          f"of {2 * n * len(grads)}")


# ---------------------------------------------------------------------------
# standardizer
# ---------------------------------------------------------------------------

STD_EPS = 1e-5
STD_NS = (1, 2, 255, 257, 3000)


def std_matrix(N, D, kind0, seed):
    """Columns cycle through: scale 1e-3, scale 1e3, mean/std = 1e4, and
    the constant 3.25, starting at kind ``kind0``."""
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=gen)
    kinds = (torch.arange(D) + kind0) % 4
    X[:, kinds == 0] *= 1e-3
    X[:, kinds == 1] *= 1e3
    X[:, kinds == 2] += 1e4
    X[:, kinds == 3] = 3.25
    return X, kinds


@pytest.mark.parametrize("D", [1, 4, 64, 256, 3, 100, 257, 784])
def test_standardize_vs_oracle(ext, dev, D):
    """standardize_fit on the fast path (D divides 256) and on the
    column-per-workgroup path, against the TWO-pass fp64 statistics, then
    standardize_apply bit for bit against torch's fp32 arithmetic, into a
    padded output whose pad columns must stay untouched."""
    eps = f32(STD_EPS)
    flat_invstd = np.float32(1.0 / np.sqrt(np.float64(eps)))
    # a matrix narrower than the four column kinds runs once per window
    kind0s = {1: (0, 1, 2, 3), 3: (0, 1)}.get(D, (0,))
    for N in STD_NS:
        for kind0 in kind0s:
            X, kinds = std_matrix(N, D, kind0, seed=D * 7 + N)
            Xd = X.to(dev)
            mean = torch.full((D,), SENTINEL, device=dev)
            invstd = torch.full((D,), SENTINEL, device=dev)
            ext.standardize_fit(Xd, mean, invstd, STD_EPS)
            pad = 5
            out = torch.full((N, D + pad), SENTINEL, dtype=torch.bfloat16, device=dev)
            ext.standardize_apply(Xd, mean, invstd, out)
            torch.cuda.synchronize()
            mean, invstd, out = mean.cpu(), invstd.cpu(), out.cpu()

            mean64, invstd64, var64 = o64.standardize64(X, eps)
            tag = f"D={D} N={N} kind0={kind0}"
            assert ((mean.double() - mean64).abs() <= 2.0 ** -23 * mean64.abs()).all(), tag
            live = var64 > 0
            rel = (invstd.double() - invstd64).abs() / invstd64
            bound = 2.0 ** -23 + N * 2.0 ** -52 * (1.0 + mean64 ** 2 / var64.clamp_min(1e-300))
            assert (rel[live] <= bound[live]).all(), tag
            # zero variance: the constant column, every column at N = 1 (and
            # any column whose few values happen to coincide): the one-pass
            # sums cancel exactly, so invstd is exactly 1/sqrt(eps)
            flat = ~live
            assert flat[(kinds == 3) | (N == 1)].all(), tag
            assert (invstd[flat].numpy() == flat_invstd).all(), tag
            if N == 1:
                assert torch.equal(mean, X[0]), tag
            assert (mean[kinds == 3] == 3.25).all(), tag

            want = ((X - mean) * invstd).bfloat16()
            assert torch.equal(out[:, :D], want), tag
            assert (out[:, D:].float() == SENTINEL).all(), f"{tag}: pad columns touched"


# ---------------------------------------------------------------------------
# smallest geometry end to end
# ---------------------------------------------------------------------------


def sign_step(gr, eps):
    """First bias-corrected Adam step from zero moments, per unit lr"""
    return -gr / (gr.abs() + eps)


@pytest.mark.parametrize("shape,B", o64.E2E_CASES,
                         ids=[f"{o64.shape_id(s)}-B{B}" for s, B in o64.E2E_CASES])
def test_one_fused_step_end_to_end(ext, dev, shape, B):
    """One _fused_adam_step (step kernel + reduce + Adam) at the smallest
    geometry and at the most padded one: master must land where
    adam64(step64()) lands. Tolerance per parameter: the first Adam step is
    -lr g/(|g|+eps), monotone in g, so a gradient within the step test's
    bound delta_s of the oracle's moves it at most to the image of
    g -+ delta_s; on top of that the Adam step-error allowance
    ADAM_RHO_MARGIN * rho_ref (both times lr). Pads stay exactly 0."""
    case = o64.make_case(shape, B, o64.case_seed(shape, B))
    clf = gpu_clf(case, dev)
    g = clf.g
    rpw = clf._rows_per_wg(B)
    clf._ensure_slabs((B + rpw - 1) // rpw)
    loss_out = torch.zeros(1, device=dev)
    clf._fused_adam_step(case.Xbf.to(dev), case.y.to(dev), case.invB, LR, loss_out)
    torch.cuda.synchronize()
    assert int(clf.t_dev.item()) == 1

    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    lr, eps = f32(LR), f32(ADAM_EPS)
    b1, b2 = f32(ADAM_BETA1), f32(ADAM_BETA2)
    grads64, _, H, _ = o64.step64(g, case.Xbf, case.y, case.W1bf, case.W2bf,
                                  case.master, case.invB)
    g64 = grads64[: g.nparam]
    p64 = o64.adam64(case.master, [g64], lr, b1, b2, eps)[0][0]

    # gradient slack per segment, from the reference's own error
    err_r = o64.segment_errors(g, o64.reference_step(case), grads64)
    delta = torch.zeros(g.nparam, dtype=F64)
    dseg, oseg = o64.real_segments(g, delta), o64.real_segments(g, g64)
    for s in o64.SEGMENTS:
        dseg[s].fill_(max(2 * err_r[s][1], o64.BF16_ULP) * float(oseg[s].abs().max()))
    move = torch.maximum((sign_step(g64 + delta, eps) - sign_step(g64, eps)).abs(),
                         (sign_step(g64 - delta, eps) - sign_step(g64, eps)).abs())
    # Adam allowance: the fp32 torch reference on the oracle's gradient
    p_r, mir_r = case.master.clone(), case.bfmirror.clone()
    m_r, v_r = torch.zeros(g.nparam), torch.zeros(g.nparam)
    ref.adam_step_g(g, p_r, mir_r, g64.float(), m_r, v_r, 1, lr, b1, b2, eps)
    rho_r = rho(p_r, case.master, p64 - case.master.double())

    p_k = clf.master.cpu()
    err = (p_k.double() - p64).abs()
    tol = lr * (move + ADAM_RHO_MARGIN * rho_r)
    tight = float((move < 1e-3).double().mean())
    print(f"RATIO e2e {o64.shape_id(shape)} B={B}: max err/tol={float((err / tol).max()):.3f} "
          f"rho_ref={rho_r:.2e} share of params with a tight (<1e-3 lr) gradient term={tight:.2f}")
    assert (err <= tol).all(), f"worst err/tol {float((err / tol).max()):.3f}"
    pads = o64.pad_mask(g)
    for name, x in (("master", p_k), ("m", clf.m.cpu()), ("v", clf.v.cpu())):
        assert (x[pads] == 0).all(), f"{name}: padded parameter moved"
    assert torch.equal(clf.bfmirror.cpu(), p_k.bfloat16())
    dloss = abs(float(loss_out.item()) - float(grads64[g.nparam]))
    assert dloss <= o64.loss_bound(H, case.W2bf, g, case.invB)
