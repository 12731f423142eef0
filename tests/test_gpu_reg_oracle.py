"""The regression instantiations of the generalized HIP kernels against the
plain fp64 oracle (tests/oracle64_reg.py).

Every mlp_step_reg_gen / mlp_predict_reg_gen instantiation is launched
directly (rt= picks the rows-per-workgroup variant), with NON-ZERO biases,
at the batch sizes around a workgroup's row count. Bounds are either derived
(loss) or measured IN THE SAME TEST on the bf16-mirroring reference
(ops/reference.py mlp_step_reg_g / mlp_predict_reg_g) against the oracle,
never on the kernel under test; tests/test_oracle64_reg_cpu.py checks the
case list's conditions on the CPU.

Run with -s to see every measured ratio (docs/kernels.md, "Regression
head", records the largest per kernel)."""

import pytest
import torch

import oracle64 as o64
import oracle64_reg as o64r
from unionml_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

LR, EPS = 1e-3, 1e-8


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def gpu_reg(case, dev):
    """A TabularMLPRegressor carrying the case's weights, non-zero biases
    and fitted target scaler"""
    from unionml_amd.ops.tabular import TabularMLPRegressor

    inf, hid, T = case.shape
    reg = TabularMLPRegressor(in_features=inf, hidden=hid, targets=T, device=dev,
                              seed=case.seed)
    reg.master.copy_(case.master.to(dev))
    reg.bfmirror.copy_(reg.master.bfloat16())
    reg._build_wimg()
    assert torch.equal(reg.bfmirror.cpu(), case.bfmirror)
    reg.y_mean.copy_(case.y_mean.to(dev))
    reg.y_invstd.copy_(case.y_invstd.to(dev))
    reg.y_scale.copy_(case.y_scale.to(dev))
    return reg


# ---------------------------------------------------------------------------
# step
# ---------------------------------------------------------------------------


def check_step_reg(name, case, grads_k):
    """The rule of tests/test_gpu_oracle.py::check_step on the squared-error
    step: exact-zero pads, per-segment error within twice the reference's
    own (floor one bf16 ulp), loss within its derived bound."""
    g = case.g
    grads_k = grads_k.cpu()
    assert torch.isfinite(grads_k).all(), "unwritten or non-finite gradient entries"
    assert (grads_k[: g.nparam][o64.pad_mask(g)] == 0).all(), "padded parameter leaked gradient"

    grads64, _, H, z = o64r.step64_reg(g, case.Xbf, case.Yt, case.W1bf, case.W2bf,
                                       case.master, case.invB)
    err_r = o64.segment_errors(g, o64r.reference_step_reg(case), grads64)
    err_k = o64.segment_errors(g, grads_k, grads64)
    failures = []
    for s in o64.SEGMENTS:
        (e_k, emax_k), (e_r, emax_r) = err_k[s], err_r[s]
        print(f"RATIO regstep {name} {s}: e_k={e_k:.3e} e_r={e_r:.3e} e_k/e_r={e_k / e_r:.3f} "
              f"emax_k={emax_k:.3e} emax_r={emax_r:.3e} emax_k/emax_r={emax_k / emax_r:.3f}")
        if not e_k <= max(2 * e_r, o64.BF16_ULP):
            failures.append(f"{s}: e_k={e_k:.3e} > max(2*{e_r:.3e}, 2^-8)")
        if not emax_k <= max(2 * emax_r, o64.BF16_ULP):
            failures.append(f"{s}: emax_k={emax_k:.3e} > max(2*{emax_r:.3e}, 2^-8)")
    assert not failures, f"{name}: " + "; ".join(failures)

    loss64 = float(grads64[g.nparam])
    bound = o64r.loss_bound_reg(H, z, case.Yt, case.W2bf, g, case.invB, loss64)
    dloss = abs(float(grads_k[g.nparam].double()) - loss64)
    print(f"RATIO regloss {name}: |dloss|={dloss:.3e} bound={bound:.3e} "
          f"dloss/bound={dloss / bound:.3f}")
    assert dloss <= bound, f"{name}: loss off by {dloss:.3e} > {bound:.3e}"


def run_reg_step(ext, dev, case, rt):
    """mlp_step_reg_gen at an explicit rows-per-workgroup, then the
    reduce-only slab sum. Slabs start as NaN: every entry the reduction
    reads must have been stored by the step kernel in this launch."""
    reg = gpu_reg(case, dev)
    g = reg.g
    n_wg = (case.B + rt - 1) // rt
    slabs = torch.full((n_wg, g.slab_stride), float("nan"), device=dev)
    counter = torch.zeros(1, dtype=torch.uint32, device=dev)
    grads = torch.full((g.nparam + 1,), float("nan"), device=dev)
    loss_out = torch.zeros(1, device=dev)
    master0 = reg.master.clone()
    ok = ext.mlp_step_reg_gen(case.Xbf.to(dev), case.Yt.to(dev), g.hid, g.classes, rt,
                              reg.wimg, reg.master, slabs, case.invB)
    assert ok
    ext.reduce_adam_gen(slabs, n_wg, g.inp, g.hid, g.cpad, reg.master, reg.bfmirror,
                        reg.m, reg.v, reg.t_dev, counter, loss_out, LR, 0.9, 0.999, EPS,
                        wimg=reg.wimg, grads_out=grads)
    torch.cuda.synchronize()
    assert int(reg.t_dev.item()) == 0 and int(counter.item()) == 0
    assert torch.equal(reg.master, master0)
    return grads


STEP = o64r.step_cases()


@pytest.mark.parametrize("cid,inst,shape,B,seed", STEP, ids=[c[0] for c in STEP])
def test_reg_step_vs_oracle(ext, dev, cid, inst, shape, B, seed):
    """Every regression step instantiation <HID,RT,CPAD>, launched directly."""
    case = o64r.make_case_reg(shape, B, seed)
    o64r.check_instantiation(inst, shape)
    check_step_reg(cid, case, run_reg_step(ext, dev, case, inst[1]))


def test_reg_step_ignores_target_pads(ext, dev):
    """The pad-leak property from the target side: garbage in Yt's pad
    columns changes nothing (a select masks it, not a multiply). B = RT+1,
    so the second workgroup is all tail rows but one; their masking is what
    the oracle cases at B = RT-1 and RT+1 check."""
    inst, shape = (64, 128, 16), (70, 50, 7)
    B = inst[1] + 1
    case = o64r.make_case_reg(shape, B, o64r.case_seed(shape, B))
    clean = run_reg_step(ext, dev, case, inst[1]).cpu()
    case.Yt[:, shape[2]:] = 1e30
    dirty = run_reg_step(ext, dev, case, inst[1]).cpu()
    g = case.g
    assert (dirty[: g.nparam][o64.pad_mask(g)] == 0).all()
    # every sum of the step is order-fixed: the whole vector, loss included
    assert torch.equal(clean, dirty)


# ---------------------------------------------------------------------------
# predict
# ---------------------------------------------------------------------------

SENTINEL = -7.0
GUARD = 3

PREDICT = o64r.predict_cases()


@pytest.mark.parametrize("cid,inst,shape,B,seed", PREDICT, ids=[c[0] for c in PREDICT])
def test_reg_predict_vs_oracle(ext, dev, cid, inst, shape, B, seed):
    """Every regression predict instantiation with a fitted, far-from-identity
    target scaler, into an oversized pre-poisoned output: rows >= B and
    columns >= T stay untouched."""
    case = o64r.make_case_reg(shape, B, seed)
    o64r.check_instantiation(inst, shape)
    reg = gpu_reg(case, dev)
    g = reg.g
    T = g.classes
    ext.standardize_fit(case.Xfit.to(dev), reg.mean, reg.invstd, 1e-5)
    out = torch.full((B + GUARD, T + GUARD), SENTINEL, device=dev)
    ext.mlp_predict_reg_gen(case.X.to(dev), g.inp, g.hid, T, reg.mean, reg.invstd,
                            reg.wimg, reg.master, reg.y_mean, reg.y_scale, out)
    torch.cuda.synchronize()
    out = out.cpu()
    assert (out[B:] == SENTINEL).all(), "wrote rows past B"
    assert (out[:, T:] == SENTINEL).all(), "wrote columns past T"
    out_k = out[:B, :T]
    assert torch.isfinite(out_k).all()

    mean, invstd = reg.mean.cpu(), reg.invstd.cpu()
    out64, _, _ = o64r.predict64_reg(g, case.X, mean, invstd, case.W1bf, case.W2bf,
                                     case.master, case.y_mean, case.y_scale)
    out_r = ref.mlp_predict_reg_g(g, case.X, mean, invstd, case.W1bf, case.W2bf,
                                  case.master, case.y_mean, case.y_scale)
    emax_k, emax_r = o64.emax(out_k, out64), o64.emax(out_r, out64)
    print(f"RATIO regpredict {cid}: emax_k={emax_k:.3e} emax_r={emax_r:.3e} "
          f"emax_k/emax_r={emax_k / max(emax_r, 1e-300):.3f}")
    assert emax_k <= max(2 * emax_r, o64.BF16_ULP), \
        f"{cid}: emax_k={emax_k:.3e} > max(2*{emax_r:.3e}, 2^-8)"

    # the class's own predict() is the same kernel into a tight [B][T]
    tight = reg.predict(case.X.to(dev)).cpu()
    assert tight.shape == (B, T) and torch.equal(tight, out_k)
