"""CPU checks of the regression fp64 oracle (tests/oracle64_reg.py) and of
the case list the GPU tests run: the oracle against torch.autograd, and, for
every case, the conditions the kernel-vs-oracle bounds rest on, measured on
the oracle and on the bf16-mirroring reference (never on a kernel)."""

import pytest
import torch

import oracle64 as o64
import oracle64_reg as o64r
from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import HEAD_REGRESSION, Geometry

STEP = o64r.step_cases()
PREDICT = o64r.predict_cases()


def _autograd_step(case):
    """The same loss through torch.autograd on plain fp64 leaves."""
    g = case.g
    W1, b1, W2, b2 = (t.clone().requires_grad_(True)
                      for t in o64._real_operands(g, case.W1bf, case.W2bf, case.master))
    X = case.Xbf.double()[:, : g.in_features]
    z = torch.relu(X @ W1 + b1) @ W2 + b2
    loss = 0.5 * case.invB * torch.nn.functional.mse_loss(
        z, case.Yt.double()[:, : g.classes], reduction="sum")
    loss.backward()
    return {"W1": W1.grad, "b1": b1.grad, "W2": W2.grad, "b2": b2.grad}, loss.detach()


@pytest.mark.parametrize("shape,B", [((20, 32, 1), 33), ((100, 50, 7), 300),
                                     ((33, 250, 3), 1), ((32, 32, 17), 129),
                                     ((200, 128, 32), 33), ((1, 1, 1), 65)],
                         ids=lambda v: o64.shape_id(v) if isinstance(v, tuple) else f"B{v}")
def test_step64_reg_matches_autograd(shape, B):
    """step64_reg is hand-written backprop; autograd on the same fp64
    forward must agree to 1e-12 relative, which makes the oracle
    independent of ops/reference.py."""
    case = o64r.make_case_reg(shape, B, seed=3)
    grads, _, _, _ = o64r.step64_reg(case.g, case.Xbf, case.Yt, case.W1bf, case.W2bf,
                                     case.master, case.invB)
    auto, loss = _autograd_step(case)
    assert abs(float(grads[case.g.nparam] - loss)) <= 1e-12 * abs(float(loss))
    seg = o64.real_segments(case.g, grads)
    for s in o64.SEGMENTS:
        scale = float(auto[s].abs().max())
        assert float((seg[s] - auto[s]).abs().max()) <= 1e-12 * scale, s
    assert (grads[: case.g.nparam][o64.pad_mask(case.g)] == 0).all()


def test_predict64_reg_is_the_affine_of_the_forward():
    """predict64_reg de-standardizes the very z that step64_reg's forward
    produces (identity feature scaler, X already bf16-exact)."""
    case = o64r.make_case_reg((100, 50, 7), 9, seed=3)
    g = case.g
    X = case.Xbf.float()[:, : g.in_features]
    mean, invstd = torch.zeros(g.in_features), torch.ones(g.in_features)
    out, _, z = o64r.predict64_reg(g, X, mean, invstd, case.W1bf, case.W2bf, case.master,
                                   case.y_mean, case.y_scale)
    _, _, _, z_step = o64r.step64_reg(g, case.Xbf, case.Yt, case.W1bf, case.W2bf,
                                      case.master, case.invB)
    assert torch.equal(z, z_step)
    assert torch.equal(out, z * case.y_scale.double() + case.y_mean.double())


def test_case_inputs():
    """make_case_reg keeps its promises: non-zero biases on real entries
    only, zero pads in master, X and Yt, target columns scaled 0.5..2, a
    fitted scaler that is far from the identity."""
    for shape, B in [((100, 50, 7), 300), ((33, 250, 3), 1), ((32, 32, 17), 5),
                     ((20, 32, 1), 129)]:
        c = o64r.make_case_reg(shape, B, seed=1)
        g = c.g
        assert g.head == HEAD_REGRESSION and not g.is_specialized
        seg = o64.real_segments(g, c.master)
        assert (seg["b1"] != 0).all() and (seg["b2"] != 0).all()
        assert (c.master[o64.pad_mask(g)] == 0).all()
        assert (c.Xbf[:, g.in_features:] == 0).all()
        assert c.Yt.shape == (B, g.cpad) and c.Yt.dtype == torch.float32
        assert (c.Yt[:, g.classes:] == 0).all() and (c.Yt[:, : g.classes] != 0).all()
        assert float(c.y_mean.abs().max()) > 50.0
        assert float(c.y_scale.min()) < 0.02
        if g.classes > 1:
            assert float(c.y_scale.max()) > 50.0
    c = o64r.make_case_reg((32, 32, 17), 4000, seed=1)
    std = c.Yt[:, :17].std(dim=0)
    assert abs(float(std[0]) - 0.5) < 0.05 and abs(float(std[-1]) - 2.0) < 0.2


def test_case_matrix_covers_every_regression_instantiation():
    """The regression head is dispatched from the classifier's one table of
    <HID, RT, CPAD> instantiations (header_instantiations asserts that
    tabular_gen.hip holds no second list), the case lists name each row
    once, and each geometry selects the instantiation it is listed under."""
    step, pred = o64.header_instantiations()
    assert len(step) == 11 and len(pred) == 8
    assert sorted(i for i, _ in o64r.STEP_INSTANTIATIONS) == sorted(step)
    assert sorted(i for i, _ in o64r.PRED_INSTANTIATIONS) == sorted(pred)
    for inst, shape in o64r.STEP_INSTANTIATIONS + o64r.PRED_INSTANTIATIONS:
        o64r.check_instantiation(inst, shape)
    shapes = [s for _, s in o64r.STEP_INSTANTIATIONS]
    assert {1, 16, 17, 32} <= {s[2] for s in shapes}
    assert (20, 32, 1) in shapes and (20, 32, 2) not in shapes


@pytest.mark.parametrize("cid,inst,shape,B,seed", STEP, ids=[c[0] for c in STEP])
def test_reference_vs_oracle_step(cid, inst, shape, B, seed):
    """Conditions on every step case. From the oracle alone: every real
    segment of its gradient has non-zero norm (else the case gets another
    seed in SEED_OVERRIDES). On the reference: it sits within 1e-2 (relative
    L2) of the oracle on every segment, so 2*e_r is a meaningful bound for
    the kernel; its pads are exact zeros; its loss is inside the bound the
    kernel is held to."""
    case = o64r.make_case_reg(shape, B, seed)
    g = case.g
    grads64, _, H, z = o64r.step64_reg(g, case.Xbf, case.Yt, case.W1bf, case.W2bf,
                                       case.master, case.invB)
    for s, blk in o64.real_segments(g, grads64).items():
        assert float(blk.norm()) > 0.0, f"{cid}: oracle {s} gradient is all zero"
    grads_r = o64r.reference_step_reg(case)
    errs = o64.segment_errors(g, grads_r, grads64)
    print(cid, {s: "%.2e/%.2e" % v for s, v in errs.items()})
    for s, (e_r, _) in errs.items():
        assert e_r <= 1e-2, f"{cid} {s}: e_r={e_r:.3e}"
    assert (grads_r[: g.nparam][o64.pad_mask(g)] == 0).all()
    loss64 = float(grads64[g.nparam])
    bound = o64r.loss_bound_reg(H, z, case.Yt, case.W2bf, g, case.invB, loss64)
    assert abs(float(grads_r[g.nparam]) - loss64) <= bound


@pytest.mark.parametrize("cid,inst,shape,B,seed", PREDICT, ids=[c[0] for c in PREDICT])
def test_reference_vs_oracle_predict(cid, inst, shape, B, seed):
    """Condition on every predict case: the reference's de-standardized
    outputs sit within 1e-2 of the oracle's largest entry, so 2*emax_r is a
    meaningful bound for the kernel."""
    case = o64r.make_case_reg(shape, B, seed)
    g = case.g
    mean, invstd = ref.standardize_fit(case.Xfit)
    out64, _, _ = o64r.predict64_reg(g, case.X, mean, invstd, case.W1bf, case.W2bf,
                                     case.master, case.y_mean, case.y_scale)
    out_r = ref.mlp_predict_reg_g(g, case.X, mean, invstd, case.W1bf, case.W2bf,
                                  case.master, case.y_mean, case.y_scale)
    assert out_r.shape == (B, g.classes) and out_r.dtype == torch.float32
    emax_r = o64.emax(out_r, out64)
    print(cid, f"emax_r={emax_r:.2e}")
    assert emax_r <= 1e-2


def test_geometry_head():
    """Geometry's head option: defaults unchanged (every ValueError
    included), regression accepts a single output, is never specialized,
    keeps the flat layout and compares unequal to the classifier."""
    with pytest.raises(ValueError):
        Geometry(64, 32, 1)
    with pytest.raises(ValueError, match="classes"):
        Geometry(64, 32, 33)
    with pytest.raises(ValueError, match="hidden"):
        Geometry(64, 300, 10)
    with pytest.raises(ValueError, match="head"):
        Geometry(64, 32, 10, head="ranking")
    with pytest.raises(ValueError):
        Geometry(64, 32, 0, head=HEAD_REGRESSION)
    with pytest.raises(ValueError, match="targets"):
        Geometry(64, 32, 33, head=HEAD_REGRESSION)
    with pytest.raises(ValueError, match="hidden"):
        Geometry(64, 300, 1, head=HEAD_REGRESSION)
    c, r = Geometry(64, 32, 10), Geometry(64, 32, 10, head=HEAD_REGRESSION)
    assert c.head == "classifier" and c.is_specialized and not r.is_specialized
    assert c != r and r == Geometry(64, 32, 10, head=HEAD_REGRESSION)
    assert c == Geometry(64, 32, 10)
    assert (c.inp, c.hid, c.cpad, c.nparam, c.off_b1, c.off_w2, c.off_b2, c.wimg_n) == \
           (r.inp, r.hid, r.cpad, r.nparam, r.off_b1, r.off_w2, r.off_b2, r.wimg_n)
    one = Geometry(10, 32, 1, head=HEAD_REGRESSION)
    assert (one.classes, one.cpad) == (1, 16)
    assert Geometry(10, 32, 17, head=HEAD_REGRESSION).cpad == 32
