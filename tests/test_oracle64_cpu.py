"""CPU checks of the fp64 oracle (tests/oracle64.py) and of the case list
the GPU oracle tests run: the oracle against torch.autograd, and, for every
case, the conditions the kernel-vs-oracle bounds rest on, measured on the
bf16-mirroring reference (never on a kernel)."""

from fractions import Fraction

import pytest
import torch

import oracle64 as o64
from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import Geometry

GEN_STEP = o64.gen_step_cases()
SPEC_STEP = o64.spec_step_cases()
PREDICT = o64.predict_cases()

ALL_STEP = [(cid, shape, B, seed) for cid, _, shape, B, seed in GEN_STEP] + SPEC_STEP
# the end-to-end cases run one step too: same conditions
ALL_STEP += [(f"e2e-{o64.shape_id(s)}-B{B}", s, B, o64.case_seed(s, B))
             for s, B in o64.E2E_CASES]


def _autograd_step(case):
    """The same loss through torch.autograd on plain fp64 leaves."""
    g = case.g
    W1, b1, W2, b2 = (t.clone().requires_grad_(True)
                      for t in o64._real_operands(g, case.W1bf, case.W2bf, case.master))
    X = case.Xbf.double()[:, : g.in_features]
    logits = torch.relu(X @ W1 + b1) @ W2 + b2
    loss = torch.nn.functional.cross_entropy(logits, case.y.long(), reduction="sum")
    loss = loss * case.invB
    loss.backward()
    return {"W1": W1.grad, "b1": b1.grad, "W2": W2.grad, "b2": b2.grad}, loss.detach()


@pytest.mark.parametrize("shape,B", [((64, 32, 10), 33), ((100, 50, 7), 300),
                                     ((33, 250, 3), 1), ((32, 32, 17), 129),
                                     ((200, 128, 32), 33), ((1, 1, 2), 65)],
                         ids=lambda v: o64.shape_id(v) if isinstance(v, tuple) else f"B{v}")
def test_step64_matches_autograd(shape, B):
    """step64 is hand-written backprop; autograd on the same fp64 forward
    must agree to 1e-12 relative. This is what makes the oracle independent
    of ops/reference.py."""
    case = o64.make_case(shape, B, seed=3)
    grads, _, _, _ = o64.step64(case.g, case.Xbf, case.y, case.W1bf, case.W2bf,
                                case.master, case.invB)
    auto, loss = _autograd_step(case)
    assert abs(float(grads[case.g.nparam] - loss)) <= 1e-12 * abs(float(loss))
    seg = o64.real_segments(case.g, grads)
    for s in o64.SEGMENTS:
        scale = float(auto[s].abs().max())
        assert float((seg[s] - auto[s]).abs().max()) <= 1e-12 * scale, s
    # pads exactly zero
    assert (grads[: case.g.nparam][o64.pad_mask(case.g)] == 0).all()


def test_case_inputs():
    """make_case keeps its promises: non-zero biases on real entries only,
    zero pads, labels that cover the classes and include the last one."""
    for shape, B in [((100, 50, 7), 300), ((33, 250, 3), 1), ((32, 32, 17), 5)]:
        c = o64.make_case(shape, B, seed=1)
        g = c.g
        seg = o64.real_segments(g, c.master)
        assert (seg["b1"] != 0).all() and (seg["b2"] != 0).all()
        assert (c.master[o64.pad_mask(g)] == 0).all()
        assert (c.Xbf[:, g.in_features:] == 0).all()
        assert int(c.y[0]) == g.classes - 1
        assert len(set(c.y.tolist())) == min(B, g.classes)
        assert int(c.y.min()) >= 0 and int(c.y.max()) == g.classes - 1


def test_case_matrix_covers_every_instantiation():
    """The lists name every step / predict row of the instantiation table
    (tabular_launch.h TABULAR_GEN_INSTANTIATIONS) once, and each geometry
    selects the instantiation it is listed under."""
    step, pred = o64.header_instantiations()
    assert len(step) == 11 and len(pred) == 8
    assert sorted(i for i, _ in o64.STEP_INSTANTIATIONS) == sorted(step)
    assert sorted(i for i, _ in o64.PRED_INSTANTIATIONS) == sorted(pred)
    for inst, shape in o64.STEP_INSTANTIATIONS + o64.PRED_INSTANTIATIONS:
        o64.check_instantiation(inst, shape)
    # the coverage the geometries were picked for
    shapes = [s for _, s in o64.STEP_INSTANTIATIONS]
    assert {2, 16, 17, 32} <= {s[2] for s in shapes}
    assert any(Geometry(*s).inp == 32 and Geometry(*s).hid < 256 for s in shapes)
    assert any(Geometry(*s).inp == 32 and Geometry(*s).hid == 256 for s in shapes)
    assert any(Geometry(*s).inp == 64 for s in shapes)
    assert any(Geometry(*s).inp == 96 and Geometry(*s).hid < 256 for s in shapes)
    assert any(Geometry(*s).inp == 160 and Geometry(*s).hid < 256 for s in shapes)
    assert any(Geometry(*s).inp == 96 and Geometry(*s).hid == 256 for s in shapes)
    assert any(s[0] % 32 for s in shapes) and any(s[1] < Geometry(*s).hid for s in shapes)


@pytest.mark.parametrize("cid,shape,B,seed", ALL_STEP, ids=[c[0] for c in ALL_STEP])
def test_reference_vs_oracle_step(cid, shape, B, seed):
    """Condition on every step case: the reference sits within 1e-2
    (relative L2) of the oracle on every segment, so 2*e_r is a meaningful
    bound for the kernel. A segment whose oracle norm is degenerate by
    cancellation fails this and gets another seed in SEED_OVERRIDES."""
    case = o64.make_case(shape, B, seed)
    grads64, _, H, _ = o64.step64(case.g, case.Xbf, case.y, case.W1bf, case.W2bf,
                                  case.master, case.invB)
    grads_r = o64.reference_step(case)
    errs = o64.segment_errors(case.g, grads_r, grads64)
    print(cid, {s: "%.2e/%.2e" % v for s, v in errs.items()})
    for s, (e_r, _) in errs.items():
        assert e_r <= 1e-2, f"{cid} {s}: e_r={e_r:.3e}"
    assert (grads_r[: case.g.nparam][o64.pad_mask(case.g)] == 0).all()
    bound = o64.loss_bound(H, case.W2bf, case.g, case.invB)
    assert abs(float(grads_r[case.g.nparam] - grads64[case.g.nparam])) <= bound


@pytest.mark.parametrize("cid,inst,shape,B,seed", PREDICT, ids=[c[0] for c in PREDICT])
def test_reference_vs_oracle_predict(cid, inst, shape, B, seed):
    """Condition on every predict case: the margin rule excludes at most
    10% of the rows, and on the others the reference's argmax is the
    oracle's."""
    case = o64.make_case(shape, B, seed)
    g = case.g
    mean, invstd = ref.standardize_fit(case.Xfit)
    logits, p64, H = o64.predict64(g, case.X, mean, invstd, case.W1bf, case.W2bf, case.master)
    preds_r, p_r = ref.mlp_predict_g(g, case.X, mean, invstd, case.W1bf, case.W2bf,
                                     case.master, return_probs=True)
    clear = o64.clear_rows(logits, H, case.W2bf, g)
    excluded = 1.0 - float(clear.double().mean())
    print(cid, f"excluded={excluded:.3f}", f"dp_r={float((p_r.double() - p64).abs().max()):.2e}")
    assert excluded <= o64.MAX_EXCLUDED, f"{cid}: {excluded:.3f} of rows inside the slack"
    assert torch.equal(preds_r[clear].long(), logits.argmax(dim=1)[clear])


def test_adam64_first_step_is_sign_step():
    """From zero moments the first bias-corrected step is lr * g/(|g|+eps)
    for ANY betas: pins adam64's bias correction."""
    gr = torch.tensor([0.5, -2.0, 0.0, 1e-6])
    for b1, b2 in ((0.9, 0.999), (0.8, 0.95)):
        p, m, v = o64.adam64(torch.zeros(4), [gr], 1e-3, b1, b2, 1e-8)
        want = -1e-3 * gr.double() / (gr.double().abs() + 1e-8)
        assert torch.allclose(p[0], want, rtol=1e-12, atol=0)
        assert torch.allclose(m[0], (1 - b1) * gr.double(), rtol=1e-15, atol=0)
        assert torch.allclose(v[0], (1 - b2) * gr.double() ** 2, rtol=1e-15, atol=0)


def test_adam64_sees_swapped_betas():
    """With a fresh gradient per step the trajectory depends on which beta
    is which (the constant-gradient case does not)."""
    grads, _ = o64.adam_gradients(64, 4, seed=0)
    a, _, _ = o64.adam64(torch.zeros(64), grads, 1e-3, 0.8, 0.95, 1e-8)
    b, _, _ = o64.adam64(torch.zeros(64), grads, 1e-3, 0.95, 0.8, 1e-8)
    assert float((a[-1] - b[-1]).abs().max()) > 1e-4


def test_standardize64_two_pass():
    """A column at mean/std = 1e4 keeps its variance (the one-pass formula
    in fp32 would lose it), a constant column gives exactly var 0."""
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(257, 2, generator=gen)
    X[:, 0] = X[:, 0] * 1e-2 + 100.0
    X[:, 1] = 3.25
    mean, invstd, var = o64.standardize64(X, 1e-5)
    assert float(var[1]) == 0.0 and float(mean[1]) == 3.25
    centered = X[:, 0].double() - 100.0
    want = centered.var(unbiased=False)
    assert abs(float(var[0]) - float(want)) <= 1e-12 * float(want)
    assert abs(float(invstd[1]) - 1e-5 ** -0.5) <= 1e-12 * 1e-5 ** -0.5


# ---------------------------------------------------------------------------
# the pinned moment formulas (adam_moments32) against exact rationals
# ---------------------------------------------------------------------------


def _rn32(x: Fraction) -> float:
    """x rounded to the nearest fp32 number, ties to even, as a float
    (exact: every fp32 number is a float). Subnormals included."""
    if x == 0:
        return 0.0
    sign, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1                      # now 2^e <= x < 2^(e+1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    q = x / ulp
    n = q.numerator // q.denominator
    r = q - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return sign * float(n * ulp)


def test_rn32_rounds_to_nearest_even():
    one, ulp = Fraction(1), Fraction(2) ** -23
    assert _rn32(one + ulp / 2) == 1.0                        # tie -> even
    assert _rn32(one + ulp + ulp / 2) == 1.0 + 2.0 ** -22     # tie -> even, upward
    assert _rn32(one + ulp / 2 + Fraction(2) ** -80) == 1.0 + 2.0 ** -23
    assert _rn32(-(one + ulp / 2 - Fraction(2) ** -80)) == -1.0
    assert _rn32(Fraction(2) ** -149 * 3 / 2) == 2.0 ** -148  # subnormal tie -> even
    assert _rn32(Fraction(2) - Fraction(2) ** -30) == 2.0     # carries into the next binade
    for x in (0.1, -3.75e-7, 12345.678):
        assert _rn32(Fraction(x)) == float(torch.tensor(x, dtype=torch.float64).float())


def _moments_exact(m, v, gr, b1, b2):
    """adam_moments32's formulas, entry by entry, in exact rationals with one
    explicit rounding per rn() and per fma"""
    B1, B2 = Fraction(b1), Fraction(b2)
    omb1, omb2 = Fraction(_rn32(1 - B1)), Fraction(_rn32(1 - B2))
    m_new, v_new = [], []
    for mi, vi, gi in zip(m.tolist(), v.tolist(), gr.tolist()):
        mi, vi, gi = Fraction(mi), Fraction(vi), Fraction(gi)
        bm, bv = Fraction(_rn32(B1 * mi)), Fraction(_rn32(B2 * vi))
        gs = Fraction(_rn32(omb2 * gi))
        m_new.append(_rn32(omb1 * gi + bm))
        v_new.append(_rn32(gi * gs + bv))
    return (torch.tensor(m_new, dtype=torch.float64).float(),
            torch.tensor(v_new, dtype=torch.float64).float())


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)], ids=["default", "b0.8-0.95"])
@pytest.mark.parametrize("shape", sorted({s for _, s in o64.ADAM_KERNELS}),
                         ids=o64.shape_id)
def test_adam_moments32_matches_exact_rationals(shape, betas):
    """The fp64 evaluation of the pinned moment formulas equals their exact
    rational evaluation on every entry it does not exempt, over the
    gradients test_gpu_oracle.py draws, and it exempts at most
    MAX_MIDPOINT_SHARE of a tensor. An fma whose double rounding really
    goes wrong must be flagged; a made-up one shows the flag works."""
    n = Geometry(*shape).nparam
    grads, _ = o64.adam_gradients(n, o64.ADAM_MOMENT_STEPS, seed=o64.ADAM_GRAD_SEED)
    b1 = float(torch.tensor(betas[0]).float())
    b2 = float(torch.tensor(betas[1]).float())
    m, v = torch.zeros(n), torch.zeros(n)
    exempted = 0
    for t, gr in enumerate(grads, start=1):
        m_new, v_new, ex_m, ex_v = o64.adam_moments32(m, v, gr, b1, b2)
        m_x, v_x = _moments_exact(m, v, gr, b1, b2)
        for name, got, want, ex in (("m", m_new, m_x, ex_m), ("v", v_new, v_x, ex_v)):
            share = float(ex.double().mean())
            assert share <= o64.MAX_MIDPOINT_SHARE, f"{name} t={t}: exempts {share:.2e}"
            assert torch.equal(got[~ex], want[~ex]), f"{name} t={t}"
            exempted += int(ex.sum())
        m, v = m_x, v_x
    print(f"adam_moments32 {o64.shape_id(shape)} betas={betas}: {exempted} entries exempted "
          f"of {2 * n * len(grads)}")


def test_fma32_flags_a_double_rounding():
    """fma(a, b, c) with a*b = 2^-24 - 2^-70 and c = 1 + 2^-23: the exact sum
    lies just below the midpoint of 1 + 2^-23 and 1 + 2^-22 and rounds to the
    former in one step; fp64 first rounds it ONTO the midpoint, and the tie
    then goes to the even neighbour 1 + 2^-22. That entry must be flagged
    (and really is wrong); a true tie is flagged too, harmlessly; a sum away
    from every midpoint is not."""
    h = 2.0 ** -12
    a = torch.tensor([h * (1 + 2.0 ** -23), h, 0.25], dtype=torch.float32)
    b = torch.tensor([h * (1 - 2.0 ** -23), h, 0.5], dtype=torch.float32)
    c = torch.tensor([1 + 2.0 ** -23, 1.0, 1.0], dtype=torch.float32)
    got, ex = o64._fma32(a, b, c)
    assert ex.tolist() == [True, True, False]
    exact = [_rn32(Fraction(x) * Fraction(y) + Fraction(z))
             for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]
    assert exact == [1 + 2.0 ** -23, 1.0, 1.125]
    assert got.tolist() == [1 + 2.0 ** -22, 1.0, 1.125]   # entry 0: double-rounded
