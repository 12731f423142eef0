"""The row segment of chunk_fwd_bwd (hip/tabular_kernels.hip), shared by
mlp_step, mlp_step_fused and mlp_train_steps: the twelve bias-gradient sums of
a wave leave through one fold (row_fold12, tabular_common.h) that gives each
lane ONE of them, stored at an offset the lane computes from its slot.

The digests (test_gpu_fused_bits.py, test_gpu_chunk_bits.py) hold the bits.
This file holds what a digest cannot name: WHICH value lands where.

Routing. A bias sum stored into another sum's slot passes any test whose sums
are alike, so the cases here are built by hand, on the CPU and from the fp64
oracle alone:
  - class 0 is never a label, so its dLogits column is positive on every row,
    and W2 has that column only: db1[h] is W2[h][0] times a positive sum over
    the rows on which unit h is active, free of cancellation (the bf16
    reference, whose own error sets the tolerance, stays at a few 1e-3). The
    column is rescaled until db1 is the ladder (-1)^h (h+1)/32 of its largest
    entry;
  - b2 is log(c + 1), which spreads the class probabilities and with them db2;
  - the case is kept only if every two db1 entries and every two db2 entries
    are at least GAP_TOLERANCES tolerances of check_step (test_gpu_oracle.py)
    apart, and every hidden unit is active on some rows and inactive on
    others, so that the mask of dH matters for every db1 entry; else the next
    seed is tried.
One row (B = 1) cannot give the last condition, and its inactive units all
have db1 = 0: there the conditions hold over the active units, and both kinds
of unit exist. A misrouted or unmasked value is then many tolerances off. The
tolerances are check_step's for gradients and, for a master after one Adam
step, the bound of test_gpu_chunk_pair.py; none is defined here.

Batches: one row; 15, 16, 17 around one wave's block of rows; 127, 128, 129
around one workgroup; 256, two workgroups.

Two more properties of the segment, which this file pins as they are:
  - the ReLU mask of dH is taken on H as stored, rounded to bf16: a
    pre-activation that is positive in fp32 and rounds to bf16 zero passes no
    gradient, exactly;
  - dW2 stands in the slab as [h][CPAD], element by element the oracle's."""

import functools

import pytest
import torch

import oracle64 as o64
from test_gpu_oracle import (ADAM_RHO_MARGIN, F64, LR, check_step, f32, gpu_clf, rho,
                             sign_step)
from unionml_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPE = o64.SPEC_SHAPE
ROWS = o64.SPEC_RT
BATCHES = [1, 15, 16, 17, 127, 128, 129, 256]
# A condition on the CASES, checked on the CPU, never a bound on a kernel's
# output: two values count as told apart by check_step when they differ by
# at least this many of its tolerances.
GAP_TOLERANCES = 4.0
SEEDS = range(40, 60)
W2_COLUMN0 = 0.05     # largest |W2[h][0]| of a routing case


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# cases (CPU only)
# ---------------------------------------------------------------------------


def _refresh(case):
    """bfmirror and its views after master changed"""
    g = case.g
    case.bfmirror = case.master.bfloat16()
    case.W1bf = case.bfmirror[g.off_w1 : g.off_w1 + g.inp * g.hid].view(g.inp, g.hid)
    case.W2bf = case.bfmirror[g.off_w2 : g.off_w2 + g.hid * g.cpad].view(g.hid, g.cpad)


def _step64(case):
    return o64.step64(case.g, case.Xbf, case.y, case.W1bf, case.W2bf, case.master, case.invB)


def seg_tol(case, grads64, s):
    """check_step's bound on the largest error in segment s, as an absolute
    number. For conditions on the cases only."""
    g = case.g
    _, emax_r = o64.segment_errors(g, o64.reference_step(case), grads64)[s]
    return max(2 * emax_r, o64.BF16_ULP) * float(o64.real_segments(g, grads64)[s].abs().max())


def _min_gap(x):
    d = (x[:, None] - x[None, :]).abs()
    d.fill_diagonal_(float("inf"))
    return float(d.min())


def _routing_candidate(B, seed):
    case = o64.make_case(SHAPE, B, seed)
    g = case.g
    gen = torch.Generator().manual_seed(7000 + seed)
    case.y = torch.randint(1, g.classes, (B,), generator=gen, dtype=torch.int32)
    ladder = torch.tensor([(-1.0) ** h * (h + 1) / g.hidden for h in range(g.hidden)], dtype=F64)
    seg = o64.real_segments(g, case.master)
    seg["W2"].zero_()
    seg["W2"][:, 0] = (W2_COLUMN0 * ladder).float()
    seg["b2"].copy_(torch.log(torch.arange(1, g.classes + 1, dtype=torch.float32)))
    _refresh(case)
    # db1[h] = W2[h][0] * S[h] with S[h] > 0 the sum of dLogits[:, 0] over the
    # rows on which h is active; S depends on W2 only through logit 0, weakly,
    # so dividing the column by S settles in a few rounds
    for _ in range(6):
        db1 = o64.real_segments(g, _step64(case)[0])["b1"]
        live = db1 != 0
        if not live.any():
            break
        S = torch.ones(g.hidden, dtype=F64)
        S[live] = db1[live] / seg["W2"][:, 0].double()[live]
        assert (S > 0).all()
        seg["W2"][:, 0] = (W2_COLUMN0 * ladder * float(S[live].min()) / S).float()
        _refresh(case)
    return case


def _routing_miss(case):
    """None if the case meets the conditions of the module docstring, else why not"""
    g = case.g
    grads64, Hpre, _, _ = _step64(case)
    seg64 = o64.real_segments(g, grads64)
    active = (Hpre > 0).any(dim=0)
    mixed = active & (Hpre <= 0).any(dim=0)
    if case.B == 1:
        if not (active.any() and (~active).any()):
            return "one row: units of one kind only"
        units = active
    else:
        if not mixed.all():
            return f"{int((~mixed).sum())} units always or never active"
        units = torch.ones(g.hidden, dtype=torch.bool)
    assert not (case.y == 0).any()
    for s, vals in (("b1", seg64["b1"][units]), ("b2", seg64["b2"])):
        tol = seg_tol(case, grads64, s)
        if _min_gap(vals) < GAP_TOLERANCES * tol:
            return f"d{s}: two entries {_min_gap(vals) / tol:.2f} tolerances apart"
    return None


@functools.lru_cache(maxsize=None)
def routing_case(B):
    why = []
    for seed in SEEDS:
        case = _routing_candidate(B, seed)
        miss = _routing_miss(case)
        if miss is None:
            return case
        why.append(f"seed {seed}: {miss}")
    raise AssertionError(f"no seed gives a routing case at B={B}: " + "; ".join(why))


def _fused(ext, dev, case, clf, grads_out):
    clf._ensure_slabs((case.B + ROWS - 1) // ROWS)
    loss_out = torch.zeros(1, device=dev)
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    assert ext.mlp_step_fused(
        case.Xbf.to(dev), case.y.to(dev), clf.W1bf, clf.W2bf, clf.master, clf.bfmirror,
        clf.m, clf.v, clf.t_dev, clf.slabs, clf.counter, loss_out, case.invB, LR,
        ADAM_BETA1, ADAM_BETA2, ADAM_EPS, grads_out=grads_out, wimg=clf.wimg)
    torch.cuda.synchronize()
    return loss_out


def check_master_after_one_step(tag, case, clf, loss_out):
    """master after one Adam step from zero moments against adam64(step64()),
    the bound of test_mlp_train_steps_one_step_vs_oracle (test_gpu_chunk_pair.py)"""
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    g = clf.g
    assert int(clf.t_dev.item()) == 1
    lr, eps = f32(LR), f32(ADAM_EPS)
    b1, b2 = f32(ADAM_BETA1), f32(ADAM_BETA2)
    grads64, _, H, _ = _step64(case)
    g64 = grads64[: g.nparam]
    p64 = o64.adam64(case.master, [g64], lr, b1, b2, eps)[0][0]
    delta = torch.zeros(g.nparam, dtype=F64)
    dseg = o64.real_segments(g, delta)
    for s in o64.SEGMENTS:
        dseg[s].fill_(seg_tol(case, grads64, s))
    move = torch.maximum((sign_step(g64 + delta, eps) - sign_step(g64, eps)).abs(),
                         (sign_step(g64 - delta, eps) - sign_step(g64, eps)).abs())
    p_r, mir_r = case.master.clone(), case.bfmirror.clone()
    m_r, v_r = torch.zeros(g.nparam), torch.zeros(g.nparam)
    ref.adam_step_g(g, p_r, mir_r, g64.float(), m_r, v_r, 1, lr, b1, b2, eps)
    rho_r = rho(p_r, case.master, p64 - case.master.double())

    p_k = clf.master.cpu()
    err = (p_k.double() - p64).abs()
    tol = lr * (move + ADAM_RHO_MARGIN * rho_r)
    print(f"RATIO {tag}: max err/tol={float((err / tol).max()):.3f}")
    assert (err <= tol).all(), f"{tag}: worst err/tol {float((err / tol).max()):.3f}"
    pads = o64.pad_mask(g)
    for name, x in (("master", p_k), ("m", clf.m.cpu()), ("v", clf.v.cpu())):
        assert (x[pads] == 0).all(), f"{tag} {name}: padded parameter moved"
    assert torch.equal(clf.bfmirror.cpu(), p_k.bfloat16())
    dloss = abs(float(loss_out.item()) - float(grads64[g.nparam]))
    assert dloss <= o64.loss_bound(H, case.W2bf, g, case.invB)


# ---------------------------------------------------------------------------
# routing of the bias sums
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("B", BATCHES)
def test_routing_fused_reduce_only(ext, dev, B):
    case = routing_case(B)
    clf = gpu_clf(case, dev)
    grads = torch.full((clf.g.nparam + 1,), float("nan"), device=dev)
    _fused(ext, dev, case, clf, grads)
    assert int(clf.t_dev.item()) == 0
    check_step(f"rowseg-reduce-B{B}", case, grads)


@pytest.mark.parametrize("B", BATCHES)
def test_routing_fused_adam(ext, dev, B):
    case = routing_case(B)
    clf = gpu_clf(case, dev)
    loss_out = _fused(ext, dev, case, clf, None)
    check_master_after_one_step(f"rowseg-fused-B{B}", case, clf, loss_out)


@pytest.mark.parametrize("B", BATCHES)
def test_routing_mlp_step(ext, dev, B):
    case = routing_case(B)
    clf = gpu_clf(case, dev)
    grads = torch.zeros(clf.g.nparam + 1, device=dev)
    ext.mlp_step(case.Xbf.to(dev), case.y.to(dev), clf.W1bf, clf.W2bf, clf.master, grads,
                 case.invB)
    torch.cuda.synchronize()
    check_step(f"rowseg-mlp_step-B{B}", case, grads)


@pytest.mark.parametrize("B", [128, 256])
def test_routing_train_steps_one_step(ext, dev, B):
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    case = routing_case(B)
    clf = gpu_clf(case, dev)
    loss_out = torch.zeros(1, device=dev)
    assert ext.mlp_train_steps(case.Xbf.to(dev), case.y.to(dev), B, 1, clf.master,
                               clf.bfmirror, clf.m, clf.v, clf.t_dev, loss_out, LR,
                               ADAM_BETA1, ADAM_BETA2, ADAM_EPS)
    torch.cuda.synchronize()
    check_master_after_one_step(f"rowseg-train_steps-B{B}", case, clf, loss_out)


# ---------------------------------------------------------------------------
# a pre-activation that is positive in fp32 and rounds to bf16 zero
# ---------------------------------------------------------------------------

TINY = 1e-41                  # fp32 subnormal; below half the smallest bf16 subnormal
DEAD_UNITS = (3, 17, 30)      # TINY on every row
MIXED_UNITS = (5, 20)         # TINY on the even rows, about 1 on the odd ones
FLAG_COLUMN = 7               # the input column that tells the rows apart


@functools.lru_cache(maxsize=None)
def tiny_case():
    B = 16
    case = o64.make_case(SHAPE, B, o64.case_seed(SHAPE, B))
    g = case.g
    case.Xbf[:, FLAG_COLUMN] = (torch.arange(B) % 2).to(torch.bfloat16)
    seg = o64.real_segments(g, case.master)
    for h in DEAD_UNITS + MIXED_UNITS:
        seg["W1"][:, h] = 0.0
        seg["b1"][h] = TINY
    for h in MIXED_UNITS:
        seg["W1"][FLAG_COLUMN, h] = 1.0
    assert float(seg["b1"][DEAD_UNITS[0]]) > 0.0, "the subnormal bias was flushed"
    _refresh(case)
    return case


def step64_mask_on_rounded_h(case):
    """o64.step64 with the ReLU mask taken on H as the kernels store it
    (rounded to bf16), which is what they are documented to do"""
    g = case.g
    W1, b1, W2, b2 = o64._real_operands(g, case.W1bf, case.W2bf, case.master)
    X = case.Xbf.to(F64)[:, : g.in_features]
    rows, yl = torch.arange(case.B), case.y.long()
    Hpre, H, logits = o64.forward64(X, W1, b1, W2, b2)
    mask = H.float().bfloat16().to(F64) > 0
    H = H * mask
    logits = H @ W2 + b2
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    dlogits = torch.exp(logp)
    dlogits[rows, yl] -= 1.0
    dlogits *= case.invB
    dH = (dlogits @ W2.T) * mask
    grads = torch.zeros(g.nparam + 1, dtype=F64)
    seg = o64.real_segments(g, grads)
    seg["W1"].copy_(X.T @ dH)
    seg["b1"].copy_(dH.sum(dim=0))
    seg["W2"].copy_(H.T @ dlogits)
    seg["b2"].copy_(dlogits.sum(dim=0))
    grads[g.nparam] = -logp[rows, yl].sum() * case.invB
    return grads, Hpre, H, logits


@pytest.mark.parametrize("kernel", ["mlp_step_fused", "mlp_step"])
def test_relu_mask_is_the_rounded_h(ext, dev, kernel, monkeypatch):
    case = tiny_case()
    g = case.g
    grads64, Hpre, H, _ = step64_mask_on_rounded_h(case)
    mask = H > 0
    # the case is what it claims to be (CPU)
    for h in DEAD_UNITS:
        assert (Hpre[:, h] > 0).all() and not mask[:, h].any()
    for h in MIXED_UNITS:
        assert (Hpre[:, h] > 0).all()
        assert not mask[0::2, h].any() and mask[1::2, h].all()
    plain = o64.real_segments(g, _step64(case)[0])
    want = o64.real_segments(g, grads64)
    tol_b1 = seg_tol(case, grads64, "b1")
    for h in MIXED_UNITS:   # a mask on the unrounded value is many tolerances off
        assert abs(float(plain["b1"][h] - want["b1"][h])) > GAP_TOLERANCES * tol_b1

    clf = gpu_clf(case, dev)
    if kernel == "mlp_step":
        grads = torch.zeros(g.nparam + 1, device=dev)
        ext.mlp_step(case.Xbf.to(dev), case.y.to(dev), clf.W1bf, clf.W2bf, clf.master, grads,
                     case.invB)
        torch.cuda.synchronize()
    else:
        grads = torch.full((g.nparam + 1,), float("nan"), device=dev)
        _fused(ext, dev, case, clf, grads)
    got = o64.real_segments(g, grads.cpu())
    for h in DEAD_UNITS:
        assert (got["W1"][:, h] == 0).all(), f"unit {h}: dW1 column not exactly zero"
        assert float(got["b1"][h]) == 0.0, f"unit {h}: db1 not exactly zero"
        assert (got["W2"][h] == 0).all(), f"unit {h}: dW2 row not exactly zero"
    # the rest, the mixed units among it: check_step itself, with the oracle it
    # calls replaced by the one that masks on the rounded H
    monkeypatch.setattr(o64, "step64", lambda *a: step64_mask_on_rounded_h(case))
    check_step(f"rowseg-tiny-{kernel}", case, grads)


# ---------------------------------------------------------------------------
# dW2 in the slab: [h][CPAD]
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("B", [16, 128])
def test_dw2_slab_layout(ext, dev, B):
    """One workgroup: slab 0 IS this launch's flat gradient, dW2 at OFF_W2 +
    h * CPAD + c among it. It goes through check_step as a gradient vector
    does: every segment, dW2 element by element against its largest entry,
    the pad classes exactly zero. A transposed or permuted tile is many
    tolerances off (asserted on the oracle)."""
    case = o64.make_case(SHAPE, B, o64.case_seed(SHAPE, B))
    g = case.g
    grads64 = _step64(case)[0]
    want = o64.real_segments(g, grads64)["W2"]
    n = min(g.hidden, g.classes)
    assert (float((want[:n, :n] - want[:n, :n].T).abs().max())
            > GAP_TOLERANCES * seg_tol(case, grads64, "W2"))

    clf = gpu_clf(case, dev)
    grads = torch.full((g.nparam + 1,), float("nan"), device=dev)
    _fused(ext, dev, case, clf, grads)
    check_step(f"rowseg-slab-B{B}", case, clf.slabs[0, : g.nparam + 1])
