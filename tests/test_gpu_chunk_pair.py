"""chunk_fwd_bwd (hip/tabular_kernels.hip), the chunk that mlp_step,
mlp_step_fused and mlp_train_steps share: its row segment rounds H, dLogits
and dH to bf16 two values at a time (f2bf_pair) and keeps the rounded H in
packed words for dH; waves 0 and 1 run two weight-gradient GEMMs, the other
waves one.

The chunk digests (test_gpu_chunk_bits.py) hold the bits against earlier
builds. This file holds the values against the fp64 oracle, with the helpers
and at the tolerances of test_gpu_oracle.py, at the row counts where a
one-workgroup chunk has one row, one full wave of rows, one row more, one row
short of full and full; and for the persistent kernel, which calls the
function in its accumulating form, with one chunk per step and with two."""

import pytest
import torch

import oracle64 as o64
from test_gpu_oracle import (ADAM_RHO_MARGIN, F64, LR, check_step, f32, gpu_clf, rho,
                             sign_step)
from unionml_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPE = o64.SPEC_SHAPE


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.mark.parametrize("B", [1, 16, 17, 127, 128])
def test_mlp_step_one_workgroup_vs_oracle(ext, dev, B):
    case = o64.make_case(SHAPE, B, o64.case_seed(SHAPE, B))
    clf = gpu_clf(case, dev)
    grads = torch.zeros(clf.g.nparam + 1, device=dev)
    ext.mlp_step(case.Xbf.to(dev), case.y.to(dev), clf.W1bf, clf.W2bf, clf.master, grads,
                 case.invB)
    torch.cuda.synchronize()
    check_step(f"mlp_step-pair-B{B}", case, grads)


@pytest.mark.parametrize("B", [128, 256])
def test_mlp_train_steps_one_step_vs_oracle(ext, dev, B):
    """One optimizer step of the persistent kernel over N = B rows (one chunk
    at B = 128, two at 256): master lands where adam64(step64()) lands, within
    the tolerance of test_one_fused_step_end_to_end: the image under the first
    Adam step of the step test's gradient bound, plus ADAM_RHO_MARGIN times
    the reference's own Adam error."""
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    case = o64.make_case(SHAPE, B, o64.case_seed(SHAPE, B))
    clf = gpu_clf(case, dev)
    g = clf.g
    loss_out = torch.zeros(1, device=dev)
    assert ext.mlp_train_steps(case.Xbf.to(dev), case.y.to(dev), B, 1, clf.master,
                               clf.bfmirror, clf.m, clf.v, clf.t_dev, loss_out, LR,
                               ADAM_BETA1, ADAM_BETA2, ADAM_EPS)
    torch.cuda.synchronize()
    assert int(clf.t_dev.item()) == 1

    lr, eps = f32(LR), f32(ADAM_EPS)
    b1, b2 = f32(ADAM_BETA1), f32(ADAM_BETA2)
    grads64, _, H, _ = o64.step64(g, case.Xbf, case.y, case.W1bf, case.W2bf, case.master,
                                  case.invB)
    g64 = grads64[: g.nparam]
    p64 = o64.adam64(case.master, [g64], lr, b1, b2, eps)[0][0]

    err_r = o64.segment_errors(g, o64.reference_step(case), grads64)
    delta = torch.zeros(g.nparam, dtype=F64)
    dseg, oseg = o64.real_segments(g, delta), o64.real_segments(g, g64)
    for s in o64.SEGMENTS:
        dseg[s].fill_(max(2 * err_r[s][1], o64.BF16_ULP) * float(oseg[s].abs().max()))
    move = torch.maximum((sign_step(g64 + delta, eps) - sign_step(g64, eps)).abs(),
                         (sign_step(g64 - delta, eps) - sign_step(g64, eps)).abs())
    p_r, mir_r = case.master.clone(), case.bfmirror.clone()
    m_r, v_r = torch.zeros(g.nparam), torch.zeros(g.nparam)
    ref.adam_step_g(g, p_r, mir_r, g64.float(), m_r, v_r, 1, lr, b1, b2, eps)
    rho_r = rho(p_r, case.master, p64 - case.master.double())

    p_k = clf.master.cpu()
    err = (p_k.double() - p64).abs()
    tol = lr * (move + ADAM_RHO_MARGIN * rho_r)
    print(f"RATIO train_steps B={B}: max err/tol={float((err / tol).max()):.3f}")
    assert (err <= tol).all(), f"worst err/tol {float((err / tol).max()):.3f}"
    pads = o64.pad_mask(g)
    for name, x in (("master", p_k), ("m", clf.m.cpu()), ("v", clf.v.cpu())):
        assert (x[pads] == 0).all(), f"{name}: padded parameter moved"
    assert torch.equal(clf.bfmirror.cpu(), p_k.bfloat16())
    dloss = abs(float(loss_out.item()) - float(grads64[g.nparam]))
    assert dloss <= o64.loss_bound(H, case.W2bf, g, case.invB)
