"""The evaluation kernels (mlp_eval_gen_kernel, both heads, all 16
instantiations, and eval_finish_kernel) on the GPU against the fp64 oracle
of tests/oracle64_eval.py, launched through the bindings with non-zero
biases at B = 1, RT-1, RT+1, 2RT+17 and 9RT+5 (ten workgroups).

Bounds are the step's own (oracle64.loss_bound, oracle64_reg.loss_bound_reg)
or measured in the same test on the bf16-mirroring reference, never on the
kernel under test. Run with -s to see every ratio (docs/kernels.md,
"Evaluation", records the largest per instantiation)."""

import pytest
import torch

import oracle64 as o64
import oracle64_eval as o64e
import oracle64_reg as o64r
import order_probe as op
from oracle64 import F64
from unionml_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

NAN = float("nan")
CLS = o64e.cls_cases(gpu=True)
REG = o64e.reg_cases(gpu=True)


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _carry(model, case, dev):
    model.master.copy_(case.master.to(dev))
    model.bfmirror.copy_(model.master.bfloat16())
    model._build_wimg()
    assert torch.equal(model.bfmirror.cpu(), case.bfmirror)
    return model


def gpu_clf(case, dev):
    """A TabularMLP carrying the case's weights and non-zero biases"""
    from unionml_amd.ops.tabular import TabularMLP

    inf, hid, cls = case.shape
    return _carry(TabularMLP(inf, hid, cls, device=dev, seed=case.seed), case, dev)


def gpu_reg(case, dev):
    """A TabularMLPRegressor carrying the case's weights and non-zero biases"""
    from unionml_amd.ops.tabular import TabularMLPRegressor

    inf, hid, T = case.shape
    return _carry(TabularMLPRegressor(inf, hid, T, device=dev, seed=case.seed), case, dev)


def run_eval(ext, dev, model, Xbf, tgt, rt, *, cap=2, slot=0, extra=3):
    """One evaluation through the binding into oversized NaN-poisoned
    buffers: part has ``extra`` rows and 3 columns too many, hist ``cap``
    rows and 3 columns too many. Returns (record, part rows written, slot
    after) on the CPU after checking that nothing else was touched."""
    g = model.g
    reg = g.head == ref.HEAD_REGRESSION
    rec = ext.eval_rec_reg_n(g.cpad) if reg else ext.EVAL_REC_CLS_N
    assert ext.eval_rows_per_wg(g.hid, g.cpad) == rt
    n_wg = (Xbf.shape[0] + rt - 1) // rt
    part = torch.full((n_wg + extra, rec + 3), NAN, device=dev)
    hist = torch.full((cap, rec + 3), NAN, device=dev)
    slot_t = torch.tensor([slot], dtype=torch.int32, device=dev)
    fn = ext.mlp_eval_reg_gen if reg else ext.mlp_eval_gen
    fn(Xbf.to(dev), tgt.to(dev), g.hid, g.classes, model.wimg, model.master, part, hist, slot_t)
    torch.cuda.synchronize()
    part, hist = part.cpu(), hist.cpu()
    at = min(slot, cap - 1)
    assert torch.isfinite(part[:n_wg, :rec]).all(), "a workgroup's partial row is incomplete"
    assert torch.isnan(part[n_wg:]).all() and torch.isnan(part[:, rec:]).all()
    assert torch.isnan(hist[:at]).all() and torch.isnan(hist[at + 1:]).all()
    assert torch.isnan(hist[at, rec:]).all()
    assert int(slot_t.item()) == slot + 1
    return hist[at, :rec].clone(), part[:n_wg, :rec].clone()


def finish_of(part, B, count_at=None):
    """eval_finish_kernel on the host: rows added in index order in fp64,
    divided by B, rounded once"""
    s = torch.zeros(part.shape[1], dtype=F64)
    for w in range(part.shape[0]):
        s = s + part[w].to(F64)
    out = (s / B).float()
    if count_at is not None:
        out.view(torch.int32)[count_at] = int(s[count_at])
    return out


def correct_of(rec) -> int:
    return int(rec.view(torch.int32)[ref.EVAL_REC_CORRECT])


# ---------------------------------------------------------------------------
# classifier head
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cid,inst,shape,B,seed", CLS, ids=[c[0] for c in CLS])
def test_eval_vs_oracle(ext, dev, cid, inst, shape, B, seed):
    case = o64.make_case(shape, B, seed)
    clf = gpu_clf(case, dev)
    rec, part = run_eval(ext, dev, clf, case.Xbf, case.y, inst[1])
    o = o64e.eval64_cls(case)

    bound = o64.loss_bound(o.H, case.W2bf, case.g, case.invB)
    dloss = abs(float(rec[ref.EVAL_REC_LOSS]) - o.loss)
    print(f"RATIO evalloss {cid}: |dloss|={dloss:.3e} bound={bound:.3e} "
          f"dloss/bound={dloss / bound:.3f}")
    assert dloss <= bound, f"{cid}: loss off by {dloss:.3e} > {bound:.3e}"

    lo, hi, share = o64e.count_window(case, o)
    assert share <= o64e.MAX_SLACK_SHARE
    assert lo <= correct_of(rec) <= hi, f"{cid}: count {correct_of(rec)} outside [{lo}, {hi}]"
    # fixed-order fp64 finish, bit for bit
    assert torch.equal(rec.view(torch.int32),
                       finish_of(part, B, ref.EVAL_REC_CORRECT).view(torch.int32))
    # the counts are whole numbers of rows
    assert torch.equal(part[:, 1], part[:, 1].round()) and float(part[:, 1].max()) <= inst[1]


@pytest.mark.parametrize("cid,inst,shape,B,seed", CLS, ids=[c[0] for c in CLS])
def test_correct_count_is_predicts(ext, dev, cid, inst, shape, B, seed):
    """Staging reproduces predict's on-load standardization bit for bit and
    the evaluation keeps predict's accumulation order: equality."""
    case = o64.make_case(shape, B, seed)
    clf = gpu_clf(case, dev)
    g = clf.g
    ext.standardize_fit(case.Xfit.to(dev), clf.mean, clf.invstd, 1e-5)
    X = case.X.to(dev)
    preds = torch.empty(B, dtype=torch.int32, device=dev)
    ext.mlp_predict_gen(X, g.inp, g.hid, g.classes, clf.mean, clf.invstd, clf.wimg,
                        clf.master, preds, None)
    rec, _ = run_eval(ext, dev, clf, clf.stage(X), case.y, inst[1])
    assert correct_of(rec) == int((preds.cpu() == case.y).sum())


@pytest.mark.parametrize("inst,shape", o64.PRED_INSTANTIATIONS,
                         ids=[o64.inst_id(i) for i, _ in o64.PRED_INSTANTIATIONS])
def test_eval_masks_labels_and_tail(ext, dev, inst, shape):
    """Out-of-range labels (-1, and == classes where the head has a pad
    column) and tail rows contribute exact zeros: the record's sums equal
    those of the scored rows alone, workgroup by workgroup."""
    rt = inst[1]
    B = rt + 21
    case = o64.make_case(shape, B, 3)
    clf = gpu_clf(case, dev)
    y = case.y.clone()
    y[::3] = -1
    y[1::3] = case.g.classes
    rec, part = run_eval(ext, dev, clf, case.Xbf, y, rt)
    keep = torch.arange(B) % 3 == 2
    # a label == classes is masked exactly as a negative one
    allbad = y.clone()
    allbad[~keep] = -1
    rec2, part2 = run_eval(ext, dev, clf, case.Xbf, allbad, rt)
    assert torch.equal(part, part2)
    # the loss is the scored rows' alone, within the step's bound on them
    o = o64e.eval64_cls(case)
    logp = o.logits - torch.logsumexp(o.logits, dim=1, keepdim=True)
    want = float(-logp[torch.arange(B), case.y.long()][keep].sum() / B)
    bound = o64.loss_bound(o.H[keep], case.W2bf, case.g, 1.0 / B)
    assert abs(float(rec[ref.EVAL_REC_LOSS]) - want) <= bound
    lo = int((o.hits & keep & o64.clear_rows(o.logits, o.H, case.W2bf, case.g)).sum())
    assert lo <= correct_of(rec) <= int(keep.sum())
    # every label out of range: exact zeros
    rec0, part0 = run_eval(ext, dev, clf, case.Xbf, torch.full((B,), -1, dtype=torch.int32), rt)
    assert (part0 == 0).all() and (rec0.view(torch.int32) == 0).all()


# ---------------------------------------------------------------------------
# regression head
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cid,inst,shape,B,seed", REG, ids=[c[0] for c in REG])
def test_eval_reg_vs_oracle(ext, dev, cid, inst, shape, B, seed):
    case = o64r.make_case_reg(shape, B, seed)
    reg = gpu_reg(case, dev)
    g, T = case.g, case.g.classes
    # pad columns of the targets poisoned: they must leak nothing
    Yt = case.Yt.clone()
    Yt[:, T:] = 1e30
    rec, part = run_eval(ext, dev, reg, case.Xbf, Yt, inst[1])
    r = o64e.eval64_reg(case)

    bound = o64r.loss_bound_reg(r.H, r.z, case.Yt, case.W2bf, g, case.invB, r.loss)
    dloss = abs(float(rec[ref.EVAL_REC_LOSS]) - r.loss)
    print(f"RATIO evalregloss {cid}: |dloss|={dloss:.3e} bound={bound:.3e} "
          f"dloss/bound={dloss / bound:.3f}")
    assert dloss <= bound, f"{cid}: loss off by {dloss:.3e} > {bound:.3e}"

    mse_k = rec[ref.EVAL_REC_FIRST_MSE:]
    assert (mse_k[T:] == 0).all() and (part[:, 1 + T:] == 0).all(), "pad column leaked"
    mirror = ref.mlp_eval_reg_g(g, case.Xbf, case.Yt, case.W1bf, case.W2bf, case.master)
    mse_r = mirror[ref.EVAL_REC_FIRST_MSE:][:T]
    e_k, e_r = o64.e(mse_k[:T], r.mse), o64.e(mse_r, r.mse)
    emax_k, emax_r = o64.emax(mse_k[:T], r.mse), o64.emax(mse_r, r.mse)
    print(f"RATIO evalmse {cid}: e_k={e_k:.3e} e_r={e_r:.3e} emax_k={emax_k:.3e} "
          f"emax_r={emax_r:.3e}")
    assert e_k <= max(2 * e_r, o64.BF16_ULP)
    assert emax_k <= max(2 * emax_r, o64.BF16_ULP)
    assert torch.equal(rec, finish_of(part, B))


@pytest.mark.parametrize("inst,shape", o64r.PRED_INSTANTIATIONS,
                         ids=[o64.inst_id(i) for i, _ in o64r.PRED_INSTANTIATIONS])
def test_eval_reg_tail_rows_are_exact_zeros(ext, dev, inst, shape):
    """B = RT + 1: the second workgroup holds one row. Its sums are that
    row's alone, and equal the sums of a launch on that row only."""
    rt = inst[1]
    case = o64r.make_case_reg(shape, rt + 1, 3)
    reg = gpu_reg(case, dev)
    _, part = run_eval(ext, dev, reg, case.Xbf, case.Yt, rt)
    _, one = run_eval(ext, dev, reg, case.Xbf[rt:], case.Yt[rt:], rt)
    assert torch.equal(part[1], one[0])


PROBES = [(f"{o64.inst_id(inst)}-B{B}", inst, B) for inst, _ in o64r.PRED_INSTANTIATIONS
          for B in op.batches(inst)]


@pytest.mark.parametrize("cid,inst,B", PROBES, ids=[c[0] for c in PROBES])
def test_eval_reg_tile_order(ext, dev, cid, inst, B):
    """order_probe's "loss" inputs: one row per tile carries d = 2^13 in
    tile 0 and d = 2 in the others, in the last real column. The per-tile
    partials are exactly 2^25, 2, 2, ... (loss) and 2^26, 4, 4, ...
    (column), and only tile 0 first, left to right, sums them back to the
    first partial: 2^25 + 2 and 2^26 + 4 are ties that round to even."""
    probe = op.make_probe(inst, B, "loss")
    reg = gpu_reg(probe, dev)
    T = probe.g.classes
    _, part = run_eval(ext, dev, reg, probe.Xbf, probe.Yt, inst[1])
    want_loss = op.sum_in_order(probe.part_loss.transpose(0, 1))
    sq = (op.sum_in_order((2.0 * probe.part_loss).transpose(0, 1)))
    assert torch.equal(part[:, ref.EVAL_REC_LOSS], want_loss)
    assert torch.equal(part[:, ref.EVAL_REC_FIRST_MSE + T - 1], sq)
    others = torch.ones(part.shape[1], dtype=torch.bool)
    others[[ref.EVAL_REC_LOSS, ref.EVAL_REC_FIRST_MSE + T - 1]] = False
    assert (part[:, others] == 0).all()
    if probe.n_tiles > 2:
        # the probe discriminates: the reversed order gives another number
        rev = op.sum_in_order(probe.part_loss.transpose(0, 1),
                              order=range(probe.n_tiles - 1, -1, -1))
        assert not torch.equal(rev[:1], want_loss[:1])


# ---------------------------------------------------------------------------
# determinism, slot
# ---------------------------------------------------------------------------


def test_repeated_launches_are_bit_equal(ext, dev):
    for head_cases, make, model_of in ((o64.PRED_INSTANTIATIONS, o64.make_case, gpu_clf),
                                       (o64r.PRED_INSTANTIATIONS, o64r.make_case_reg, gpu_reg)):
        for inst, shape in head_cases:
            B = 2 * inst[1] + 17
            case = make(shape, B, 5)
            model = model_of(case, dev)
            tgt = case.Yt if hasattr(case, "Yt") else case.y
            first = run_eval(ext, dev, model, case.Xbf, tgt, inst[1])
            for _ in range(4):
                again = run_eval(ext, dev, model, case.Xbf, tgt, inst[1])
                assert torch.equal(first[0].view(torch.int32), again[0].view(torch.int32))
                assert torch.equal(first[1], again[1])


def test_slot_advances_and_saturates(ext, dev):
    case = o64.make_case((70, 50, 7), 150, 5)
    clf = gpu_clf(case, dev)
    g = clf.g
    Xbf = case.Xbf.to(dev)
    n = [150, 40, 129, 7]
    part = torch.zeros(2, 2, device=dev)
    hist = torch.full((3, 2), NAN, device=dev)
    slot = torch.zeros(1, dtype=torch.int32, device=dev)
    want = []
    for i, rows in enumerate(n):
        if i == 3:
            before = hist.clone()
        ext.mlp_eval_gen(Xbf[:rows], case.y[:rows].to(dev), g.hid, g.classes, clf.wimg,
                         clf.master, part, hist, slot)
        want.append(run_eval(ext, dev, clf, case.Xbf[:rows], case.y[:rows], 128)[0])
        if i == 2:
            assert int(slot.item()) == 3
            assert torch.equal(hist.cpu().view(torch.int32),
                               torch.stack(want).view(torch.int32))
    # the fourth pass, cap = 3: only row 2 is overwritten
    assert int(slot.item()) == 4
    assert torch.equal(hist[:2], before[:2])
    assert torch.equal(hist[2].cpu().view(torch.int32), want[3].view(torch.int32))
