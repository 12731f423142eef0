"""The generalized step kernel (mlp_step_gen_kernel) sums db1, db2 and the
loss over a workgroup's 16-row tiles in a documented order: tile 0 first,
left to right, ((p0 + p1) + p2) + ... . The first test here knows the answer:
on the order-probe inputs (tests/order_probe.py, whose construction
tests/test_order_probe_cpu.py checks) every tile partial is an exactly known
fp32 number and the fp32 sum depends on the order, so the slab entries are
compared bit for bit with the host's sum in the documented order. The other
tests compare runs with each other, which cannot prove a fixed order but is
the guard where no exact probe exists (the classifier head)."""

import pytest
import torch

import oracle64 as o64
import oracle64_reg as o64r
import order_probe as op

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


def carrying(case, dev, cls):
    """A TabularMLP / TabularMLPRegressor carrying the case's weights"""
    model = cls(*case.shape, device=dev, seed=case.seed)
    model.master.copy_(case.master.to(dev))
    model.bfmirror.copy_(model.master.bfloat16())
    model._build_wimg()
    assert torch.equal(model.bfmirror.cpu(), case.bfmirror)
    return model


# ---------------------------------------------------------------------------
# the documented order, bit for bit
# ---------------------------------------------------------------------------

PROBES = op.cases()


@pytest.mark.parametrize("kind", ["bias", "loss"])
@pytest.mark.parametrize("cid,inst,B", PROBES, ids=[c[0] for c in PROBES])
def test_tile_sums_follow_the_documented_order(ext, dev, cid, inst, B, kind):
    """Each workgroup's slab entries for db1, db2 and (on the loss probe) the
    loss, read straight from NaN-prefilled slabs, equal the fp32 sum of the
    designed tile partials taken tile 0 first, left to right. Pad entries
    and all-tail tiles add exact zeros. On the loss probe every other sum of
    the step is exact in any order, so the rest of the slab must equal the
    fp64 oracle's; on the bias probe dW1 and dW2 add +-2^24 and 1 inside an
    MFMA, whose internal order is not specified: finite, pads zero.

    The RT = 32 cases sum two tiles: fp32 addition commutes, so they cannot
    tell one order from another and are here for coverage only."""
    from unionml_amd.ops.tabular import TabularMLPRegressor

    case = op.make_probe(inst, B, kind)
    g = case.g
    reg = carrying(case, dev, TabularMLPRegressor)
    slabs = torch.full((case.n_wg, g.slab_stride), float("nan"), device=dev)
    assert ext.mlp_step_reg_gen(case.Xbf.to(dev), case.Yt.to(dev), g.hid, g.classes,
                                case.rt, reg.wimg, reg.master, slabs, 1.0)
    torch.cuda.synchronize()
    slabs = slabs.cpu()

    pads = o64.pad_mask(g)
    for w in range(case.n_wg):
        slab = slabs[w]
        assert torch.isfinite(slab[: g.nparam + 1]).all(), "unwritten or non-finite entries"
        assert (slab[: g.nparam][pads] == 0).all(), "padded parameter leaked gradient"
        want_b1 = op.sum_in_order(case.part_b1[w])
        want_b2 = op.sum_in_order(case.part_b2[w])
        got_b1 = slab[g.off_b1 : g.off_b1 + g.hid]
        got_b2 = slab[g.off_b2 : g.off_b2 + g.cpad]
        assert torch.equal(got_b2, want_b2), f"wg {w} db2: {got_b2} != {want_b2}"
        assert torch.equal(got_b1, want_b1), f"wg {w} db1: {got_b1} != {want_b1}"
        if kind == "loss":
            want_loss = op.sum_in_order(case.part_loss[w])
            assert slab[g.nparam] == want_loss, f"wg {w} loss: {slab[g.nparam]} != {want_loss}"
            oracle = op.oracle_rows(case, op.rows_of(case, w))[: g.nparam]
            assert torch.equal(slab[: g.nparam].double(), oracle), f"wg {w}: slab != oracle"


# ---------------------------------------------------------------------------
# run-to-run bits: both heads, all 22 instantiations
# ---------------------------------------------------------------------------

RUNS = 5


def _repeat_step(ext, dev, model, launch, n_wg):
    """launch(slabs) + reduce-only into fresh NaN-filled buffers, RUNS times"""
    g = model.g
    counter = torch.zeros(1, dtype=torch.uint32, device=dev)
    loss_out = torch.zeros(1, device=dev)
    out = []
    for _ in range(RUNS):
        slabs = torch.full((n_wg, g.slab_stride), float("nan"), device=dev)
        grads = torch.full((g.nparam + 1,), float("nan"), device=dev)
        assert launch(slabs)
        ext.reduce_adam_gen(slabs, n_wg, g.inp, g.hid, g.cpad, model.master, model.bfmirror,
                            model.m, model.v, model.t_dev, counter, loss_out, LR, 0.9, 0.999,
                            EPS, wimg=model.wimg, grads_out=grads)
        out.append(grads)
    torch.cuda.synchronize()
    assert torch.isfinite(out[0]).all()
    for k in range(1, RUNS):
        assert torch.equal(out[0], out[k]), f"run {k} differs from run 0"


@pytest.mark.parametrize("head", ["classifier", "regression"])
@pytest.mark.parametrize("inst,shape", o64.STEP_INSTANTIATIONS,
                         ids=[o64.inst_id(i) for i, _ in o64.STEP_INSTANTIATIONS])
def test_step_bits_repeat(ext, dev, inst, shape, head):
    """The same step five times into fresh slabs gives the same gradient
    vector, loss included, at B = 2 RT + 17 (three workgroups, a ragged
    last one) on the oracle tests' geometries. Equal runs cannot prove that
    the sums are order-fixed (waves that arrive alike five times pass it
    too): test_tile_sums_follow_the_documented_order is the proof, for the
    regression head. This is the guard for the classifier head, where an
    exact probe cannot be built (the softmax outputs of equal logits are all
    of one magnitude); the accumulation lines are the same code for both."""
    from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor

    rt = inst[1]
    B = 2 * rt + 17
    n_wg = (B + rt - 1) // rt
    if head == "classifier":
        o64.check_instantiation(inst, shape)
        case = o64.make_case(shape, B, o64.case_seed(shape, B))
        clf = carrying(case, dev, TabularMLP)
        Xbf, y, g = case.Xbf.to(dev), case.y.to(dev), clf.g
        _repeat_step(ext, dev, clf, lambda slabs: ext.mlp_step_gen(
            Xbf, y, g.hid, g.classes, rt, clf.wimg, clf.master, slabs, case.invB), n_wg)
    else:
        shape = dict(o64r.STEP_INSTANTIATIONS)[inst]   # the class count read as T
        o64r.check_instantiation(inst, shape)
        case = o64r.make_case_reg(shape, B, o64r.case_seed(shape, B))
        reg = carrying(case, dev, TabularMLPRegressor)
        Xbf, Yt, g = case.Xbf.to(dev), case.Yt.to(dev), reg.g
        _repeat_step(ext, dev, reg, lambda slabs: ext.mlp_step_reg_gen(
            Xbf, Yt, g.hid, g.classes, rt, reg.wimg, reg.master, slabs, case.invB), n_wg)


# ---------------------------------------------------------------------------
# class level: the generalized twin of test_step_kernels_reproducible_bitwise
# ---------------------------------------------------------------------------

N_ROWS, EPOCHS, BATCH = 600, 3, 273   # batches of 273, 273 and 54 rows


@pytest.mark.parametrize("head", ["classifier", "regression"])
@pytest.mark.parametrize("outputs,rt", [(10, 64), (20, 128)], ids=["RT64", "RT128"])
def test_training_reproducible_bitwise(ext, dev, outputs, rt, head):
    """Two identically seeded hidden = 64 models trained alike end in the
    same bits: master, m, v, the step counter and the returned loss. At 600
    rows _rows_per_wg gives 64 rows per workgroup to every batch of a
    16-column head; 128 rows per workgroup are what the 32-column head
    always runs, so the second geometry has 20 outputs."""
    from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor

    inf = 40
    if head == "classifier":
        gen = torch.Generator().manual_seed(3)
        X = torch.randn(N_ROWS, inf, generator=gen) * torch.linspace(0.5, 2.0, inf) + 0.3
        T = torch.randint(0, outputs, (N_ROWS,), generator=gen, dtype=torch.int32)
    else:
        X, T = o64r.synth_reg(inf, outputs, N_ROWS, seed=3)

    def run():
        if head == "classifier":
            m = TabularMLP(in_features=inf, hidden=64, classes=outputs, device=dev, seed=8)
            m.fit_standardizer(X)
            targets = T.to(dev)
        else:
            m = TabularMLPRegressor(in_features=inf, hidden=64, targets=outputs, device=dev,
                                    seed=8)
            m.fit_standardizer(X)
            m.fit_target_standardizer(T)
            targets = m.stage_targets(T)
        assert not m.use_spec and m._rows_per_wg(BATCH) == rt
        loss = m.train_epochs(m.stage(X), targets, epochs=EPOCHS, batch_size=BATCH, lr=2e-3)
        torch.cuda.synchronize()
        return {"master": m.master.clone(), "m": m.m.clone(), "v": m.v.clone(),
                "t_dev": m.t_dev.clone(), "loss": torch.tensor(loss)}

    a, b = run(), run()
    assert int(a["t_dev"].item()) == EPOCHS * 3
    for k in a:
        assert torch.isfinite(a[k].float()).all(), k
        assert torch.equal(a[k], b[k]), f"{k}: not bit-identical"
