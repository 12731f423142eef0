"""Evaluation on the CPU: the fp64 oracle (tests/oracle64_eval.py) against
torch, the bf16-mirroring reference (ref.mlp_eval_g / mlp_eval_reg_g)
against the oracle on every geometry the GPU tests run, the conditions of
that case list, and the class-level API on the CPU path: evaluate,
evaluate_raw, train_epochs(validation=...), the apps' evaluators."""

import math
import re
from pathlib import Path

import numpy as np
import pandas as pd
import pytest
import torch

import oracle64 as o64
import oracle64_eval as o64e
import oracle64_reg as o64r
from oracle64 import F64
from unionml_amd.ops import reference as ref
from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor, split_validation

CLS = o64e.cls_cases()
REG = o64e.reg_cases()


def correct_of(rec) -> int:
    return int(rec.view(torch.int32)[ref.EVAL_REC_CORRECT])


def test_record_layout_matches_header():
    header = (Path(ref.__file__).parent / "hip" / "tabular_launch.h").read_text()
    got = dict(re.findall(r"constexpr int (EVAL_REC_\w+) = (\d+);", header))
    assert {k: int(v) for k, v in got.items()} == {
        "EVAL_REC_LOSS": ref.EVAL_REC_LOSS, "EVAL_REC_CORRECT": ref.EVAL_REC_CORRECT,
        "EVAL_REC_CLS_N": ref.EVAL_REC_CLS_N, "EVAL_REC_FIRST_MSE": ref.EVAL_REC_FIRST_MSE,
    }
    assert "return EVAL_REC_FIRST_MSE + cpad;" in header
    g = ref.Geometry(30, 256, 20, head=ref.HEAD_REGRESSION)
    assert ref.eval_rec_n(g) == 33 and ref.eval_rec_n(ref.Geometry(64, 32, 10)) == 2


def test_eval_kernels_follow_the_predict_rows():
    """tabular_eval.hip holds no instantiation list of its own, and the
    evaluation's rows per workgroup are the predict rows' RT."""
    src = (Path(ref.__file__).parent / "hip" / "tabular_eval.hip").read_text()
    assert re.findall(r"launch_eval_gen_t<([^>]*)>", src) == ["H, R, C, HEAD"]
    assert set(re.findall(r"mlp_eval_gen_kernel<([^>]*)>", src)) == {"HID, RT, CP, HEAD"}
    _, pred = o64.header_instantiations()
    for inst, shape in o64.PRED_INSTANTIATIONS:
        assert inst in pred
        assert ref.eval_rows_per_wg(ref.Geometry(*shape)) == inst[1]


# ---------------------------------------------------------------------------
# the oracle against torch
# ---------------------------------------------------------------------------


def test_oracle_matches_torch_losses():
    case = o64.make_case((70, 50, 7), 37, 3)
    o = o64e.eval64_cls(case)
    want = torch.nn.functional.cross_entropy(o.logits, case.y.long())
    assert abs(o.loss - float(want)) <= 1e-12
    assert o.correct == int((o.logits.argmax(1) == case.y.long()).sum())

    rcase = o64r.make_case_reg((100, 64, 26), 37, 3)
    r = o64e.eval64_reg(rcase)
    Y = rcase.Yt.to(F64)[:, :26]
    want = 0.5 * torch.nn.functional.mse_loss(r.z, Y, reduction="sum") / 37
    assert abs(r.loss - float(want)) <= 1e-12 * max(1.0, float(want))
    col = torch.nn.functional.mse_loss(r.z, Y, reduction="none").mean(dim=0)
    assert float((r.mse - col).abs().max()) <= 1e-12 * float(col.max())


# ---------------------------------------------------------------------------
# the mirror against the oracle, on the GPU tests' cases
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cid,inst,shape,B,seed", CLS, ids=[c[0] for c in CLS])
def test_ref_eval_vs_oracle(cid, inst, shape, B, seed):
    o64.check_instantiation(inst, shape)
    case = o64.make_case(shape, B, seed)
    o = o64e.eval64_cls(case)
    rec = ref.mlp_eval_g(case.g, case.Xbf, case.y, case.W1bf, case.W2bf, case.master)
    assert rec.shape == (ref.EVAL_REC_CLS_N,) and rec.dtype == torch.float32
    bound = o64.loss_bound(o.H, case.W2bf, case.g, case.invB)
    assert abs(float(rec[ref.EVAL_REC_LOSS]) - o.loss) <= bound
    lo, hi, share = o64e.count_window(case, o)
    # a condition of the case list: few rows inside the slack, so a wrong
    # count cannot hide there
    assert share <= o64e.MAX_SLACK_SHARE, f"{cid}: {share:.3f} of the rows inside the slack"
    assert lo <= correct_of(rec) <= hi


def column_bounds(case, r):
    """Per column, how far rounding H to bf16 can move the mean of (z-y)^2:
    |2 d e + e^2| with |e| <= delta_b (oracle64.logit_slack), mean over rows;
    plus the fp32 accumulation term of oracle64_reg.loss_bound_reg."""
    T = case.g.classes
    delta = o64.logit_slack(r.H, case.W2bf, case.g)[:, None]
    absd = (r.z - case.Yt.to(F64)[:, :T]).abs()
    return (2 * absd * delta + delta * delta).mean(dim=0) + 1e-5 * r.mse.clamp(min=1.0)


@pytest.mark.parametrize("cid,inst,shape,B,seed", REG, ids=[c[0] for c in REG])
def test_ref_eval_reg_vs_oracle(cid, inst, shape, B, seed):
    o64r.check_instantiation(inst, shape)
    case = o64r.make_case_reg(shape, B, seed)
    g, T = case.g, case.g.classes
    r = o64e.eval64_reg(case)
    rec = ref.mlp_eval_reg_g(g, case.Xbf, case.Yt, case.W1bf, case.W2bf, case.master)
    assert rec.shape == (ref.EVAL_REC_FIRST_MSE + g.cpad,)
    bound = o64r.loss_bound_reg(r.H, r.z, case.Yt, case.W2bf, g, case.invB, r.loss)
    assert abs(float(rec[ref.EVAL_REC_LOSS]) - r.loss) <= bound
    mse = rec[ref.EVAL_REC_FIRST_MSE:]
    assert (mse[T:] == 0).all(), "pad column leaked"
    assert ((mse[:T].double() - r.mse).abs() <= column_bounds(case, r)).all()
    # loss is half the sum of the column means
    assert float(rec[0]) == pytest.approx(0.5 * float(mse.double().sum()), rel=1e-6)


def test_ref_eval_masks_labels_and_pads():
    case = o64.make_case((70, 50, 7), 40, 3)
    full = ref.mlp_eval_g(case.g, case.Xbf, case.y, case.W1bf, case.W2bf, case.master)
    y = case.y.clone()
    y[::3] = -1
    y[1::3] = 7            # == classes: a pad column of the head
    keep = torch.arange(40) % 3 == 2
    rec = ref.mlp_eval_g(case.g, case.Xbf, y, case.W1bf, case.W2bf, case.master)
    sub = ref.mlp_eval_g(case.g, case.Xbf[keep], case.y[keep], case.W1bf, case.W2bf,
                         case.master)
    assert correct_of(rec) == correct_of(sub) <= correct_of(full)
    assert float(rec[0]) * 40 == pytest.approx(float(sub[0]) * int(keep.sum()), rel=1e-6)

    rcase = o64r.make_case_reg((70, 50, 7), 40, 3)
    clean = ref.mlp_eval_reg_g(rcase.g, rcase.Xbf, rcase.Yt, rcase.W1bf, rcase.W2bf,
                               rcase.master)
    Yt = rcase.Yt.clone()
    Yt[:, 7:] = 1e30
    dirty = ref.mlp_eval_reg_g(rcase.g, rcase.Xbf, Yt, rcase.W1bf, rcase.W2bf, rcase.master)
    assert torch.equal(clean, dirty)


# ---------------------------------------------------------------------------
# the class-level API on the CPU path
# ---------------------------------------------------------------------------


def blobs(n, inf, cls, seed):
    gen = torch.Generator().manual_seed(seed)
    y = torch.randint(0, cls, (n,), generator=gen, dtype=torch.int32)
    centers = torch.randn(cls, inf, generator=gen) * 2.0
    return centers[y.long()] + torch.randn(n, inf, generator=gen), y


def fitted_clf(shape=(20, 32, 3), n=300, seed=1, epochs=2):
    X, y = blobs(n, shape[0], shape[2], seed)
    clf = TabularMLP(*shape, device="cpu", seed=seed)
    clf.fit_standardizer(X)
    clf.train_epochs(clf.stage(X), y, epochs=epochs, batch_size=128, lr=5e-3)
    return clf, X, y


@pytest.mark.parametrize("shape", [(20, 32, 3), (64, 32, 10)], ids=o64.shape_id)
def test_evaluate_accuracy_is_predicts(shape):
    clf, X, y = fitted_clf(shape)
    m = clf.evaluate(clf.stage(X), y)
    assert m["n"] == 300
    assert m["accuracy"] == float((clf.predict(X).numpy() == y.numpy()).mean())
    assert 0.0 < m["accuracy"] < 1.0 or m["accuracy"] in (0.0, 1.0)
    assert m == clf.evaluate_raw(X, y)
    logits = o64.predict64(clf.g, X, clf.mean, clf.invstd, clf.W1bf, clf.W2bf, clf.master)[0]
    want = float(torch.nn.functional.cross_entropy(logits, y.long()))
    assert m["loss"] == pytest.approx(want, abs=5e-3)


def test_evaluate_empty_input():
    clf, X, y = fitted_clf()
    m = clf.evaluate(clf.stage(X[:0]), y[:0])
    assert m["n"] == 0 and math.isnan(m["loss"]) and math.isnan(m["accuracy"])
    assert clf.evaluate_raw(X[:0], y[:0])["n"] == 0
    reg = TabularMLPRegressor(10, 32, 2, device="cpu")
    m = reg.evaluate_raw(torch.zeros(0, 10), torch.zeros(0, 2))
    assert m["n"] == 0 and math.isnan(m["loss"]) and len(m["r2"]) == 2
    with pytest.raises(ValueError):
        clf.evaluate(clf.stage(X), y[:-1])
    with pytest.raises(ValueError):
        clf.evaluate(X, y)            # raw features where staged ones belong


def test_evaluate_ignores_out_of_range_labels():
    clf, X, y = fitted_clf()
    y2 = y.clone()
    y2[:50] = -1
    a, b = clf.evaluate_raw(X, y2), clf.evaluate_raw(X[50:], y[50:])
    assert a["accuracy"] * 300 == pytest.approx(b["accuracy"] * 250)
    assert a["loss"] * 300 == pytest.approx(b["loss"] * 250, rel=1e-6)


def reg_data(T, n, seed):
    """Targets whose offset is of the order of their spread (as the diabetes
    app's: mean ~150, spread ~50-77). The OLD evaluator squares residuals of
    fp32 predictions, each rounded to half an ulp of |y|; for that formula to
    define R^2 to 1e-6 at all, ulp(|y|) / spread must stay far below 1e-6,
    which oracle64_reg.synth_reg's first column (offset -50, spread 0.1)
    does not meet."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, 10, generator=g) * torch.linspace(0.5, 2.0, 10) + 0.3
    W = torch.randn(10, T, generator=g) / 10 ** 0.5
    scale = torch.tensor([50.0, 1.0, 10.0])[:T]
    offset = torch.tensor([150.0, 0.0, 5.0])[:T]
    return X, torch.tanh(X @ W) * scale + offset


def fitted_reg(T=3, n=300, seed=2, epochs=3):
    X, Y = reg_data(T, n, seed)
    reg = TabularMLPRegressor(10, 32, T, device="cpu", seed=seed)
    reg.fit_standardizer(X)
    reg.fit_target_standardizer(Y)
    reg.train_epochs(reg.stage(X), reg.stage_targets(Y), epochs=epochs, batch_size=128,
                     lr=5e-3)
    return reg, X, Y


def test_regressor_evaluate_matches_numpy_formula():
    reg, X, Y = fitted_reg()
    m = reg.evaluate_raw(X, Y)
    preds = reg.predict(X).double().numpy()
    y = Y.double().numpy()
    ss_res = ((y - preds) ** 2).sum(axis=0)
    ss_tot = ((y - y.mean(axis=0)) ** 2).sum(axis=0)
    assert np.abs(np.asarray(m["r2"]) - (1.0 - ss_res / ss_tot)).max() <= 1e-6
    assert np.asarray(m["mse"]) == pytest.approx(ss_res / 300, rel=1e-5)
    assert m["r2_mean"] == pytest.approx(float(np.mean(m["r2"])))
    assert m["mse_mean"] == pytest.approx(float(np.mean(m["mse"])))
    # poisoned pad columns of the staged targets leak nothing
    Yt = reg.stage_targets(Y)
    Yt[:, 3:] = 1e30
    assert reg.evaluate(reg.stage(X), Yt) == m


# -- train_epochs(validation=...) ---------------------------------------------


def val_setup(seed=4):
    X, y = blobs(377, 20, 3, seed)
    clf = TabularMLP(20, 32, 3, device="cpu", seed=seed)
    clf.fit_standardizer(X[:300])
    return clf, clf.stage(X[:300]), y[:300], clf.stage(X[300:]), y[300:]


def test_validation_records_one_per_epoch_and_match_evaluate():
    clf, Xbf, y, Xv, yv = val_setup()
    loss = clf.train_epochs(Xbf, y, epochs=3, batch_size=128, lr=5e-3, validation=(Xv, yv))
    assert clf.val_history.shape == (3, ref.EVAL_REC_CLS_N)

    twin, *_ = val_setup()
    by_hand, last = [], None
    for _ in range(3):
        last = twin.train_epochs(Xbf, y, epochs=1, batch_size=128, lr=5e-3)
        by_hand.append(twin.evaluate(Xv, yv))
    assert clf.val_metrics() == by_hand
    assert loss == last                      # the return value stays the training loss
    assert torch.equal(clf.master, twin.master)   # validation only reads


def test_patience_stops_where_the_recorded_losses_say():
    clf, Xbf, y, Xv, yv = val_setup()
    clf.train_epochs(Xbf, y, epochs=12, batch_size=128, lr=0.3, validation=(Xv, yv))
    losses = [m["loss"] for m in clf.val_metrics()]
    assert len(losses) == 12

    patience, min_delta = 2, 0.01
    best, bad, stop = float("inf"), 0, len(losses)
    for e, v in enumerate(losses):
        if v < best - min_delta:
            best, bad = v, 0
        else:
            bad += 1
            if bad >= patience:
                stop = e + 1
                break
    assert stop < 12, "the case must stop early to show anything"

    twin, *_ = val_setup()
    twin.train_epochs(Xbf, y, epochs=12, batch_size=128, lr=0.3, validation=(Xv, yv),
                      patience=patience, min_delta=min_delta)
    assert [m["loss"] for m in twin.val_metrics()] == losses[:stop]


def test_restore_best_restores_the_snapshot_epoch_bit_for_bit():
    clf, Xbf, y, Xv, yv = val_setup()
    clf.train_epochs(Xbf, y, epochs=8, batch_size=128, lr=0.3, validation=(Xv, yv),
                     restore_best=True)
    losses = [m["loss"] for m in clf.val_metrics()]
    best = int(np.argmin(losses))            # first minimum: later ties do not improve
    assert best < 7, "the case must restore an earlier epoch to show anything"

    twin, *_ = val_setup()
    twin.train_epochs(Xbf, y, epochs=best + 1, batch_size=128, lr=0.3)
    for name in ("master", "bfmirror", "m", "v", "t_dev"):
        assert torch.equal(getattr(clf, name), getattr(twin, name)), name
    assert clf.evaluate(Xv, yv)["loss"] == losses[best]


def test_validation_argument_errors():
    clf, Xbf, y, Xv, yv = val_setup()
    with pytest.raises(ValueError, match="data parallel"):
        clf.train_epochs(Xbf, y, epochs=1, validation=(Xv, yv), world_size=2)
    with pytest.raises(ValueError, match="persistent"):
        clf.train_epochs(Xbf, y, epochs=1, validation=(Xv, yv), engine="persistent")
    with pytest.raises(ValueError, match="validation"):
        clf.train_epochs(Xbf, y, epochs=1, patience=2)
    with pytest.raises(ValueError, match="validation"):
        clf.train_epochs(Xbf, y, epochs=1, restore_best=True)
    with pytest.raises(ValueError):
        clf.train_epochs(Xbf, y, epochs=1, validation=(Xv[:0], yv[:0]))
    assert clf.t_dev.item() == 0, "a refused call must not train"


def test_regressor_validation_history():
    X, Y = o64r.synth_reg(10, 2, 377, 6)
    reg = TabularMLPRegressor(10, 32, 2, device="cpu", seed=6)
    reg.fit_standardizer(X[:300])
    reg.fit_target_standardizer(Y[:300])
    Xv, Yv = reg.stage(X[300:]), reg.stage_targets(Y[300:])
    reg.train_epochs(reg.stage(X[:300]), reg.stage_targets(Y[:300]), epochs=3,
                     batch_size=128, lr=5e-3, validation=(Xv, Yv))
    assert reg.val_history.shape == (3, ref.EVAL_REC_FIRST_MSE + 16)
    last = reg.evaluate(Xv, Yv)
    got = reg.val_metrics()[-1]
    assert got["loss"] == last["loss"] and got["mse"] == last["mse"]


def test_split_validation():
    tr, va = split_validation(1797, 0.1)
    assert len(va) == 180 and len(tr) == 1617
    assert sorted(tr.tolist() + va.tolist()) == list(range(1797))
    assert torch.equal(va, split_validation(1797, 0.1)[1])
    with pytest.raises(ValueError):
        split_validation(10, 1.0)


# -- the apps ------------------------------------------------------------------


def test_app_evaluators_return_what_predict_plus_numpy_returned():
    from unionml_amd.models import mlp, mlp_regress

    clf, X, y = fitted_clf((64, 32, 10))
    feats = pd.DataFrame(X.numpy(), columns=mlp.FEATURES)
    target = pd.DataFrame({"target": y.numpy()})
    old = float((np.asarray(mlp.predictor(clf, feats)) == target.squeeze().to_numpy()).mean())
    assert mlp.evaluator(clf, feats, target) == old

    reg, Xr, Yr = fitted_reg(T=1)
    feats = pd.DataFrame(Xr.numpy(), columns=mlp_regress.FEATURES)
    target = pd.DataFrame({"target": Yr[:, 0].numpy()})
    preds = np.asarray(mlp_regress.predictor(reg, feats), dtype=np.float64)
    yy = target.to_numpy().astype(np.float64).reshape(-1)
    old = 1.0 - float(((yy - preds) ** 2).sum()) / float(((yy - yy.mean()) ** 2).sum())
    assert mlp_regress.evaluator(reg, feats, target) == pytest.approx(old, abs=1e-6)


def test_app_trainer_validation_kwargs():
    from unionml_amd.models import mlp

    X, y = blobs(200, 64, 10, 8)
    feats = pd.DataFrame(X.numpy(), columns=mlp.FEATURES)
    target = pd.DataFrame({"target": y.numpy()})
    clf = mlp.trainer(TabularMLP(device="cpu"), feats, target, epochs=4,
                      validation_fraction=0.25, patience=3, restore_best=True)
    assert 1 <= len(clf.val_history) <= 4 and clf._val_n == 50
    plain = mlp.trainer(TabularMLP(device="cpu"), feats, target, epochs=1)
    assert plain.val_history is None
