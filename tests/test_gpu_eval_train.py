"""Validation inside training, end to end on the GPU, at the smallest
shapes that still cross a workgroup and a tail: 20x32x2 (generalized
kernels throughout) and 64x32x10 (the digits path: specialized training,
generalized evaluation). N = 300, batch 128, 3 epochs, 77 validation rows."""

import numpy as np
import pandas as pd
import pytest
import torch

from unionml_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SHAPES = [(20, 32, 2), (64, 32, 10)]
N, NV, BATCH, EPOCHS, LR = 300, 77, 128, 3, 5e-3
STATE = ("master", "bfmirror", "m", "v", "t_dev")


@pytest.fixture(scope="module")
def dev():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    hip_ext(required=True)
    return torch.device("cuda:0")


def shape_id(shape):
    return "x".join(map(str, shape))


def data(shape, seed=3):
    gen = torch.Generator().manual_seed(seed)
    inf, _, cls = shape
    y = torch.randint(0, cls, (N + NV,), generator=gen, dtype=torch.int32)
    centers = torch.randn(cls, inf, generator=gen) * 2.0
    return centers[y.long()] + torch.randn(N + NV, inf, generator=gen), y


def setup(shape, dev):
    """(model, staged train X, y, staged validation X, y), identically
    seeded on every call"""
    from unionml_amd.ops.tabular import TabularMLP

    X, y = data(shape)
    clf = TabularMLP(*shape, device=dev, seed=2)
    clf.fit_standardizer(X[:N].to(dev))
    return (clf, clf.stage(X[:N].to(dev)), y[:N].to(dev), clf.stage(X[N:].to(dev)),
            y[N:].to(dev))


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_graph_history_equals_eager_and_evaluate_by_hand(dev, shape):
    clf, Xbf, y, Xv, yv = setup(shape, dev)
    loss = clf.train_epochs(Xbf, y, epochs=EPOCHS, batch_size=BATCH, lr=LR,
                            validation=(Xv, yv))
    assert clf._graph is not None, "the epoch with its validation pass was not captured"
    assert clf.val_history.shape == (EPOCHS, ref.EVAL_REC_CLS_N)

    eager, *_ = setup(shape, dev)
    eager.train_epochs(Xbf, y, epochs=EPOCHS, batch_size=BATCH, lr=LR, use_graph=False,
                       validation=(Xv, yv))
    assert torch.equal(bits(clf.val_history), bits(eager.val_history))

    hand, *_ = setup(shape, dev)
    by_hand, last = [], None
    for _ in range(EPOCHS):
        last = hand.train_epochs(Xbf, y, epochs=1, batch_size=BATCH, lr=LR)
        by_hand.append(hand.evaluate(Xv, yv))
    assert clf.val_metrics() == by_hand
    assert loss == last
    # validation only reads: training is bit-equal to training without it
    for name in STATE:
        assert torch.equal(getattr(clf, name), getattr(hand, name)), name

    # two identically seeded runs are bit-equal
    again, *_ = setup(shape, dev)
    again.train_epochs(Xbf, y, epochs=EPOCHS, batch_size=BATCH, lr=LR, validation=(Xv, yv))
    assert torch.equal(bits(clf.val_history), bits(again.val_history))
    # accuracy is predict's, on the held-out rows
    X, yy = data(shape)
    acc = float((clf.predict(X[N:].to(dev)).cpu() == yy[N:]).double().mean())
    assert clf.val_metrics()[-1]["accuracy"] == acc


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_patience_and_restore_best_on_the_device_path(dev, shape):
    clf, Xbf, y, Xv, yv = setup(shape, dev)
    clf.train_epochs(Xbf, y, epochs=8, batch_size=BATCH, lr=0.3, validation=(Xv, yv))
    losses = [m["loss"] for m in clf.val_metrics()]
    best, bad, stop, best_e = float("inf"), 0, 8, 0
    for e, v in enumerate(losses):
        if v < best:
            best, bad, best_e = v, 0, e
        else:
            bad += 1
            if bad >= 2:
                stop = e + 1
                break

    twin, *_ = setup(shape, dev)
    twin.train_epochs(Xbf, y, epochs=8, batch_size=BATCH, lr=0.3, validation=(Xv, yv),
                      patience=2, restore_best=True)
    assert [m["loss"] for m in twin.val_metrics()] == losses[:stop]
    snap, *_ = setup(shape, dev)
    snap.train_epochs(Xbf, y, epochs=best_e + 1, batch_size=BATCH, lr=0.3)
    for name in STATE:
        assert torch.equal(getattr(twin, name), getattr(snap, name)), name
    assert torch.equal(twin.wimg, snap.wimg)
    assert twin.evaluate(Xv, yv)["loss"] == losses[best_e]


class Recorder:
    """The extension with every call's name recorded"""

    def __init__(self, ext):
        self._ext, self.calls = ext, []

    def __getattr__(self, name):
        attr = getattr(self._ext, name)
        if not callable(attr):
            return attr

        def wrapped(*a, **k):
            self.calls.append(name)
            return attr(*a, **k)

        return wrapped


@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_no_validation_means_todays_launches_and_graph_key(dev, shape, monkeypatch):
    from unionml_amd.ops import hip_ext, tabular

    clf, Xbf, y, Xv, yv = setup(shape, dev)
    rec = Recorder(hip_ext())
    monkeypatch.setattr(tabular, "hip_ext", lambda required=None: rec)
    clf.train_epochs(Xbf, y, epochs=2, batch_size=BATCH, lr=LR, use_graph=False)
    step = (["mlp_step_fused"] if clf.use_spec else ["mlp_step_gen", "reduce_adam_gen"])
    assert rec.calls == step * 3 * 2          # three batches, two epochs, nothing else
    batches = ((0, 128), (128, 128), (256, 44))
    clf.train_epochs(Xbf, y, epochs=2, batch_size=BATCH, lr=LR)
    assert clf._graph_key == ("fused", batches, LR, Xbf.data_ptr(), y.data_ptr())

    rec.calls.clear()
    clf.train_epochs(Xbf, y, epochs=1, batch_size=BATCH, lr=LR, use_graph=False,
                     validation=(Xv, yv))
    # (sizing the partial rows asks the extension for the rows per workgroup)
    launches = [c for c in rec.calls if c != "eval_rows_per_wg"]
    assert launches == step * 3 + ["mlp_eval_gen"]
    clf.train_epochs(Xbf, y, epochs=2, batch_size=BATCH, lr=LR, validation=(Xv, yv))
    assert clf._graph_key[:5] == ("fused", batches, LR, Xbf.data_ptr(), y.data_ptr())
    assert clf._graph_key[5:9] == ("val", Xv.data_ptr(), yv.data_ptr(), NV)


def test_regressor_validation_on_the_device(dev):
    from unionml_amd.ops.tabular import TabularMLPRegressor

    gen = torch.Generator().manual_seed(5)
    X = torch.randn(N + NV, 20, generator=gen)
    Y = torch.tanh(X[:, :3] @ torch.randn(3, 2, generator=gen)) * torch.tensor([50.0, 2.0]) \
        + torch.tensor([150.0, 0.0])

    def make():
        reg = TabularMLPRegressor(20, 32, 2, device=dev, seed=2)
        reg.fit_standardizer(X[:N].to(dev))
        reg.fit_target_standardizer(Y[:N].to(dev))
        return reg

    reg = make()
    tr = (reg.stage(X[:N].to(dev)), reg.stage_targets(Y[:N]))
    va = (reg.stage(X[N:].to(dev)), reg.stage_targets(Y[N:]))
    reg.train_epochs(*tr, epochs=EPOCHS, batch_size=BATCH, lr=LR, validation=va)
    hand = make()
    for e in range(EPOCHS):
        hand.train_epochs(*tr, epochs=1, batch_size=BATCH, lr=LR)
        m = hand.evaluate(*va)
        got = reg.val_metrics()[e]
        assert (got["loss"], got["mse"]) == (m["loss"], m["mse"])
    # R^2 against the formula the app's evaluator used
    preds = reg.predict(X[N:].to(dev)).cpu().double().numpy()
    yy = Y[N:].double().numpy()
    r2 = 1.0 - ((yy - preds) ** 2).sum(axis=0) / ((yy - yy.mean(axis=0)) ** 2).sum(axis=0)
    assert np.abs(np.asarray(m["r2"]) - r2).max() <= 1e-6


def test_app_evaluators_return_what_predict_plus_numpy_returned(dev):
    from unionml_amd.models import mlp, mlp_regress
    from unionml_amd.ops.tabular import TabularMLPRegressor

    clf, Xbf, y, _, _ = setup((64, 32, 10), dev)
    clf.train_epochs(Xbf, y, epochs=2, batch_size=BATCH, lr=LR)
    X, yy = data((64, 32, 10))
    feats = pd.DataFrame(X.numpy(), columns=mlp.FEATURES)
    target = pd.DataFrame({"target": yy.numpy()})
    old = float((np.asarray(mlp.predictor(clf, feats)) == target.squeeze().to_numpy()).mean())
    assert mlp.evaluator(clf, feats, target) == old

    frame = mlp_regress.reader(n=N, synthetic=True)
    feats, target = frame[mlp_regress.FEATURES], frame[["target"]]
    reg = mlp_regress.trainer(TabularMLPRegressor(10, 32, 1, device=dev, seed=1), feats, target,
                              epochs=5)
    preds = np.asarray(mlp_regress.predictor(reg, feats), dtype=np.float64)
    t = target.to_numpy().astype(np.float64).reshape(-1)
    old = 1.0 - float(((t - preds) ** 2).sum()) / float(((t - t.mean()) ** 2).sum())
    assert mlp_regress.evaluator(reg, feats, target) == pytest.approx(old, abs=1e-6)
