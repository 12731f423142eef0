"""CPU tests for TabularMLPRegressor (the class that runs the regression
HIP kernels on a GPU runs ops/reference.py's mlp_step_reg_g here: one code
path, two substrates) and for the packaged regression app."""

import pickle

import numpy as np
import pytest
import torch

import oracle64_reg as o64r
from oracle64_reg import synth_reg
from unionml_amd.ops import reference as ref
from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor


def r2(pred, Y):
    return 1.0 - ((pred - Y) ** 2).sum(dim=0) / ((Y - Y.mean(dim=0)) ** 2).sum(dim=0)


@pytest.mark.parametrize("shape", [(10, 32, 1), (100, 50, 7), (33, 250, 3), (64, 32, 26)],
                         ids=lambda s: "x".join(map(str, s)))
def test_cpu_train_predict(shape):
    inf, hid, T = shape
    reg = TabularMLPRegressor(in_features=inf, hidden=hid, targets=T, device="cpu", seed=0)
    assert reg.targets == T and reg.g.head == "regression" and not reg.use_spec
    X, Y = synth_reg(inf, T, 512, seed=1)
    reg.fit_standardizer(X)
    reg.fit_target_standardizer(Y)
    Xbf, Yt = reg.stage(X), reg.stage_targets(Y)
    assert Yt.shape == (512, reg.g.cpad) and Yt.dtype == torch.float32
    assert (Yt[:, T:] == 0).all(), "target staging must zero-pad"
    assert float(Yt[:, :T].mean(dim=0).abs().max()) < 1e-3
    assert float((Yt[:, :T].std(dim=0) - 1).abs().max()) < 1e-2
    first = reg.train_epochs(Xbf, Yt, epochs=1, batch_size=128, lr=5e-3)
    loss = reg.train_epochs(Xbf, Yt, epochs=30, batch_size=128, lr=5e-3)
    assert loss == loss and loss < first
    pred = reg.predict(X)
    assert pred.shape == (512, T) and pred.dtype == torch.float32
    # every target far better than the mean predictor (26 independent tanh
    # targets share 32 hidden units: capacity, not training, caps that shape)
    assert float(r2(pred, Y).min()) > 0.5, f"{shape}: R2 {r2(pred, Y)}, loss {loss}"
    # padded params stayed exactly zero through training
    W1, b1, W2, b2 = ref.unpack_master_g(reg.g, reg.master)
    assert (W1[inf:, :] == 0).all() and (W1[:, hid:] == 0).all()
    assert (W2[hid:, :] == 0).all() and (W2[:, T:] == 0).all()
    assert (b1[hid:] == 0).all() and (b2[T:] == 0).all()


def test_single_target_accepts_flat_y_and_identity_scaler():
    reg = TabularMLPRegressor(in_features=10, device="cpu")
    assert reg.g.classes == 1 and reg.g.hidden == 32
    X, Y = synth_reg(10, 1, 64, seed=2)
    # identity until fitted: staging is a plain zero-pad, predict returns z
    Yt = reg.stage_targets(Y[:, 0])
    assert torch.equal(Yt[:, 0], Y[:, 0]) and (Yt[:, 1:] == 0).all()
    assert torch.equal(reg.y_scale, torch.ones(1)) and torch.equal(reg.y_mean, torch.zeros(1))
    reg.fit_target_standardizer(Y[:, 0])
    assert torch.equal(reg.y_scale, 1.0 / reg.y_invstd)
    with pytest.raises(ValueError, match="targets"):
        reg.stage_targets(torch.zeros(4, 3))
    with pytest.raises(ValueError, match="stage_targets"):
        reg.train_epochs(reg.stage(X), Y, epochs=1)
    with pytest.raises(ValueError, match="persistent"):
        reg.train_epochs(reg.stage(X), reg.stage_targets(Y), epochs=1, engine="persistent")


def test_loss_is_half_mean_squared_error():
    """train_epochs returns the last step's loss before its update:
    0.5/B * sum (z - y)^2 in standardized units."""
    reg = TabularMLPRegressor(in_features=20, hidden=32, targets=3, device="cpu", seed=4)
    X, Y = synth_reg(20, 3, 96, seed=5)
    reg.fit_standardizer(X)
    reg.fit_target_standardizer(Y)
    Xbf, Yt = reg.stage(X), reg.stage_targets(Y)
    z = (reg.predict(X) - reg.y_mean) * reg.y_invstd
    want = 0.5 / 96 * float(((z - Yt[:, :3]) ** 2).sum())
    got = reg.train_epochs(Xbf, Yt, epochs=1, batch_size=96, lr=1e-3)
    assert abs(got - want) <= 1e-5 * max(1.0, want)


def test_checkpoint_resumes_training_exactly():
    """2+2 epochs through a state_dict roundtrip equals 4 straight epochs
    bit for bit, target scaler included."""
    X, Y = synth_reg(100, 7, 128, seed=11)

    def fresh(seed):
        return TabularMLPRegressor(in_features=100, hidden=50, targets=7, device="cpu", seed=seed)

    a = fresh(0)
    a.fit_standardizer(X)
    a.fit_target_standardizer(Y)
    a.train_epochs(a.stage(X), a.stage_targets(Y), epochs=4, batch_size=32, lr=1e-3)

    b = fresh(0)
    b.fit_standardizer(X)
    b.fit_target_standardizer(Y)
    b.train_epochs(b.stage(X), b.stage_targets(Y), epochs=2, batch_size=32, lr=1e-3)
    state = b.state_dict()

    c = fresh(99)
    c.load_state_dict(state)
    assert torch.equal(c.y_mean, b.y_mean) and torch.equal(c.y_scale, b.y_scale)
    c.train_epochs(c.stage(X), c.stage_targets(Y), epochs=2, batch_size=32, lr=1e-3)

    assert int(c.t_dev.item()) == int(a.t_dev.item()) == 16
    assert torch.equal(a.master, c.master), (a.master - c.master).abs().max()
    assert torch.equal(a.predict(X), c.predict(X))


def test_pickle_roundtrip():
    reg = TabularMLPRegressor(in_features=200, hidden=96, targets=5, device="cpu", seed=0)
    X, Y = synth_reg(200, 5, 32, seed=3)
    reg.fit_standardizer(X)
    reg.fit_target_standardizer(Y)
    clone = pickle.loads(pickle.dumps(reg))
    assert isinstance(clone, TabularMLPRegressor)
    assert clone.g == reg.g and clone.g.head == "regression"
    assert torch.equal(clone.y_mean, reg.y_mean) and torch.equal(clone.y_scale, reg.y_scale)
    assert torch.equal(clone.predict(X), reg.predict(X))


def test_head_mismatch_loads_raise_and_classifier_state_is_unchanged():
    clf = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=0)
    reg = TabularMLPRegressor(in_features=100, hidden=50, targets=7, device="cpu", seed=0)
    assert clf.g != reg.g
    cstate, rstate = clf.state_dict(), reg.state_dict()
    # the classifier's checkpoint format did not move
    assert list(cstate) == ["W1", "b1", "W2", "b2", "mean", "invstd", "geometry",
                            "adam_m", "adam_v", "adam_t"]
    assert set(rstate) - set(cstate) == {"head", "y_mean", "y_invstd"}
    with pytest.raises(ValueError, match="head"):
        reg.load_state_dict(cstate)
    with pytest.raises(ValueError, match="head"):
        clf.load_state_dict(rstate)
    # same head, other geometry: the existing guard
    other = TabularMLPRegressor(in_features=100, hidden=50, targets=6, device="cpu")
    with pytest.raises(ValueError, match="geometry"):
        other.load_state_dict(rstate)
    clf.load_state_dict(cstate)
    reg.load_state_dict(rstate)
    # a regression state without its target scaler names what is missing
    # (and loads nothing), like the other mismatches: no KeyError
    before = reg.master.clone()
    bare = {k: v for k, v in rstate.items() if k != "y_invstd"}
    bare["W1"] = bare["W1"] + 1.0
    with pytest.raises(ValueError, match="y_invstd"):
        reg.load_state_dict(bare)
    assert torch.equal(reg.master, before)


def test_graph_runner_cpu_passthrough():
    from unionml_amd.serving.graph_runner import TabularGraphRunner

    reg = TabularMLPRegressor(in_features=10, hidden=32, targets=2, device="cpu", seed=1)
    X, _ = synth_reg(10, 2, 70, seed=6)
    out = TabularGraphRunner(reg, max_batch_size=64)(X.numpy())
    assert out.shape == (70, 2) and out.dtype == np.float32
    assert np.array_equal(out, reg.predict(X).numpy())


# ---------------------------------------------------------------------------
# the packaged app
# ---------------------------------------------------------------------------


def test_app_reader():
    from unionml_amd.models.mlp_regress import FEATURES, reader

    frame = reader()
    assert frame.shape == (442, 11) and list(frame.columns) == FEATURES + ["target"]
    assert reader(n=50).shape == (50, 11)
    a, b = reader(n=300, synthetic=True), reader(n=300, synthetic=True)
    assert a.shape == (300, 11) and a.equals(b)
    assert not a.equals(reader(n=300, synthetic=True, seed=18))


def test_app_trains_and_margin_is_the_measured_one(tmp_path):
    """The app through Model.train on the CPU path for the five init
    seeds: held-out R^2 beats the mean predictor every time, and three
    times their spread is the margin the GPU test allows
    (oracle64_reg.APP_R2_MARGIN; the window covers last-bit differences
    between BLAS builds)."""
    from unionml_amd.models.mlp_regress import model

    scores = []
    for seed in o64r.APP_SEEDS:
        reg, metrics = o64r.train_app("cpu", seed)
        assert isinstance(reg, TabularMLPRegressor) and reg.g.in_features == 10
        assert metrics["test"] > 0.0 and metrics["train"] > metrics["test"]
        scores.append(metrics["test"])
    spread = max(scores) - min(scores)
    print("held-out R2 per seed:", ["%.4f" % s for s in scores], "spread %.4f" % spread)
    assert 0.75 * o64r.APP_R2_SPREAD <= spread <= 1.25 * o64r.APP_R2_SPREAD

    # predictor, saver and loader on the last artifact
    feats = [{f"x{i}": 0.01 * i for i in range(10)}, {f"x{i}": -0.02 for i in range(10)}]
    preds = model.predict(features=feats)
    assert len(preds) == 2 and all(isinstance(p, float) for p in preds)
    path = tmp_path / "reg.pt"
    model.save(path)
    loaded = model.load(path)
    assert isinstance(loaded, TabularMLPRegressor)
    assert model.predict(features=feats) == preds


def test_app_batched_serving_answers_like_predict():
    """The @graphed forward the DynamicBatcher and /predict with batch=True
    use must answer in the predictor's shape: one float per row, equal to
    Model.predict on the same features."""
    from fastapi import FastAPI
    from fastapi.testclient import TestClient

    from unionml_amd.models.mlp_regress import model

    o64r.train_app("cpu", 0)
    want = [model.predict(features=r) for r in o64r.APP_REQUESTS]
    assert [len(w) for w in want] == [1, 2, 1]
    assert all(isinstance(v, float) for w in want for v in w)
    assert o64r.batched_predict(model, o64r.APP_REQUESTS) == want

    app = FastAPI()
    model.serve(app, batch=True, max_delay_ms=1.0)
    with TestClient(app) as client:
        for r, w in zip(o64r.APP_REQUESTS, want):
            resp = client.post("/predict", json={"features": r})
            assert resp.status_code == 200, resp.text
            assert resp.json() == w


def test_app_synthetic_path():
    from unionml_amd.models.mlp_regress import model

    model.artifact = None
    _, metrics = model.train(hyperparameters={"device": "cpu"}, synthetic=True, n=1000)
    assert metrics["test"] > 0.8, metrics
