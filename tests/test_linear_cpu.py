"""unionml_amd.ops.linear without a GPU: the numpy fallback against the
longdouble reference and against sklearn, the refusals, the cache, the app."""

import pickle

import numpy as np
import pytest
import scipy.sparse

from linear_reference import fit_problem, fit_tolerance, objective_case, reference
from unionml_amd.ops.linear import (MAX_FEATURES, DeviceLogisticRegression, LinearPredictor,
                                    device_linear, objective_numpy)


@pytest.mark.parametrize("shape", [(131, 65, 17), (300, 5, 2)], ids=["multinomial", "binomial"])
def test_numpy_objective_within_the_derived_bound(shape):
    X, y, W, b, sw = objective_case(*shape)
    loss, gW, gb, bound = reference(X, y, W, b, sw, 0.37)
    got = objective_numpy(X.astype(np.float64), y, sw, W, b, float(sw.sum()), 0.37)
    assert abs(float(got[0] - loss)) <= bound.tol_loss
    assert (np.abs(got[1] - gW).astype(np.float64) <= bound.tol_gW).all()
    assert (np.abs(got[2] - gb).astype(np.float64) <= bound.tol_gb).all()


@pytest.mark.parametrize("binary", [False, True], ids=["300x7x3", "200x5x2"])
def test_numpy_fit_matches_sklearn(binary):
    X, y = fit_problem(binary)
    base, tol, _ = fit_tolerance(X, y)
    model = DeviceLogisticRegression(tol=1e-8, max_iter=1000, device="cpu").fit(X, y)
    assert np.abs(model.coef_ - base.coef_).max() <= tol
    assert np.abs(model.intercept_ - base.intercept_).max() <= tol
    est = model.to_sklearn()
    assert (est.predict(X.astype(np.float64)) == model.predict(X)).all()
    assert (est.classes_ == base.classes_).all() and est.n_features_in_ == X.shape[1]
    np.testing.assert_allclose(model.predict_proba(X).numpy(), base.predict_proba(X), atol=1e-9)


@pytest.mark.parametrize("refused", ["classes33", "one_class", "sparse", "l1", "l1_ratio",
                                     "features"])
def test_refusals(refused):
    rng = np.random.default_rng(0)
    X, y, params = rng.standard_normal((66, 3)).astype(np.float32), np.arange(66) % 3, {}
    if refused == "classes33":
        y = np.arange(66) % 33
    elif refused == "one_class":
        y = np.zeros(66, dtype=int)
    elif refused == "sparse":
        X = scipy.sparse.csr_matrix(X)
    elif refused == "l1":
        params = {"penalty": "l1"}
    elif refused == "l1_ratio":
        params = {"l1_ratio": 0.5}
    elif refused == "features":
        with pytest.raises(ValueError):
            LinearPredictor(np.broadcast_to(0.0, (1, MAX_FEATURES + 1)), None, [0, 1],
                            device="cpu")
        return
    with pytest.raises(ValueError):
        DeviceLogisticRegression(device="cpu", **params).fit(X, y)


def test_empty_batch_and_cache():
    X, y = fit_problem(False)
    est = DeviceLogisticRegression(device="cpu").fit(X, y).to_sklearn()
    predictor = device_linear(est)
    assert device_linear(est) is predictor
    assert predictor.predict_proba(X[:0]).shape == (0, 3)
    assert predictor.decision_function(X[:0]).shape == (0, 3) and len(predictor.predict(X[:0])) == 0
    assert (predictor.predict(X) == est.predict(X.astype(np.float64))).all()
    restored = pickle.loads(pickle.dumps(est))
    assert restored._unionml_linear.predictor is None       # pickles empty
    assert (restored.predict(X.astype(np.float64)) == est.predict(X.astype(np.float64))).all()


def test_logreg_app_trains_and_predicts():
    from sklearn.linear_model import LogisticRegression

    from unionml_amd.models import logreg

    logreg.model.artifact = None
    clf, metrics = logreg.model.train(trainer_kwargs={"max_iter": 200}, n=300)
    assert type(clf) is LogisticRegression and metrics["train"] > 0.9
    frame = logreg.reader(n=300)[logreg.FEATURES]
    assert logreg.model.predict(features=frame) == [int(c) for c in clf.predict(frame)]
