"""ForestPredictor on the CPU substrate: packing, rd32 and the sum order
against sklearn's own fp64 scores, bit for bit."""

import pickle

import numpy as np
import pytest
import scipy.sparse
from forest_fixtures import MODELS, fitted, probe_rows, raw_argmax_labels, sklearn_scores
from sklearn.ensemble import HistGradientBoostingClassifier, HistGradientBoostingRegressor

from unionml_amd.ops.forest import ForestPredictor, rd32, rows_per_wg


@pytest.mark.parametrize("name", sorted(MODELS))
def test_scores_equal_sklearn_bit_for_bit(name):
    est = fitted(name)
    forest = ForestPredictor.from_sklearn(est, device="cpu")
    X = probe_rows(forest, 300)
    want = sklearn_scores(est, X)
    got = forest.decision_function(X)
    assert got.dtype.is_floating_point and got.element_size() == 8
    assert np.array_equal(got.numpy(), want)
    if hasattr(est, "classes_"):
        assert np.array_equal(forest.predict(X), raw_argmax_labels(est, want))
    else:
        assert np.array_equal(forest.predict(X).numpy(), want[:, 0])
    assert forest.decision_function(X[:0]).shape == (0, want.shape[1])


def test_rd32_is_round_towards_minus_infinity():
    up = 1.0 + 0.75 * 2.0 ** -23        # nearest fp32 is 1 + 2^-23, above it
    down = 1.0 + 0.25 * 2.0 ** -23      # nearest fp32 is 1.0, below it
    got = rd32([up, down, np.inf, -np.inf, 1e300, -1e300, 0.5])
    fmax = np.finfo(np.float32).max
    assert got.dtype == np.float32
    assert got.tolist() == [1.0, 1.0, np.inf, -np.inf, fmax, -np.inf, 0.5]


def test_refusals():
    rng = np.random.RandomState(0)
    X = rng.randn(200, 3)
    category = rng.randint(0, 4, 200)
    cat = HistGradientBoostingRegressor(max_iter=2, categorical_features=[0]).fit(
        np.column_stack([category, X[:, 1:]]), np.array([3.0, -1.0, 2.0, 0.0])[category])
    with pytest.raises(ValueError, match="categorical"):
        ForestPredictor.from_sklearn(cat, device="cpu")
    many = HistGradientBoostingClassifier(max_iter=1).fit(X[:198], np.arange(198) % 33)
    with pytest.raises(ValueError, match="33"):
        ForestPredictor.from_sklearn(many, device="cpu")
    poisson = HistGradientBoostingRegressor(max_iter=3, loss="poisson").fit(X, X[:, 0] ** 2)
    forest = ForestPredictor.from_sklearn(poisson, device="cpu")
    with pytest.raises(ValueError, match="link"):
        forest.predict(X)
    assert np.array_equal(forest.decision_function(X).numpy()[:, 0],
                          poisson._raw_predict(X).ravel())
    with pytest.raises(ValueError, match="sparse"):
        forest.decision_function(scipy.sparse.csr_matrix(X))


def test_rows_per_wg_is_the_header_table():
    # the literals forest.h holds forest_rows_per_wg to
    assert [rows_per_wg(*fk) for fk in ((64, 10), (64, 32), (5, 1), (300, 3), (2048, 1),
                                        (2049, 1))] == [128, 64, 2048, 32, 4, 0]


@pytest.mark.parametrize("app", ["gbdt", "rforest"])
def test_cache_saved_under_the_apps_path_loads_empty(app):
    # what an artifact saved before the cache moved to ops/forest.py holds
    old = b"cunionml_amd.models." + app.encode() + b"\n_ForestCache\n)R."
    cache = pickle.loads(old)
    assert (cache.forest, cache.count) == (None, 0)
    assert pickle.loads(pickle.dumps(cache)).forest is None
