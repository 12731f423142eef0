"""BaggedForestPredictor on the CPU substrate: breadth-first packing, rd32
and the sum order against sklearn's own fp64 results, bit for bit."""

import pickle

import numpy as np
import pytest
import scipy.sparse
from bagged_fixtures import MODELS, fitted, probe_rows, sklearn_means
from sklearn.ensemble import RandomForestClassifier, RandomForestRegressor
from sklearn.tree import ExtraTreeRegressor

from unionml_amd.ops import forest as F


@pytest.mark.parametrize("name", sorted(MODELS))
def test_packed_walk_equals_sklearn_bit_for_bit(name):
    est = fitted(name)
    forest = F.from_sklearn(est, device="cpu")
    assert isinstance(forest, F.BaggedForestPredictor)
    trees = getattr(est, "estimators_", [est])
    assert (forest.n_trees, forest.n_features) == (len(trees), est.n_features_in_)
    assert forest.max_tree_nodes == max(t.tree_.node_count for t in trees)
    X = probe_rows(name, forest, 150)
    want = sklearn_means(est, X)
    finite = ~np.isinf(X).any(axis=1)
    if hasattr(est, "classes_"):
        assert np.array_equal(forest.predict_proba(X).numpy(), want)
        assert np.array_equal(forest.predict(X)[finite], est.predict(X[finite]))
    else:
        got = forest.predict(X)
        assert got.dtype.is_floating_point and got.element_size() == 8
        assert np.array_equal(got.numpy(), want[:, 0])
        with pytest.raises(ValueError, match="classifier"):
            forest.predict_proba(X)


def test_refusals_and_empty_batch():
    rng = np.random.RandomState(0)
    X = rng.randn(198, 3)
    many = RandomForestClassifier(n_estimators=2, random_state=0).fit(X, np.arange(198) % 33)
    with pytest.raises(ValueError, match="33"):
        F.from_sklearn(many, device="cpu")
    two = RandomForestRegressor(n_estimators=2, random_state=0).fit(X, X[:, :2])
    with pytest.raises(ValueError, match="2 outputs"):
        F.from_sklearn(two, device="cpu")
    with pytest.raises(TypeError):
        F.from_sklearn(object(), device="cpu")
    one = F.from_sklearn(ExtraTreeRegressor(random_state=0).fit(X, X[:, 0]), device="cpu")
    assert (one.n_trees, one.n_scores) == (1, 1)
    with pytest.raises(ValueError, match="sparse"):
        one.predict(scipy.sparse.csr_matrix(X))
    assert one.predict(X[:0]).shape == (0,)
    forest = F.from_sklearn(fitted("single_tree"), device="cpu")
    assert forest.predict_proba(np.zeros((0, 7), np.float32)).shape == (0, 3)
    assert forest.predict(np.zeros((0, 7), np.float32)).shape == (0,)


def test_rows_per_wg_is_the_header_table():
    # the literals bagged_forest.h holds bagged_rows_per_wg and
    # bagged_trees_per_chunk to
    assert [F.bagged_rows_per_wg(*fk) for fk in ((64, 10), (64, 32), (5, 2), (300, 3),
                                                 (2048, 1), (2049, 1), (4, 33))] == [
        128, 64, 256, 16, 4, 0, 0]
    assert [F.bagged_trees_per_chunk(*a) for a in ((1, 100, 0), (1, 1000, 0), (128, 100, 0),
                                                   (65, 100, 5), (256, 100, 0))] == [
        100, 256, 16, 5, 8]


def test_app_cache_pickles_empty():
    from unionml_amd.models import rforest

    clf = rforest.init({"n_estimators": 3})
    frame = rforest.reader(n=200)
    clf = rforest.trainer(clf, frame[rforest.FEATURES], frame[["target"]])
    forest = rforest.device_forest(clf)
    assert rforest.device_forest(clf) is forest and forest.n_trees == 3
    again = pickle.loads(pickle.dumps(clf))
    assert again._unionml_forest.forest is None
    assert np.array_equal(again.predict(frame[rforest.FEATURES]),
                          clf.predict(frame[rforest.FEATURES]))
