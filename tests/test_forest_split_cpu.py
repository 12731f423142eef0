"""The split packing of ForestPredictor on the CPU substrate: the host walk in
the sum kernel's order against sklearn's fp64 scores, bit for bit, and the
Python copies of the launcher rule."""

import numpy as np
import pytest
from forest_fixtures import fitted, probe_rows, sklearn_scores
from forest_split_fixtures import grown

from unionml_amd.ops import forest as F


def test_grown_regressor_is_served_by_the_split_walk():
    est, X, want = grown()
    assert max(len(t.nodes) for it in est._predictors for t in it) > F.CHUNK_NODES
    forest = F.ForestPredictor.from_sklearn(est, device="cpu")
    assert forest._nodes_np is None and forest._nodes is None
    assert forest.walk_for(len(X)) == forest.walk_for(10 ** 9) == "split"
    assert np.array_equal(forest.predict(X).numpy(), want)
    assert np.array_equal(forest.predict(X, walk="split").numpy(), want)
    with pytest.raises(ValueError, match="chunked"):
        forest.predict(X, walk="chunked")


@pytest.mark.parametrize("name", ["classes17", "deep"])
def test_split_scores_equal_sklearn_bit_for_bit(name):
    est = fitted(name)
    forest = F.ForestPredictor.from_sklearn(est, device="cpu")
    X = probe_rows(forest, 300)
    want = sklearn_scores(est, X)
    assert np.array_equal(forest.decision_function(X, walk="split").numpy(), want)
    assert np.array_equal(forest.decision_function(X, walk="chunked").numpy(), want)
    assert forest.walk_for(1) == ("split" if F.split_max_rows >= 1 else "chunked")
    assert forest.walk_for(1, trees_per_chunk=5) == "chunked"
    with pytest.raises(ValueError, match="walk"):
        forest.decision_function(X, walk="fused")


def test_launcher_rule_is_the_header_table():
    # the literals forest_split.h holds its two constexpr functions to
    assert [F.split_rows_per_wg(f) for f in (64, 5, 45, 300, 2048, 2049)] == [
        128, 256, 256, 32, 4, 0]
    assert [F.split_trees_per_slice(*a) for a in (
        (1, 1000, 0), (1, 100, 0), (3, 1000, 0), (64, 1000, 0), (128, 1000, 0), (256, 3, 0),
        (256, 1000, 0), (65, 100, 5))] == [256, 100, 256, 16, 8, 3, 4, 5]
