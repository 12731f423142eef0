"""Gradient-boosted-trees app — the non-neural built-in model family.

sklearn's HistGradientBoostingClassifier on the digits shape through
the same decorator API (the reference's sklearn surface is exactly this
kind of estimator; its quickstart uses LogisticRegression —
tests/integration/sklearn_app/quickstart.py). Trees don't map to MFMA, so
the app fits on the CPU, predicts on the device: with a GPU present the
predictor (and thereby the evaluator) scores through
:class:`unionml_amd.ops.forest.ForestPredictor`, whose kernel reproduces the
estimator's fp64 raw scores bit for bit. It exists so the framework's "any
sklearn estimator" path has a first-class, tested boosting example with
warm-start iteration control.
"""

from typing import List

import numpy as np
import pandas as pd
from sklearn.ensemble import HistGradientBoostingClassifier

from unionml_amd import Dataset, Model
from unionml_amd.ops import hip_available
from unionml_amd.ops.forest import ForestPredictor

FEATURES = [f"p{i}" for i in range(64)]

dataset = Dataset(name="gbdt_digits", features=FEATURES, targets=["target"], test_size=0.2)
model = Model(name="digits_gbdt", dataset=dataset)


@dataset.reader
def reader(n: int = 0, synthetic: bool = False, seed: int = 17) -> pd.DataFrame:
    if synthetic:
        rng = np.random.RandomState(seed)
        X = rng.rand(n or 1797, 64).astype(np.float32) * 16.0
        y = rng.randint(0, 10, size=len(X))
    else:
        from sklearn.datasets import load_digits

        digits = load_digits()
        X, y = digits.data, digits.target
        if n:
            X, y = X[:n], y[:n]
    frame = pd.DataFrame(X, columns=FEATURES)
    frame["target"] = y
    return frame


@model.init
def init(hyperparameters: dict) -> HistGradientBoostingClassifier:
    return HistGradientBoostingClassifier(
        **{"max_iter": 100, "random_state": 0, **(hyperparameters or {})}
    )


@model.trainer
def trainer(
    clf: HistGradientBoostingClassifier,
    features: pd.DataFrame,
    target: pd.DataFrame,
    *,
    max_iter: int = None,
) -> HistGradientBoostingClassifier:
    """One training pass; ``max_iter`` overrides the boosting-iteration
    count per run (a "step" for this family = one boosting iteration)."""
    if max_iter is not None:
        clf.set_params(max_iter=max_iter)
    return clf.fit(features, target.squeeze())


class _ForestCache:
    """The packed forest of a fitted estimator, kept on the estimator object.
    Valid while the estimator holds the same list of iterations at the same
    length (a refit makes a new list, a warm start extends it). Pickles as an
    empty cache, so that a saved artifact holds no device memory."""

    def __init__(self):
        self.iterations, self.count, self.forest = None, 0, None

    def __reduce__(self):
        return (_ForestCache, ())

    def get(self, clf) -> ForestPredictor:
        its = clf._predictors
        if self.iterations is not its or self.count != len(its):
            self.forest = ForestPredictor.from_sklearn(clf)
            self.iterations, self.count = its, len(its)
        return self.forest


def device_forest(clf: HistGradientBoostingClassifier) -> ForestPredictor:
    """The estimator's device-resident forest, built once per fit."""
    cache = getattr(clf, "_unionml_forest", None)
    if cache is None:
        cache = clf._unionml_forest = _ForestCache()
    return cache.get(clf)


@model.predictor
def predictor(clf: HistGradientBoostingClassifier, features: pd.DataFrame) -> List[int]:
    if hip_available():
        X = features.to_numpy(dtype=np.float32)
        return [int(x) for x in device_forest(clf).predict(X)]
    return [int(x) for x in clf.predict(features)]


@model.evaluator
def evaluator(
    clf: HistGradientBoostingClassifier, features: pd.DataFrame, target: pd.DataFrame
) -> float:
    return float((np.asarray(predictor(clf, features)) == target.squeeze().to_numpy()).mean())
