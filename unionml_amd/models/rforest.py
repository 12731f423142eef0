"""Random-forest app — the bagged-trees member of the built-in sklearn family.

sklearn's RandomForestClassifier on the digits shape through the same
decorator API as :mod:`unionml_amd.models.gbdt`. The app fits on the CPU and
predicts on the device: with a GPU present the predictor (and thereby the
evaluator) scores through
:class:`unionml_amd.ops.forest.BaggedForestPredictor`, whose kernel
reproduces the estimator's fp64 ``predict_proba`` bit for bit, so the labels
are ``clf.predict``'s.
"""

from typing import List

import numpy as np
import pandas as pd
from sklearn.ensemble import RandomForestClassifier

from unionml_amd import Dataset, Model
from unionml_amd.ops import hip_available
from unionml_amd.ops.forest import BaggedForestPredictor

FEATURES = [f"p{i}" for i in range(64)]

dataset = Dataset(name="rforest_digits", features=FEATURES, targets=["target"], test_size=0.2)
model = Model(name="digits_rforest", dataset=dataset)


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
def init(hyperparameters: dict) -> RandomForestClassifier:
    return RandomForestClassifier(
        **{"n_estimators": 100, "random_state": 0, **(hyperparameters or {})}
    )


@model.trainer
def trainer(
    clf: RandomForestClassifier,
    features: pd.DataFrame,
    target: pd.DataFrame,
    *,
    n_estimators: int = None,
) -> RandomForestClassifier:
    """One training pass; ``n_estimators`` overrides the tree count per run."""
    if n_estimators is not None:
        clf.set_params(n_estimators=n_estimators)
    return clf.fit(features, target.squeeze())


class _ForestCache:
    """The packed forest of a fitted estimator, kept on the estimator object.
    Valid while the estimator holds the same list of trees at the same length
    (a refit makes a new list, a warm start extends it). Pickles as an empty
    cache, so that a saved artifact holds no device memory."""

    def __init__(self):
        self.trees, self.count, self.forest = None, 0, None

    def __reduce__(self):
        return (_ForestCache, ())

    def get(self, clf) -> BaggedForestPredictor:
        trees = clf.estimators_
        if self.trees is not trees or self.count != len(trees):
            self.forest = BaggedForestPredictor.from_sklearn(clf)
            self.trees, self.count = trees, len(trees)
        return self.forest


def device_forest(clf: RandomForestClassifier) -> BaggedForestPredictor:
    """The estimator's device-resident forest, built once per fit."""
    cache = getattr(clf, "_unionml_forest", None)
    if cache is None:
        cache = clf._unionml_forest = _ForestCache()
    return cache.get(clf)


@model.predictor
def predictor(clf: RandomForestClassifier, features: pd.DataFrame) -> List[int]:
    if hip_available():
        X = features.to_numpy(dtype=np.float32)
        return [int(x) for x in device_forest(clf).predict(X)]
    return [int(x) for x in clf.predict(features)]


@model.evaluator
def evaluator(
    clf: RandomForestClassifier, features: pd.DataFrame, target: pd.DataFrame
) -> float:
    return float((np.asarray(predictor(clf, features)) == target.squeeze().to_numpy()).mean())
