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
from unionml_amd.models._forest_app import FEATURES, device_labels, digits_frame
# _ForestCache: artifacts saved by earlier versions name it in this module
from unionml_amd.ops.forest import _ForestCache, device_forest  # noqa: F401

dataset = Dataset(name="rforest_digits", features=FEATURES, targets=["target"], test_size=0.2)
model = Model(name="digits_rforest", dataset=dataset)


@dataset.reader
def reader(n: int = 0, synthetic: bool = False, seed: int = 17) -> pd.DataFrame:
    return digits_frame(n, synthetic, seed)


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


@model.predictor
def predictor(clf: RandomForestClassifier, features: pd.DataFrame) -> List[int]:
    return device_labels(clf, features)


@model.evaluator
def evaluator(
    clf: RandomForestClassifier, features: pd.DataFrame, target: pd.DataFrame
) -> float:
    return float((np.asarray(predictor(clf, features)) == target.squeeze().to_numpy()).mean())
