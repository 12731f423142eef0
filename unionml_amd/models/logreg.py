"""Logistic-regression app — the README example of the project this one
follows, through the same decorator API as :mod:`unionml_amd.models.rforest`.

``init`` returns sklearn's ``LogisticRegression``. With a GPU present the
trainer fits through
:class:`unionml_amd.ops.linear.DeviceLogisticRegression` (scipy's L-BFGS-B
driving the fp64 loss/gradient kernel) and hands back a plain sklearn
estimator, so the saved artifact and the serving code see nothing new; the
predictor scores through the estimator's device predictor. Without a GPU
both go through sklearn.
"""

from typing import List

import numpy as np
import pandas as pd
from sklearn.linear_model import LogisticRegression

from unionml_amd import Dataset, Model
from unionml_amd.models._forest_app import FEATURES, digits_frame
from unionml_amd.ops import hip_available
from unionml_amd.ops.linear import DeviceLogisticRegression, device_linear

dataset = Dataset(name="logreg_digits", features=FEATURES, targets=["target"], test_size=0.2)
model = Model(name="digits_logreg", dataset=dataset)


@dataset.reader
def reader(n: int = 0, synthetic: bool = False, seed: int = 17) -> pd.DataFrame:
    return digits_frame(n, synthetic, seed)


@model.init
def init(hyperparameters: dict) -> LogisticRegression:
    return LogisticRegression(**{"max_iter": 1000, **(hyperparameters or {})})


@model.trainer
def trainer(
    clf: LogisticRegression,
    features: pd.DataFrame,
    target: pd.DataFrame,
    *,
    max_iter: int = None,
) -> LogisticRegression:
    """One fit; ``max_iter`` overrides the iteration cap per run."""
    if max_iter is not None:
        clf.set_params(max_iter=max_iter)
    if not hip_available():
        return clf.fit(features, target.squeeze())
    fitted = DeviceLogisticRegression(
        C=clf.C, penalty=clf.penalty, fit_intercept=clf.fit_intercept, tol=clf.tol,
        max_iter=clf.max_iter, class_weight=clf.class_weight, l1_ratio=clf.l1_ratio,
    ).fit(features.to_numpy(dtype=np.float32), target.squeeze().to_numpy())
    return fitted.to_sklearn()


@model.predictor
def predictor(clf: LogisticRegression, features: pd.DataFrame) -> List[int]:
    if hip_available():
        return [int(x) for x in device_linear(clf).predict(features.to_numpy(dtype=np.float32))]
    return [int(x) for x in clf.predict(features)]


@model.evaluator
def evaluator(clf: LogisticRegression, features: pd.DataFrame, target: pd.DataFrame) -> float:
    return float((np.asarray(predictor(clf, features)) == target.squeeze().to_numpy()).mean())
