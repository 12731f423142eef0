"""Ridge-regression app on sklearn's bundled diabetes set, through the same
decorator API as :mod:`unionml_amd.models.logreg`.

``init`` returns sklearn's ``Ridge``. With a GPU present the trainer fits
through :class:`unionml_amd.ops.linear.DeviceRidge` (the fp64 Gram kernel and a
host Cholesky solve) and hands back a plain sklearn estimator, so the saved
artifact and the serving code see nothing new; the predictor scores through the
estimator's device predictor. Without a GPU both go through sklearn.
"""

from typing import List

import numpy as np
import pandas as pd
from sklearn.linear_model import Ridge

from unionml_amd import Dataset, Model
from unionml_amd.models.mlp_regress import FEATURES
from unionml_amd.models.mlp_regress import reader as diabetes_frame
from unionml_amd.ops import hip_available
from unionml_amd.ops.linear import DeviceRidge, device_linear_regressor

dataset = Dataset(name="ridge_diabetes", features=FEATURES, targets=["target"], test_size=0.2)
model = Model(name="diabetes_ridge", dataset=dataset)


@dataset.reader
def reader(n: int = 0, synthetic: bool = False, seed: int = 17) -> pd.DataFrame:
    return diabetes_frame(n, synthetic, seed)


@model.init
def init(hyperparameters: dict) -> Ridge:
    return Ridge(**(hyperparameters or {}))


@model.trainer
def trainer(reg: Ridge, features: pd.DataFrame, target: pd.DataFrame) -> Ridge:
    if not hip_available():
        return reg.fit(features, target.squeeze())
    fitted = DeviceRidge(alpha=reg.alpha, fit_intercept=reg.fit_intercept).fit(
        features.to_numpy(dtype=np.float32), target.squeeze().to_numpy(dtype=np.float64))
    return fitted.to_sklearn()


@model.predictor
def predictor(reg: Ridge, features: pd.DataFrame) -> List[float]:
    if hip_available():
        scores = device_linear_regressor(reg).predict(features.to_numpy(dtype=np.float32))
        return [float(x) for x in scores]
    return [float(x) for x in reg.predict(features)]


@model.evaluator
def evaluator(reg: Ridge, features: pd.DataFrame, target: pd.DataFrame) -> float:
    """Coefficient of determination R^2 (1 is exact, 0 the mean predictor)."""
    y = target.squeeze().to_numpy(dtype=np.float64)
    residual = y - np.asarray(predictor(reg, features))
    return float(1.0 - (residual @ residual) / ((y - y.mean()) @ (y - y.mean())))
