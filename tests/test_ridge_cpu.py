"""unionml_amd.ops.linear.DeviceRidge without a GPU: the numpy path against
sklearn, the refusals, and the Python copy of linear_gram.h's limits."""

import numpy as np
import pytest
import scipy.sparse

from ridge_reference import (FIT_PROBLEMS, difference, fit_problem, fit_tolerance,
                             predict_bound)
from unionml_amd.ops import linear
from unionml_amd.ops.linear import DeviceRidge


@pytest.mark.parametrize("problem", FIT_PROBLEMS, ids=lambda p: "x".join(map(str, p[:3])))
def test_numpy_fit_matches_sklearn(problem):
    X, y, sw = fit_problem(*problem)
    base, tol, _ = fit_tolerance(X, y, sw, problem[4])
    model = DeviceRidge(alpha=1.0, fit_intercept=problem[4], device="cpu").fit(X, y, sw)
    assert model.coef_.shape == base.coef_.shape and model.n_features_in_ == X.shape[1]
    assert np.shape(model.intercept_) == np.shape(base.intercept_)
    assert difference(model, base) <= tol
    served = model.to_sklearn().predict(X.astype(np.float64))
    assert served.shape == model.predict(X).shape
    assert np.abs(served - model.predict(X)).max() <= predict_bound(X, model.coef_,
                                                                    model.intercept_)


@pytest.mark.parametrize("refused", ["f4097", "t33", "y3d", "sparse", "alpha", "singular"])
def test_refusals(refused):
    X, y, alpha = np.ones((4, 3), np.float32), np.ones(4), 1.0
    if refused == "f4097":
        X, y = np.ones((2, 4097), np.float32), np.ones(2)
    elif refused == "t33":
        y = np.ones((4, 33))
    elif refused == "y3d":
        y = np.ones((4, 1, 1))
    elif refused == "sparse":
        X = scipy.sparse.csr_matrix(X)
    elif refused == "alpha":
        alpha = -1e-3
    elif refused == "singular":
        alpha = 0.0                      # three equal columns
    with pytest.raises(ValueError):
        DeviceRidge(alpha=alpha, device="cpu").fit(X, y)


def test_limits_are_the_headers():
    assert (linear.RIDGE_MAX_FEATURES, linear.RIDGE_MAX_TARGETS) == (4096, 32)
