"""What the tree apps (:mod:`unionml_amd.models.gbdt`,
:mod:`unionml_amd.models.rforest`) share: the digits frame and the
predictor's route through the estimator's device forest."""

from typing import List

import numpy as np
import pandas as pd

from unionml_amd.ops import hip_available
from unionml_amd.ops.forest import device_forest

FEATURES = [f"p{i}" for i in range(64)]


def digits_frame(n: int, synthetic: bool, seed: int) -> pd.DataFrame:
    """sklearn's digits (the first ``n`` rows when n > 0), or ``n or 1797``
    seeded random rows of the same shape, as FEATURES plus "target"."""
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


def device_labels(clf, features: pd.DataFrame) -> List[int]:
    """Labels from the estimator's device forest when a GPU is present,
    from the estimator itself otherwise."""
    if hip_available():
        X = features.to_numpy(dtype=np.float32)
        return [int(x) for x in device_forest(clf).predict(X)]
    return [int(x) for x in clf.predict(features)]
