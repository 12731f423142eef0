"""The grown-out regressor of the split-walk tests (trees of more than 2,048
nodes, which the chunked kernel refuses) and the rows that probe it."""

import functools

import numpy as np
from forest_fixtures import noisy_rows
from sklearn.ensemble import HistGradientBoostingRegressor

from unionml_amd.ops.forest import rd32

N_FEATURES = 6


@functools.lru_cache(maxsize=None)
def grown():
    """-> (estimator, probe rows, est.predict of them): 3 trees grown to one
    sample a leaf on 3,000 rows; 600 noisy rows and, for 64 thresholds, one
    row AT rd32(t) and one at the next fp32 above it."""
    rng = np.random.RandomState(17)
    X = noisy_rows(rng, 3000, N_FEATURES)
    y = np.nansum(X[:, :3], axis=1) + 0.3 * rng.randn(3000)
    est = HistGradientBoostingRegressor(max_iter=3, max_leaf_nodes=None,
                                        min_samples_leaf=1).fit(X, y)
    nodes = est._predictors[1][0].nodes
    inner = nodes[(nodes["is_leaf"] == 0) & np.isfinite(nodes["num_threshold"])][:64]
    rows = noisy_rows(rng, 600 + 2 * len(inner), N_FEATURES)
    for i, node in enumerate(inner):
        thr = rd32(node["num_threshold"])
        rows[600 + 2 * i, node["feature_idx"]] = thr
        rows[601 + 2 * i, node["feature_idx"]] = np.nextafter(thr, np.float32(np.inf))
    return est, rows, est.predict(rows)
