"""Small seeded sklearn forests and the rows that probe them, shared by
tests/test_forest_cpu.py and tests/test_gpu_forest.py. Every model fits in
well under a second (at most 400 rows, 8 iterations); the training data
holds NaNs, so both values of missing_go_to_left occur."""

import functools

import numpy as np
from sklearn.ensemble import HistGradientBoostingClassifier, HistGradientBoostingRegressor

N_TRAIN = 400
# name -> (classes, 0 for a regressor; features; estimator arguments)
MODELS = {
    "regressor": (0, 9, {}),
    "binary": (2, 5, {}),
    "classes3": (3, 7, {"max_leaf_nodes": 15}),
    "classes17": (17, 6, {}),          # produces infinite thresholds
    "classes32": (32, 1, {}),
    "root_only": (3, 4, {"min_samples_leaf": N_TRAIN // 2 + 1}),
    "deep": (2, 6, {"max_leaf_nodes": None, "min_samples_leaf": 1}),
    "wide": (3, 300, {}),              # forces a smaller row tile
}


def noisy_rows(rng, n, n_features):
    """fp32 normals, about 15 % NaN."""
    X = rng.randn(n, n_features).astype(np.float32)
    X[rng.rand(n, n_features) < 0.15] = np.nan
    return X


@functools.lru_cache(maxsize=None)
def fitted(name):
    classes, n_features, kw = MODELS[name]
    rng = np.random.RandomState(sorted(MODELS).index(name))
    X = noisy_rows(rng, N_TRAIN, n_features)
    signal = np.nansum(X[:, :3], axis=1) + 0.3 * rng.randn(N_TRAIN)
    if classes == 0:
        return HistGradientBoostingRegressor(max_iter=8, **kw).fit(X, signal)
    y = np.argsort(np.argsort(signal)) * classes // N_TRAIN    # equal bins, all present
    return HistGradientBoostingClassifier(max_iter=8, **kw).fit(X, y)


def probe_rows(forest, n, seed=99):
    """n rows: noisy normals with a few +-inf, and for up to 64 distinct
    finite thresholds of the packed forest one row with that feature AT
    rd32(t) and one at the next fp32 above it."""
    rng = np.random.RandomState(seed)
    X = noisy_rows(rng, n, forest.n_features)
    X[rng.randint(0, n, 6), rng.randint(0, forest.n_features, 6)] = [np.inf, -np.inf] * 3
    nodes = forest._nodes_np
    finite = np.isfinite(nodes["thr"])
    pairs = np.unique(np.stack([(nodes["meta"][finite] & 0xFFFF).astype(np.float64),
                                nodes["thr"][finite].astype(np.float64)], axis=1),
                      axis=0)[:min(64, (n - 1) // 2)]
    for i, (feature, thr) in enumerate(pairs):
        thr = np.float32(thr)
        X[2 * i + 1, int(feature)] = thr
        X[2 * i + 2, int(feature)] = np.nextafter(thr, np.float32(np.inf))
    return X


def sklearn_scores(est, X):
    """sklearn's fp64 raw scores as [B][K]."""
    raw = est.decision_function(X) if hasattr(est, "classes_") else est.predict(X)
    return np.asarray(raw, dtype=np.float64).reshape(len(X), -1)


def raw_argmax_labels(est, scores):
    """Labels by the raw-score argmax (score > 0 when binary) through classes_."""
    idx = (scores[:, 0] > 0).astype(int) if scores.shape[1] == 1 else scores.argmax(axis=1)
    return est.classes_[idx]
