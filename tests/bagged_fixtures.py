"""Small seeded sklearn bagged forests and the rows that probe them, shared by
tests/test_bagged_forest_cpu.py and tests/test_gpu_bagged_forest.py. Every
model is fitted with n_jobs=None (sklearn then adds the trees in order) and
fits in well under a second."""

import functools

import numpy as np
from sklearn.ensemble import (ExtraTreesClassifier, ExtraTreesRegressor,
                              RandomForestClassifier, RandomForestRegressor)
from sklearn.tree import DecisionTreeClassifier

N_TRAIN = 400
# name -> (estimator class, classes (0: a regressor), features, training rows,
#          share of NaN in the training rows, estimator arguments)
MODELS = {
    "rf_digits": (RandomForestClassifier, 10, 64, 600, 0.0, {"n_estimators": 7}),
    "et_binary": (ExtraTreesClassifier, 2, 5, N_TRAIN, 0.0, {"n_estimators": 9}),
    "rf_classes32": (RandomForestClassifier, 32, 6, N_TRAIN, 0.0, {"n_estimators": 5}),
    "rf_regressor": (RandomForestRegressor, 0, 9, N_TRAIN, 0.0, {"n_estimators": 11}),
    "single_tree": (DecisionTreeClassifier, 3, 7, N_TRAIN, 0.0, {}),
    "root_only": (RandomForestRegressor, 0, 4, N_TRAIN, 0.0,
                  {"n_estimators": 3, "min_samples_leaf": N_TRAIN}),
    "stumps": (RandomForestClassifier, 3, 4, N_TRAIN, 0.0,
               {"n_estimators": 13, "max_depth": 1}),
    "rf_nan": (RandomForestClassifier, 4, 6, N_TRAIN, 0.1, {"n_estimators": 7}),
    # 79,999 nodes a tree: beyond 16-bit offsets and any LDS prefix
    "et_huge": (ExtraTreesRegressor, 0, 4, 40000, 0.0, {"n_estimators": 2}),
    # 300 features: the row tile's F > 256 branch at 16 rows a workgroup
    "wide": (RandomForestClassifier, 3, 300, N_TRAIN, 0.0, {"n_estimators": 5}),
}


def noisy_rows(rng, n, n_features, nan_share):
    X = rng.randn(n, n_features).astype(np.float32)
    X[rng.rand(n, n_features) < nan_share] = np.nan
    return X


@functools.lru_cache(maxsize=None)
def fitted(name):
    cls, classes, n_features, n, nan_share, kw = MODELS[name]
    rng = np.random.RandomState(sorted(MODELS).index(name))
    if name == "rf_digits":
        from sklearn.datasets import load_digits

        digits = load_digits()
        return cls(random_state=0, **kw).fit(digits.data[:n], digits.target[:n])
    X = noisy_rows(rng, n, n_features, nan_share)
    signal = np.nansum(X[:, :3], axis=1) + 0.3 * rng.randn(n)
    if classes == 0:
        return cls(random_state=0, **kw).fit(X, signal)
    y = np.argsort(np.argsort(signal)) * classes // n    # equal bins, all present
    return cls(random_state=0, **kw).fit(X, y)


def probe_rows(name, forest, n, seed=99):
    """n rows in the training rows' range; for the model fitted with NaN about
    10 % NaN and six +-inf; and for up to 64 distinct thresholds of the packed
    forest one row with that feature AT rd32(t) and one at the next fp32
    above it."""
    rng = np.random.RandomState(seed)
    nan_share = MODELS[name][4]
    X = noisy_rows(rng, n, forest.n_features, nan_share)
    if name == "rf_digits":
        X = np.abs(X) * 6.0
    if nan_share:
        X[rng.randint(0, n, 6), rng.randint(0, forest.n_features, 6)] = [np.inf, -np.inf] * 3
    nodes = forest._nodes_np
    inner = (nodes["meta"] >> 12) > 0
    pairs = np.unique(np.stack([nodes["meta"][inner] & 0x7FF, nodes["thr"][inner]], axis=1),
                      axis=0)
    pairs = pairs[rng.permutation(len(pairs))[:min(64, (n - 1) // 2)]]
    for i, (feature, bits) in enumerate(pairs):
        thr = np.uint32(bits).view(np.float32)
        X[2 * i + 1, int(feature)] = thr
        X[2 * i + 2, int(feature)] = np.nextafter(thr, np.float32(np.inf))
    return X


def sklearn_means(est, X):
    """sklearn's fp64 predict_proba (predict of a regressor) as [B][K]. Its
    input check refuses +-inf, so rows that hold one get what predict_proba
    computes, from sklearn's own tree walk: the leaves' values added in
    estimator order, then divided by the tree count."""
    finite = ~np.isinf(X).any(axis=1)
    public = est.predict_proba if hasattr(est, "classes_") else est.predict
    first = np.asarray(public(X[finite]), dtype=np.float64).reshape(int(finite.sum()), -1)
    out = np.empty((len(X), first.shape[1]))
    out[finite] = first
    if not finite.all():
        trees = [e.tree_ for e in getattr(est, "estimators_", [est])]
        acc = np.zeros((int((~finite).sum()), first.shape[1]))
        for tree in trees:
            acc += tree.value[tree.apply(X[~finite]), 0, :]
        acc /= len(trees)
        out[~finite] = acc
    return out
