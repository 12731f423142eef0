"""The ridge tests' reference: the Gram kernel's outputs in ``np.longdouble``
with the derived error bounds (docs/kernels.md "Ridge regression"), and the
three fit problems with sklearn's own sensitivity to row order."""

import numpy as np

U = 2.0 ** -53
L = np.longdouble


def gram_case(N, F, T):
    """Seeded inputs -> X fp32 (column scales 0.5..2 and offsets -3..3, so that
    centring matters), Y fp64, weights in 0.5..2."""
    rng = np.random.default_rng(1000 * N + 10 * F + T)
    X = (rng.standard_normal((N, F)) * rng.uniform(0.5, 2.0, F) + rng.uniform(-3, 3, F))
    Y = rng.standard_normal((N, T)) * 2.0 + rng.uniform(-3, 3, T)
    return X.astype(np.float32), Y, rng.uniform(0.5, 2.0, N)


def mean_reference(X, Y, sw, center):
    """(mean [F + T], its bound): u (N + 4) sum|w x| / sum w + u |mean|."""
    Z = np.concatenate([X.astype(L), Y.astype(L)], axis=1)
    if not center:
        return np.zeros(Z.shape[1], L), np.zeros(Z.shape[1])
    w = np.ones(len(X), L) if sw is None else sw.astype(L)
    mean = w @ Z / w.sum()
    bound = U * (len(X) + 4) * (w @ np.abs(Z)) / w.sum() + U * np.abs(mean)
    return mean, bound.astype(np.float64)


def gram_reference(X, Y, sw, alpha, mean):
    """(A, Xy, bound of A, bound of Xy) centred with ``mean``, the kernel's
    own: u (N + 8) sum|w c_p c_q| + u |A_pq|, the worst case of an N-term fp64
    sum in any order plus the operand path's three roundings and alpha."""
    N, F = X.shape
    w = np.ones(N, L) if sw is None else sw.astype(L)
    Xc, Yc = X.astype(L) - mean[:F].astype(L), Y.astype(L) - mean[F:].astype(L)
    wX = Xc * w[:, None]
    A, Xy = wX.T @ Xc + alpha * np.eye(F, dtype=L), wX.T @ Yc
    tol_A = U * (N + 8) * (np.abs(wX).T @ np.abs(Xc)) + U * np.abs(A)
    tol_Xy = U * (N + 8) * (np.abs(wX).T @ np.abs(Yc)) + U * np.abs(Xy)
    return A, Xy, tol_A.astype(np.float64), tol_Xy.astype(np.float64)


# (N, F, T, weighted, fit_intercept)
FIT_PROBLEMS = [(300, 7, 1, False, True), (200, 5, 3, True, True), (150, 40, 2, True, False)]


def fit_problem(N, F, T, weighted, fit_intercept):
    """A well-conditioned problem -> X fp32, y ([N] for one target), weights or
    None."""
    rng = np.random.default_rng(11 * N + F + T)
    X = rng.standard_normal((N, F)).astype(np.float32)
    y = X @ rng.standard_normal((F, T)) + 0.5 * rng.standard_normal((N, T)) + 1.0
    return X, (y[:, 0] if T == 1 else y), (rng.uniform(0.5, 2.0, N) if weighted else None)


def sklearn_fit(X, y, sw, fit_intercept):
    from sklearn.linear_model import Ridge

    return Ridge(alpha=1.0, fit_intercept=fit_intercept, solver="cholesky").fit(
        X.astype(np.float64), y, sample_weight=sw)


def difference(a, b):
    return max(np.abs(a.coef_ - b.coef_).max(),
               np.abs(np.asarray(a.intercept_) - np.asarray(b.intercept_)).max())


def fit_tolerance(X, y, sw, fit_intercept):
    """(sklearn's fit, tolerance, sensitivity): ten times the largest
    coefficient or intercept difference between sklearn on X and on five row
    permutations of X, at least 1e-12."""
    base = sklearn_fit(X, y, sw, fit_intercept)
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(5):
        perm = rng.permutation(len(y))
        other = sklearn_fit(X[perm], y[perm], None if sw is None else sw[perm], fit_intercept)
        worst = max(worst, difference(other, base))
    return base, max(10 * worst, 1e-12), worst


def predict_bound(X, coef, intercept):
    """The predict bound of the logistic section: (F + 1) u max(|X| |W|^T + |b|)."""
    W = np.atleast_2d(coef).astype(L)
    b = np.broadcast_to(np.asarray(intercept, dtype=L), (W.shape[0],))
    return float((X.shape[1] + 1) * U * (np.abs(X.astype(L)) @ np.abs(W).T + np.abs(b)).max())
