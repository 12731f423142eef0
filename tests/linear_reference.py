"""The logistic-regression tests' reference: sklearn's LinearModelLoss formulas
in ``np.longdouble``, with the magnitude sums of the derived error bounds
(docs/kernels.md "Logistic regression"), and the two fit problems."""

from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
L = np.longdouble


def reference(X, y, W, b, sw, l2=0.0):
    """(loss, gW [Kc][F], gb [Kc]) of the objective at (W, b), W [1][F] being
    the binomial head, and a namespace of the forward values (z, p, eps_z) and
    of the bounds on each output's error (tol_loss, tol_gW, tol_gb)."""
    N, F = X.shape
    Kc = W.shape[0]
    Xl, Wl = X.astype(L), W.astype(L)
    bl = np.zeros(Kc, L) if b is None else b.astype(L)
    swl = np.ones(N, L) if sw is None else sw.astype(L)
    sw_sum = swl.sum()
    rows = np.arange(N)
    z = Xl @ Wl.T + bl
    if Kc == 1:
        z0 = z[:, 0]
        li = np.log1p(np.exp(-np.abs(z0))) + np.maximum(z0, 0) - y * z0
        s = 1 / (1 + np.exp(-z0))
        p = np.stack([1 - s, s], axis=1)
        d = (s - y)[:, None]
    else:
        mx = z.max(axis=1)
        e = np.exp(z - mx[:, None])
        li = mx + np.log(e.sum(axis=1)) - z[rows, y]
        p = e / e.sum(axis=1, keepdims=True)
        d = p.copy()
        d[rows, y] -= 1
    d = d * swl[:, None]
    loss = (swl * li).sum() / sw_sum + l2 * (Wl * Wl).sum() / 2
    gW = d.T @ Xl / sw_sum + l2 * Wl
    gb = d.sum(axis=0) / sw_sum

    # the rounding of z, carried through a head whose slope is at most 1/2
    eps_z = (F + 1) * U * (np.abs(Xl) @ np.abs(Wl).T + np.abs(bl)).max()
    n_ulp = U * (N + 64)      # an N-term fp64 sum in any order, 64 ulps for exp and log
    bounds = SimpleNamespace(
        z=z, p=p, eps_z=float(eps_z),
        tol_gW=((n_ulp * (np.abs(d).T @ np.abs(Xl)) + eps_z * (swl @ np.abs(Xl))) / sw_sum
                + 4 * U * np.abs(l2 * Wl)).astype(np.float64),
        tol_gb=((n_ulp * np.abs(d).sum(axis=0) + eps_z * sw_sum) / sw_sum).astype(np.float64),
        tol_loss=float((n_ulp * np.abs(swl * li).sum() + 2 * eps_z * sw_sum) / sw_sum
                       + 4 * U * l2 * (Wl * Wl).sum() / 2))
    return loss, gW, gb, bounds


def objective_case(N, F, K, seed=0):
    """The asymmetric inputs of the objective tests -> X fp32, y, W, b, sw."""
    rng = np.random.default_rng(1000 * N + 10 * F + K + seed)
    Kc = 1 if K == 2 else K
    X = (rng.standard_normal((N, F)) * 1.5).astype(np.float32)
    y = rng.integers(0, K, N)
    y[0] = K - 1                      # the highest class is used
    W = rng.standard_normal((Kc, F)) * 1.5 / np.sqrt(F)
    return X, y, W, rng.standard_normal(Kc), rng.uniform(0.25, 2.0, N)


def fit_problem(binary):
    """A well-conditioned problem: 300 x 7 with 3 classes, or 200 x 5 binary;
    labels from a noisy linear rule."""
    N, F, K = (200, 5, 2) if binary else (300, 7, 3)
    rng = np.random.default_rng(7 + K)
    X = rng.standard_normal((N, F)).astype(np.float32)
    scores = X @ rng.standard_normal((F, K)) + 1.5 * rng.standard_normal((N, K))
    return X, scores.argmax(axis=1)


def sklearn_fit(X, y, **params):
    from sklearn.linear_model import LogisticRegression

    return LogisticRegression(tol=1e-8, max_iter=1000, **params).fit(X.astype(np.float64), y)


def fit_tolerance(X, y):
    """(sklearn's fit, tolerance): ten times the largest coefficient
    difference between sklearn on X and on five row permutations of X, at
    least 1e-12; also the measured sensitivity itself."""
    base = sklearn_fit(X, y)
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(5):
        perm = rng.permutation(len(y))
        other = sklearn_fit(X[perm], y[perm])
        worst = max(worst, np.abs(other.coef_ - base.coef_).max(),
                    np.abs(other.intercept_ - base.intercept_).max())
    return base, max(10 * worst, 1e-12), worst
