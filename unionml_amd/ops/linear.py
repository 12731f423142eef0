"""Logistic regression fitted and scored on the device.

``DeviceLogisticRegression`` is sklearn's ``LogisticRegression(solver="lbfgs")``
with the one hot function moved to the GPU: scipy's L-BFGS-B drives
``logistic_loss_grad`` (``hip/linear_logistic.hip``), which evaluates the loss
and gradient of sklearn's ``LinearModelLoss`` over the whole training set in
fp64 on the matrix cores. The optimiser call, the starting point, the penalty
scaling and the parameter ravelling are sklearn's, so on a well-conditioned
problem the coefficients agree with sklearn's to the reference's own
sensitivity to summation order (docs/kernels.md "Logistic regression").

**X is held in fp32 on the device.** An fp64 X that is not fp32-representable
is rounded once, on the way in; results equal sklearn's fp64 path only for an
fp32-representable X (sklearn fitted on ``X.astype(np.float32).astype(np.float64)``).

``LinearPredictor`` scores rows through ``linear_predict`` (scores,
probabilities and labels in one launch); ``LinearPredictor.from_sklearn(est)``
and ``device_linear(est)`` serve a fitted sklearn ``LogisticRegression``.
Without a GPU the same classes run a numpy fp64 implementation of the same
formulas; on a GPU machine a missing extension is ``KernelExtensionNotBuilt``.

``DeviceRidge`` is sklearn's ``Ridge(solver="cholesky")`` with the centred,
weighted Gram matrix and moment matrix formed on the device by ``ridge_gram``
(``hip/linear_gram.hip``) and scipy's ``solve(A, Xy, assume_a="pos")`` on the
host (docs/kernels.md "Ridge regression"). ``LinearRegressionPredictor`` and
``device_linear_regressor(est)`` score a fitted ``Ridge`` or
``LinearRegression`` through ``linear_predict``.
"""

import warnings

import numpy as np
import torch

from unionml_amd.ops import hip_ext

# the Python copy of hip/linear_logistic.h
MAX_CLASSES = 32
MAX_FEATURES = 1 << 20
# the Python copy of hip/linear_gram.h
RIDGE_MAX_FEATURES = 4096
RIDGE_MAX_TARGETS = 32


def _refuse_beyond_limits(n_classes, n_features):
    if n_classes < 2:
        raise ValueError(f"{n_classes} class: a classifier needs at least two")
    if n_classes > MAX_CLASSES:
        raise ValueError(f"{n_classes} classes: the kernels take at most {MAX_CLASSES}")
    if not 1 <= n_features <= MAX_FEATURES:
        raise ValueError(f"{n_features} features: the kernels take 1..{MAX_FEATURES}")


def _rows(X, n_features=None):
    """A dense float [B][F] as a contiguous fp32 CPU tensor (one rounding of
    an fp64 X)."""
    if hasattr(X, "tocsr"):
        raise ValueError("a sparse X is not supported: pass a dense float [B][F]")
    if not torch.is_tensor(X):
        X = torch.as_tensor(np.asarray(X))
    if X.dim() != 2 or not (X.is_floating_point() or n_features is None):
        raise ValueError(f"X must be a float [B][F], is {tuple(X.shape)} {X.dtype}")
    if n_features is not None and X.shape[1] != n_features:
        raise ValueError(f"X must be [B][{n_features}], is {tuple(X.shape)}")
    return X.to(torch.float32).contiguous()


def _expit(z):
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def objective_numpy(X, y, sw, W, b, sw_sum, l2):
    """The kernels' formulas in numpy fp64 -> (loss, gW [Kc][F], gb [Kc]).
    ``W`` [1][F] is the binomial head, y in {0, 1}."""
    z = X @ W.T
    if b is not None:
        z = z + b
    rows = np.arange(len(y))
    if W.shape[0] == 1:
        z = z[:, 0]
        loss = np.log1p(np.exp(-np.abs(z))) + np.maximum(z, 0.0) - y * z
        d = (_expit(z) - y)[:, None]
    else:
        mx = z.max(axis=1)
        e = np.exp(z - mx[:, None])
        s = e.sum(axis=1)
        loss = mx + np.log(s) - z[rows, y]
        d = e / s[:, None]
        d[rows, y] -= 1.0
    if sw is not None:
        loss, d = loss * sw, d * sw[:, None]
    return (loss.sum() / sw_sum + 0.5 * l2 * (W * W).sum(), d.T @ X / sw_sum + l2 * W,
            d.sum(axis=0) / sw_sum)


class LinearPredictor:
    """A linear classifier (``coef`` [Kc][F], ``intercept`` [Kc] or None; Kc 1
    for two classes) on one device. Build with :meth:`from_sklearn`."""

    def __init__(self, coef, intercept, classes, device=None):
        coef = np.ascontiguousarray(coef, dtype=np.float64)
        classes = np.asarray(classes)
        _refuse_beyond_limits(len(classes), coef.shape[1])
        if coef.shape[0] != (1 if len(classes) == 2 else len(classes)):
            raise ValueError(f"coef is {coef.shape} for {len(classes)} classes")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.classes_ = classes
        self.n_features = coef.shape[1]
        self.n_scores = coef.shape[0]
        self._W_np = coef
        self._b_np = (None if intercept is None
                      else np.array(intercept, dtype=np.float64).reshape(-1))
        self._ext = None
        if self.device.type == "cuda":
            self._ext = hip_ext(required=True)
            self._W = torch.from_numpy(coef).to(self.device)
            self._b = None if self._b_np is None else torch.from_numpy(self._b_np).to(self.device)

    @classmethod
    def from_sklearn(cls, est, device=None):
        from sklearn.linear_model import LogisticRegression

        if not isinstance(est, LogisticRegression) or not hasattr(est, "coef_"):
            raise TypeError(f"{type(est).__name__} is no fitted LogisticRegression")
        if len(est.classes_) > 2 and getattr(est, "multi_class", "auto") == "ovr":
            raise ValueError("a one-vs-rest model is not supported: the kernel's "
                             "probabilities are the softmax of the scores")
        intercept = np.broadcast_to(np.asarray(est.intercept_, dtype=np.float64),
                                    (est.coef_.shape[0],))
        return cls(est.coef_, intercept, est.classes_, device=device)

    def _score(self, X, rows_per_wg=0, max_wgs=0):
        """-> (scores fp64 [B][Kc], probs fp64 [B][K], class indices int32 [B])
        on the predictor's device."""
        X = _rows(X, self.n_features).to(self.device)
        B, K = X.shape[0], len(self.classes_)
        scores = torch.empty(B, self.n_scores, dtype=torch.float64, device=self.device)
        probs = torch.empty(B, K, dtype=torch.float64, device=self.device)
        labels = torch.empty(B, dtype=torch.int32, device=self.device)
        if B == 0:
            return scores, probs, labels
        if self._ext is not None:
            self._ext.linear_predict(X, self._W, self._b, scores, probs, labels, rows_per_wg,
                                     max_wgs)
            return scores, probs, labels
        z = X.numpy().astype(np.float64) @ self._W_np.T
        if self._b_np is not None:
            z = z + self._b_np
        if self.n_scores == 1:
            p = _expit(z[:, 0])
            p, idx = np.stack([1.0 - p, p], axis=1), z[:, 0] > 0
        else:
            e = np.exp(z - z.max(axis=1, keepdims=True))
            p, idx = e / e.sum(axis=1, keepdims=True), z.argmax(axis=1)   # first largest
        scores.copy_(torch.from_numpy(z))
        probs.copy_(torch.from_numpy(p))
        labels.copy_(torch.from_numpy(idx.astype(np.int32)))
        return scores, probs, labels

    def decision_function(self, X):
        """``X W^T + b`` in fp64 on the predictor's device: ``[B][K]``, or
        ``[B]`` for two classes, as sklearn shapes it."""
        scores = self._score(X)[0]
        return scores[:, 0] if self.n_scores == 1 else scores

    def predict_proba(self, X):
        """fp64 ``[B][n_classes]``: the softmax of a row's scores, or
        ``[1 - s, s]`` with ``s`` the logistic function of the one score."""
        return self._score(X)[1]

    def predict(self, X):
        """``classes_`` at the first largest score (``score > 0`` for two
        classes), a numpy array."""
        return self.classes_[self._score(X)[2].cpu().numpy()]


class DeviceLogisticRegression:
    """sklearn's ``LogisticRegression(solver="lbfgs")`` with the objective on
    the device. ``penalty`` is ``"l2"`` or ``None``; the other parameters mean
    what sklearn's mean. X is held in fp32 (see the module docstring)."""

    def __init__(self, C=1.0, penalty="l2", fit_intercept=True, tol=1e-4, max_iter=100,
                 class_weight=None, device=None, l1_ratio=None):
        if penalty not in ("l2", None) or l1_ratio is not None:
            raise ValueError(f"penalty={penalty!r}, l1_ratio={l1_ratio!r}: only the l2 penalty "
                             "and no penalty are served")
        if not C > 0:
            raise ValueError(f"C must be positive, is {C}")
        self.C, self.penalty, self.fit_intercept = float(C), penalty, bool(fit_intercept)
        self.tol, self.max_iter, self.class_weight = float(tol), int(max_iter), class_weight
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self._predictor = None

    # -- fitting ------------------------------------------------------------------

    def fit(self, X, y, sample_weight=None, rows_per_wg=0, max_wgs=0):
        """Fit by L-BFGS-B from zero, as sklearn does. ``rows_per_wg`` and
        ``max_wgs`` override the launcher's choices (tests)."""
        from sklearn.preprocessing import LabelEncoder
        from sklearn.utils.class_weight import compute_class_weight

        X = _rows(X)
        y = np.asarray(y)
        if y.ndim != 1 or len(y) != X.shape[0] or len(y) == 0:
            raise ValueError(f"y must be [{X.shape[0]}] with at least one row, is {y.shape}")
        encoder = LabelEncoder()
        y_idx = encoder.fit_transform(y)
        classes = encoder.classes_
        N, F, K = X.shape[0], X.shape[1], len(classes)
        _refuse_beyond_limits(K, F)
        Kc = 1 if K == 2 else K

        sw = None
        if sample_weight is not None or self.class_weight is not None:
            sw = (np.ones(N) if sample_weight is None
                  else np.array(sample_weight, dtype=np.float64))
            if sw.shape != (N,):
                raise ValueError(f"sample_weight must be [{N}], is {sw.shape}")
            if self.class_weight is not None:
                sw *= compute_class_weight(self.class_weight, classes=classes, y=y,
                                           sample_weight=sw)[y_idx]
        sw_sum = float(N) if sw is None else float(np.sum(sw))
        if not sw_sum > 0:
            raise ValueError("the sample weights must have a positive sum")
        l2 = 0.0 if self.penalty is None else 1.0 / (self.C * sw_sum)

        objective = (self._device_objective if self.device.type == "cuda"
                     else self._numpy_objective)(X, y_idx, sw, Kc, sw_sum, l2, rows_per_wg, max_wgs)
        # sklearn's call: parameters [Kc][F + intercept] ravelled column-major
        from scipy.optimize import minimize

        w0 = np.zeros(Kc * (F + int(self.fit_intercept)))
        res = minimize(objective, w0, method="L-BFGS-B", jac=True,
                       options={"maxiter": self.max_iter, "maxls": 50, "gtol": self.tol,
                                "ftol": 64 * np.finfo(float).eps})
        if res.status != 0:
            from sklearn.exceptions import ConvergenceWarning

            warnings.warn(f"lbfgs failed to converge (status={res.status}): {res.message}",
                          ConvergenceWarning)
        w = res.x.reshape((Kc, -1), order="F")
        self.coef_ = np.ascontiguousarray(w[:, :F])
        self.intercept_ = w[:, F].copy() if self.fit_intercept else np.zeros(Kc)
        self.classes_ = classes
        self.n_iter_ = np.asarray([min(res.nit, self.max_iter)], dtype=np.int32)
        self.n_features_in_ = F
        self.n_evaluations_ = int(res.nfev)
        self._predictor = LinearPredictor(self.coef_,
                                          self.intercept_ if self.fit_intercept else None,
                                          classes, device=self.device)
        return self

    def _numpy_objective(self, X, y_idx, sw, Kc, sw_sum, l2, *launch):
        X = X.numpy().astype(np.float64)
        F = X.shape[1]

        def objective(w):
            w2 = w.reshape((Kc, -1), order="F")
            loss, gW, gb = objective_numpy(X, y_idx, sw, w2[:, :F],
                                           w2[:, F] if self.fit_intercept else None, sw_sum, l2)
            grad = np.concatenate([gW, gb[:, None]], axis=1) if self.fit_intercept else gW
            return float(loss), grad.ravel(order="F")

        return objective

    def _device_objective(self, X, y_idx, sw, Kc, sw_sum, l2, rows_per_wg, max_wgs):
        """X, y and the weights go to the device once; an evaluation uploads
        the parameters, runs the two launches and brings ``out`` back through
        one pinned buffer."""
        ext, dev = hip_ext(required=True), self.device
        N, F = X.shape
        n_w, P = Kc * F, Kc * (F + int(self.fit_intercept))
        with torch.cuda.device(dev):
            _, grid = ext.logistic_launch_shape(N, rows_per_wg, max_wgs)
        Xd = X.to(dev)
        yd = torch.from_numpy(y_idx.astype(np.int32)).to(dev)
        swd = None if sw is None else torch.from_numpy(sw).to(dev)
        slabs = torch.empty(grid, n_w + Kc + 1, dtype=torch.float64, device=dev)
        params = torch.empty(P, dtype=torch.float64, device=dev)
        out = torch.empty(P + 1, dtype=torch.float64, device=dev)
        params_host = torch.empty(P, dtype=torch.float64).pin_memory()
        out_host = torch.empty(P + 1, dtype=torch.float64).pin_memory()
        params_np, out_np = params_host.numpy(), out_host.numpy()
        Wd = params[:n_w].view(Kc, F)
        bd = params[n_w:] if self.fit_intercept else None

        def objective(w):
            # column-major [Kc][F + 1] -> the kernels' [W row-major | b]
            w2 = w.reshape((Kc, -1), order="F")
            params_np[:n_w] = w2[:, :F].ravel()
            if self.fit_intercept:
                params_np[n_w:] = w2[:, F]
            with torch.cuda.device(dev):
                params.copy_(params_host, non_blocking=True)
                ext.logistic_loss_grad(Xd, yd, swd, Wd, bd, sw_sum, l2, slabs, out, rows_per_wg,
                                       max_wgs)
                out_host.copy_(out, non_blocking=True)
                torch.cuda.current_stream().synchronize()
            grad = np.empty((Kc, F + int(self.fit_intercept)), order="F")
            grad[:, :F] = out_np[:n_w].reshape(Kc, F)
            if self.fit_intercept:
                grad[:, F] = out_np[n_w:P]
            return float(out_np[P]), grad.ravel(order="F")

        return objective

    # -- the fitted model ---------------------------------------------------------

    def _fitted(self):
        if self._predictor is None:
            raise ValueError("this DeviceLogisticRegression is not fitted yet")
        return self._predictor

    def decision_function(self, X):
        return self._fitted().decision_function(X)

    def predict_proba(self, X):
        return self._fitted().predict_proba(X)

    def predict(self, X):
        return self._fitted().predict(X)

    def to_sklearn(self):
        """A plain ``sklearn.linear_model.LogisticRegression`` carrying the
        fitted attributes: what artifacts save and the serving code loads."""
        from sklearn.linear_model import LogisticRegression

        self._fitted()
        est = LogisticRegression(C=self.C, penalty=self.penalty, fit_intercept=self.fit_intercept,
                                 tol=self.tol, max_iter=self.max_iter,
                                 class_weight=self.class_weight)
        est.coef_, est.intercept_ = self.coef_.copy(), self.intercept_.copy()
        est.classes_, est.n_iter_ = self.classes_.copy(), self.n_iter_.copy()
        est.n_features_in_ = self.n_features_in_
        return est


class _LinearCache:
    """The device predictor of a fitted estimator, kept on the estimator
    object. Valid while the estimator holds the same ``coef_`` and
    ``intercept_`` arrays: a refit makes new ones. Pickles as an empty cache,
    so that a saved artifact holds no device memory."""

    def __init__(self):
        self.coef, self.intercept, self.predictor = None, None, None

    def __reduce__(self):
        return (_LinearCache, ())

    def get(self, est):
        if self.coef is not est.coef_ or self.intercept is not est.intercept_:
            self.predictor = LinearPredictor.from_sklearn(est)
            self.coef, self.intercept = est.coef_, est.intercept_
        return self.predictor


def device_linear(est):
    """The device predictor of a fitted sklearn ``LogisticRegression``, built
    once per fit and kept on the estimator."""
    cache = getattr(est, "_unionml_linear", None)
    if cache is None:
        cache = est._unionml_linear = _LinearCache()
    return cache.get(est)


# ---- ridge regression ---------------------------------------------------------------


def _refuse_beyond_ridge_limits(n_features, n_targets):
    if not 1 <= n_features <= RIDGE_MAX_FEATURES:
        raise ValueError(f"{n_features} features: the Gram kernel takes 1..{RIDGE_MAX_FEATURES}")
    if not 1 <= n_targets <= RIDGE_MAX_TARGETS:
        raise ValueError(f"{n_targets} targets: the kernels take 1..{RIDGE_MAX_TARGETS}")


def gram_numpy(X, Y, sw, alpha, center):
    """The Gram kernel's formulas in numpy fp64 -> (mean [F + T], A [F][F],
    Xy [F][T])."""
    w = np.ones(len(X)) if sw is None else sw
    if center:
        mu, ybar = w @ X / w.sum(), w @ Y / w.sum()
    else:
        mu, ybar = np.zeros(X.shape[1]), np.zeros(Y.shape[1])
    Xc, Yc = X - mu, Y - ybar
    A = (Xc * w[:, None]).T @ Xc
    A[np.diag_indices_from(A)] += alpha
    return np.concatenate([mu, ybar]), A, (Xc * w[:, None]).T @ Yc


class LinearRegressionPredictor:
    """A linear regressor (``coef`` [T][F] or [F], ``intercept`` [T], a scalar
    or None) on one device: ``predict`` is ``X coef^T + intercept`` in fp64
    through ``linear_predict``. Build with :meth:`from_sklearn`."""

    def __init__(self, coef, intercept, device=None):
        coef = np.asarray(coef, dtype=np.float64)
        self.single = coef.ndim == 1           # sklearn's shapes for a 1-D y
        coef = np.ascontiguousarray(np.atleast_2d(coef))
        if coef.ndim != 2 or not 1 <= coef.shape[1] <= MAX_FEATURES:
            raise ValueError(f"coef is {coef.shape}: [T][F] or [F] with 1..{MAX_FEATURES} features")
        if not 1 <= coef.shape[0] <= RIDGE_MAX_TARGETS:
            raise ValueError(f"{coef.shape[0]} targets: the kernels take 1..{RIDGE_MAX_TARGETS}")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.n_targets, self.n_features = coef.shape
        self._W_np = coef
        self._b_np = (None if intercept is None else np.array(
            np.broadcast_to(np.asarray(intercept, dtype=np.float64), (self.n_targets,))))
        self._ext = None
        if self.device.type == "cuda":
            self._ext = hip_ext(required=True)
            self._W = torch.from_numpy(coef).to(self.device)
            self._b = None if self._b_np is None else torch.from_numpy(self._b_np).to(self.device)

    @classmethod
    def from_sklearn(cls, est, device=None):
        from sklearn.linear_model import LinearRegression, Ridge

        if not isinstance(est, (Ridge, LinearRegression)) or not hasattr(est, "coef_"):
            raise TypeError(f"{type(est).__name__} is no fitted Ridge or LinearRegression")
        return cls(est.coef_, est.intercept_, device=device)

    def predict(self, X):
        """fp64 ``[B]`` (a 1-D ``coef``) or ``[B][T]``, a numpy array."""
        X = _rows(X, self.n_features).to(self.device)
        B = X.shape[0]
        scores = torch.empty(B, self.n_targets, dtype=torch.float64, device=self.device)
        if B > 0 and self._ext is not None:
            # the classifier's kernel as it is: its labels go to a throwaway buffer
            labels = torch.empty(B, dtype=torch.int32, device=self.device)
            self._ext.linear_predict(X, self._W, self._b, scores, None, labels, 0, 0)
        elif B > 0:
            z = X.numpy().astype(np.float64) @ self._W_np.T
            scores.copy_(torch.from_numpy(z if self._b_np is None else z + self._b_np))
        out = scores.cpu().numpy()
        return out[:, 0] if self.single else out


class DeviceRidge:
    """sklearn's ``Ridge(solver="cholesky")`` with the Gram matrix on the
    device: ``ridge_gram`` forms ``A = Xc^T S Xc + alpha I`` and
    ``Xy = Xc^T S Yc`` in fp64 from the fp32 X, the host solves
    ``scipy.linalg.solve(A, Xy, assume_a="pos")``, sklearn's own call. The
    primal form is used for N < F too. X is held in fp32 (see the module
    docstring)."""

    def __init__(self, alpha=1.0, fit_intercept=True, device=None):
        if not alpha >= 0:
            raise ValueError(f"alpha must be non-negative, is {alpha}")
        self.alpha, self.fit_intercept = float(alpha), bool(fit_intercept)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self._predictor = None

    def _gram(self, X, Y, sw, row_slices):
        """-> (mean, A, Xy) as numpy fp64, from the device or from numpy."""
        if self.device.type != "cuda":
            return gram_numpy(X.numpy().astype(np.float64), Y, sw, self.alpha, self.fit_intercept)
        ext, dev = hip_ext(required=True), self.device
        (N, F), T = X.shape, Y.shape[1]
        with torch.cuda.device(dev):
            slices, stride, moment_rows = ext.ridge_launch_shape(N, F, T, row_slices)
            f64 = dict(dtype=torch.float64, device=dev)
            mean, A, Xy = torch.empty(F + T, **f64), torch.empty(F, F, **f64), torch.empty(F, T, **f64)
            ext.ridge_gram(X.to(dev), torch.from_numpy(Y).to(dev),
                           None if sw is None else torch.from_numpy(sw).to(dev), self.alpha,
                           self.fit_intercept, mean, A, Xy,
                           torch.empty(slices * stride, **f64),
                           torch.empty(moment_rows, F + T + 1, **f64), row_slices)
            return mean.cpu().numpy(), A.cpu().numpy(), Xy.cpu().numpy()

    def fit(self, X, y, sample_weight=None, row_slices=0):
        """One ``ridge_gram`` call and one host solve. ``row_slices`` overrides
        the launcher's choice (tests)."""
        import scipy.linalg

        X = _rows(X)
        y = np.asarray(y, dtype=np.float64)
        N, F = X.shape
        if y.ndim not in (1, 2) or len(y) != N or N == 0:
            raise ValueError(f"y must be [{N}] or [{N}][T] with at least one row, is {y.shape}")
        Y = np.ascontiguousarray(y.reshape(N, -1))
        T = Y.shape[1]
        _refuse_beyond_ridge_limits(F, T)
        sw = None
        if sample_weight is not None:
            sw = np.ascontiguousarray(sample_weight, dtype=np.float64)
            if sw.shape != (N,) or not (sw >= 0).all() or not sw.sum() > 0:
                raise ValueError(f"sample_weight must be [{N}], non-negative with a positive sum")
        mean, A, Xy = self._gram(X, Y, sw, row_slices)
        try:
            coef = scipy.linalg.solve(A, Xy, assume_a="pos", overwrite_a=True).T
        except np.linalg.LinAlgError as exc:
            raise ValueError("the Gram matrix is singular (alpha = 0 on dependent columns?): "
                             "sklearn's SVD fallback is not served") from exc
        intercept = mean[F:] - coef @ mean[:F] if self.fit_intercept else np.zeros(T)
        if y.ndim == 1:
            self.coef_ = coef[0].copy()
            self.intercept_ = np.float64(intercept[0]) if self.fit_intercept else 0.0
        else:
            self.coef_ = np.ascontiguousarray(coef)
            self.intercept_ = intercept if self.fit_intercept else 0.0
        self.n_features_in_ = F
        self._predictor = LinearRegressionPredictor(
            self.coef_, self.intercept_ if self.fit_intercept else None, device=self.device)
        return self

    def predict(self, X):
        if self._predictor is None:
            raise ValueError("this DeviceRidge is not fitted yet")
        return self._predictor.predict(X)

    def to_sklearn(self):
        """A plain ``sklearn.linear_model.Ridge`` carrying the fitted
        attributes: what artifacts save and the serving code loads."""
        from sklearn.linear_model import Ridge

        if self._predictor is None:
            raise ValueError("this DeviceRidge is not fitted yet")
        est = Ridge(alpha=self.alpha, fit_intercept=self.fit_intercept, solver="cholesky")
        est.coef_ = self.coef_.copy()
        est.intercept_ = (self.intercept_.copy() if isinstance(self.intercept_, np.ndarray)
                          else self.intercept_)
        est.n_features_in_, est.n_iter_, est.solver_ = self.n_features_in_, None, "cholesky"
        return est


class _LinearRegressionCache(_LinearCache):
    """:class:`_LinearCache` for a fitted ``Ridge`` or ``LinearRegression``."""

    def __reduce__(self):
        return (_LinearRegressionCache, ())

    def get(self, est):
        if self.coef is not est.coef_ or self.intercept is not est.intercept_:
            self.predictor = LinearRegressionPredictor.from_sklearn(est)
            self.coef, self.intercept = est.coef_, est.intercept_
        return self.predictor


def device_linear_regressor(est):
    """The device predictor of a fitted sklearn ``Ridge`` or
    ``LinearRegression``, built once per fit and kept on the estimator."""
    cache = getattr(est, "_unionml_linear", None)
    if cache is None:
        cache = est._unionml_linear = _LinearRegressionCache()
    return cache.get(est)
