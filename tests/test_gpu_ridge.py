"""ridge_gram (hip/linear_gram.hip) against the longdouble reference under the
derived bounds of docs/kernels.md "Ridge regression", DeviceRidge against
sklearn's own fit, and the ridge app on the device."""

from functools import lru_cache

import numpy as np
import pytest
import torch

from ridge_reference import (FIT_PROBLEMS, difference, fit_problem, fit_tolerance, gram_case,
                             gram_reference, mean_reference, predict_bound)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (63, 63, 1), (65, 64, 3), (131, 65, 17), (259, 130, 32), (67, 129, 2)]
ALPHA = 0.37
POISON = -7.25


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    return hip_ext(required=True)


@lru_cache(maxsize=None)
def case(N, F, T):
    X, Y, sw = gram_case(N, F, T)
    return (X, Y, sw), tuple(torch.from_numpy(a).cuda() for a in (X, Y, sw))


def run_gram(ext, dev, weighted, center, row_slices):
    Xd, Yd, swd = dev
    (N, F), T = Xd.shape, Yd.shape[1]
    slices, stride, moment_rows = ext.ridge_launch_shape(N, F, T, row_slices)
    full = lambda *shape: torch.full(shape, POISON, dtype=torch.float64, device="cuda")
    mean, A, Xy = full(F + T), full(F, F), full(F, T)
    ext.ridge_gram(Xd, Yd, swd if weighted else None, ALPHA, center, mean, A, Xy,
                   full(slices * stride), full(moment_rows, F + T + 1), row_slices)
    return mean, A, Xy


@pytest.mark.parametrize("row_slices", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_within_the_derived_bound(ext, shape, row_slices):
    (X, Y, sw), dev = case(*shape)
    for weighted in (False, True):
        for center in (False, True):
            w = sw if weighted else None
            mean, A, Xy = run_gram(ext, dev, weighted, center, row_slices)
            assert torch.equal(A, A.T)
            mean, A, Xy = (a.cpu().numpy() for a in (mean, A, Xy))
            ref_mean, tol_mean = mean_reference(X, Y, w, center)
            ref_A, ref_Xy, tol_A, tol_Xy = gram_reference(X, Y, w, ALPHA, mean)
            err_mean = np.abs(mean - ref_mean).astype(np.float64)
            err_A, err_Xy = (np.abs(A - ref_A).astype(np.float64),
                             np.abs(Xy - ref_Xy).astype(np.float64))
            share = lambda err, tol: float((err[tol > 0] / tol[tol > 0]).max(initial=0.0))
            print(shape, row_slices, weighted, center, "mean", share(err_mean, tol_mean),
                  "A", share(err_A, tol_A), "Xy", share(err_Xy, tol_Xy))
            assert (err_mean <= tol_mean).all()
            assert (err_A <= tol_A).all()
            assert (err_Xy <= tol_Xy).all()


def test_same_call_same_bits(ext):
    _, dev = case(259, 130, 32)
    first, again = run_gram(ext, dev, True, True, 3), run_gram(ext, dev, True, True, 3)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


@pytest.mark.parametrize("broken", ["dtype", "host", "t33", "short_A", "aliased"])
def test_binding_preconditions(ext, broken):
    N, F, T = 65, 64, 3
    _, (Xd, Yd, _) = case(N, F, T)
    # X and A are parts of one buffer, apart unless the case overlaps them
    buf = torch.full((N * F // 2 + F * F,), POISON, dtype=torch.float64, device="cuda")
    buf[:N * F // 2].view(torch.float32).copy_(Xd.view(-1))
    args = dict(X=buf[:N * F // 2].view(torch.float32).view(N, F), Y=Yd.clone(),
                A=buf[N * F // 2:].view(F, F))
    if broken == "dtype":
        args["X"] = args["X"].double()
    elif broken == "host":
        args["Y"] = args["Y"].cpu()
    elif broken == "t33":
        args["Y"] = torch.zeros(N, 33, dtype=torch.float64, device="cuda")
    elif broken == "short_A":
        args["A"] = args["A"][:-1]
    elif broken == "aliased":
        args["A"] = buf[N * F // 2 - 1:-1].view(F, F)
    kept = {k: v.clone() for k, v in args.items()}
    full = lambda *shape: torch.full(shape, POISON, dtype=torch.float64, device="cuda")
    Tb = args["Y"].shape[1]                   # every other buffer fits the call
    outs = [full(F + Tb), full(F, Tb), full(4 * (64 * 64 + 64 * 32)), full(2, F + Tb + 1)]
    with pytest.raises(RuntimeError):
        ext.ridge_gram(args["X"], args["Y"], None, ALPHA, True, outs[0], args["A"], *outs[1:])
    torch.cuda.synchronize()
    assert all(torch.equal(v, kept[k]) for k, v in args.items())
    assert all((o == POISON).all() for o in outs)


@pytest.mark.parametrize("problem", FIT_PROBLEMS, ids=lambda p: "x".join(map(str, p[:3])))
def test_device_fit_matches_sklearn(problem):
    """Against sklearn's Ridge(solver="cholesky") on the same data, within ten
    times sklearn's own sensitivity to row order (floor 1e-12). Measured on an
    MI355X: the sensitivities are 1.7e-15, 1.6e-15 and 3.1e-15, the device
    differences 1.3e-15, 1.2e-15 and 2.7e-15."""
    from unionml_amd.ops.linear import DeviceRidge

    X, y, sw = fit_problem(*problem)
    base, tol, sensitivity = fit_tolerance(X, y, sw, problem[4])
    model = DeviceRidge(alpha=1.0, fit_intercept=problem[4], device="cuda").fit(X, y, sw)
    diff = difference(model, base)
    served, scored = model.to_sklearn().predict(X.astype(np.float64)), model.predict(X)
    eps_z = predict_bound(X, model.coef_, model.intercept_)
    print(problem, "sensitivity", sensitivity, "tolerance", tol, "device difference", diff,
          "predict", np.abs(served - scored).max() / eps_z, "of eps_z", eps_z)
    assert model.coef_.shape == base.coef_.shape
    assert diff <= tol
    assert served.shape == scored.shape and np.abs(served - scored).max() <= eps_z


def test_ridge_app_trains_and_predicts_on_the_device():
    from sklearn.linear_model import Ridge
    from sklearn.metrics import r2_score

    from unionml_amd.models import ridge

    ridge.model.artifact = None
    reg, metrics = ridge.model.train()
    assert type(reg) is Ridge
    # sklearn in fp64: on the fp32 frame as it is, Ridge would compute in fp32
    splits = {name: (features, target.squeeze().astype(np.float64))
              for name, (features, target) in ridge.dataset.get_data(ridge.reader()).items()}
    host = Ridge().fit(splits["train"][0].astype(np.float64), splits["train"][1])
    for name, (features, target) in splits.items():
        want = r2_score(target, host.predict(features.astype(np.float64)))
        served = r2_score(target, ridge.model.predict(features=features))
        print(name, "R2 device", served, "evaluator", metrics[name], "sklearn", want)
        assert abs(served - want) <= 1e-9 and abs(metrics[name] - want) <= 1e-9
