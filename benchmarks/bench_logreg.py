"""Logistic regression on the device against sklearn on the same machine.

Per shape (digits 1797 x 64 x 10 and a synthetic 60000 x 784 x 10):

* device time of one objective evaluation (the two launches, device events
  around ``--evals`` evaluations) under each cap on the workgroups (1x, 2x
  and 4x the CU count), warmed, several windows each, the variants
  alternating;
* wall time of a whole fit, warmed, median of ``--windows`` fits, for
  ``DeviceLogisticRegression`` and for ``LogisticRegression(solver="lbfgs")``
  at the same ``tol`` and ``max_iter``, with the ``n_iter_`` of both.

Needs a GPU. Prints one JSON document with the raw windows; ``--out`` also
writes it to a file.
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch


def shapes(which):
    from sklearn.datasets import load_digits

    if which in ("digits", "all"):
        d = load_digits()
        yield "digits", d.data.astype(np.float32), d.target
    if which in ("mnist", "all"):
        rng = np.random.default_rng(0)
        X = rng.random((60000, 784), dtype=np.float32)
        y = (X[:, :64] @ rng.standard_normal((64, 10))).argmax(axis=1)
        yield "synthetic-60000x784", X, y


def objective_timer(ext, Xd, yd, K, rb, max_wgs, evals):
    """-> (workgroups, a function timing one window: device milliseconds per
    evaluation over ``evals`` evaluations)."""
    N, F = Xd.shape
    W = torch.randn(K, F, dtype=torch.float64, device="cuda") * 0.01
    b = torch.zeros(K, dtype=torch.float64, device="cuda")
    _, grid = ext.logistic_launch_shape(N, rb, max_wgs)
    slabs = torch.empty(grid, K * F + K + 1, dtype=torch.float64, device="cuda")
    out = torch.empty(K * F + K + 1, dtype=torch.float64, device="cuda")

    def run(n):
        for _ in range(n):
            ext.logistic_loss_grad(Xd, yd, None, W, b, float(N), 1e-4, slabs, out, rb, max_wgs)

    def window():
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run(evals)
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / evals

    run(5)                            # warm-up
    torch.cuda.synchronize()
    return grid, window


def time_fit(make, X, y, windows):
    model = make().fit(X, y)          # warm-up
    times = []
    for _ in range(windows):
        t0 = time.perf_counter()
        model = make().fit(X, y)
        times.append(time.perf_counter() - t0)
    return model, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["digits", "mnist", "all"])
    ap.add_argument("--evals", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=1000)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--sklearn-windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_logreg.py needs a GPU"
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

    from sklearn.linear_model import LogisticRegression

    from unionml_amd.ops import hip_ext
    from unionml_amd.ops.linear import DeviceLogisticRegression

    ext = hip_ext(required=True)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    result = {"device": torch.cuda.get_device_name(0), "cus": cus, "shapes": {}}
    for name, X, y in shapes(args.shape):
        entry = {"rows": int(X.shape[0]), "features": int(X.shape[1]), "objective_ms": {}}
        Xd = torch.from_numpy(X).cuda()
        yd = torch.from_numpy(y.astype(np.int32)).cuda()
        rb = ext.LOGISTIC_RB
        timers = {f"rb{rb}-wgs{mult}x": objective_timer(ext, Xd, yd, int(y.max()) + 1, rb,
                                                        mult * cus, args.evals)
                  for mult in (1, 2, 4)}
        windows = {name: [] for name in timers}
        for _ in range(args.windows):          # the variants alternate window by window
            for variant, (_, window) in timers.items():
                windows[variant].append(window())
        for variant, (grid, _) in timers.items():
            entry["objective_ms"][variant] = {"grid": grid, "windows": windows[variant],
                                              "median": statistics.median(windows[variant])}
        del Xd, yd, timers
        kw = dict(tol=args.tol, max_iter=args.max_iter)
        dev, dev_t = time_fit(lambda: DeviceLogisticRegression(**kw), X, y, args.windows)
        X64 = X.astype(np.float64)
        ref, ref_t = time_fit(lambda: LogisticRegression(solver="lbfgs", **kw), X64, y,
                              args.sklearn_windows)
        entry["fit_s"] = {
            "device": {"windows": dev_t, "median": statistics.median(dev_t),
                       "n_iter": int(dev.n_iter_[0]), "evaluations": dev.n_evaluations_},
            "sklearn": {"windows": ref_t, "median": statistics.median(ref_t),
                        "n_iter": int(ref.n_iter_[0])}}
        entry["train_accuracy"] = {"device": float((dev.predict(X) == y).mean()),
                                   "sklearn": float((ref.predict(X64) == y).mean())}
        result["shapes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
