"""Ridge regression on the device against sklearn and against the library's
fp64 product on the same machine.

Per shape (diabetes 442 x 10 x 1 and a seeded synthetic 60000 x 784 x 10):

* device time of one ``ridge_gram`` call (its four launches, device events
  around ``--calls`` calls), warmed, several windows;
* the device yardstick: torch's fp64 ``Xc^T Xc`` (and ``Xc^T Yc``) on the
  device, once on a prepared fp64 centred, weighted copy and once with the time
  to build that copy from the fp32 X;
* wall time of a whole ``DeviceRidge.fit`` and of sklearn's
  ``Ridge(solver="cholesky")`` on the CPU, warmed, medians of ``--windows`` fits;
* achieved fp64 FLOP/s: N F (F + 64) / 2 + N F T multiply-adds over the kernel
  time, against ``--peak-tflops``.

Needs a GPU. Prints one JSON document with the raw windows; ``--out`` writes
it to a file and ``--md`` a table of medians and ranges.
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
    if which in ("diabetes", "all"):
        from sklearn.datasets import load_diabetes

        d = load_diabetes()
        yield "diabetes-442x10x1", d.data.astype(np.float32), d.target.astype(np.float64)
    if which in ("synthetic", "all"):
        rng = np.random.default_rng(0)
        X = rng.random((60000, 784), dtype=np.float32)
        Y = X[:, :64].astype(np.float64) @ rng.standard_normal((64, 10)) + \
            rng.standard_normal((60000, 10))
        yield "synthetic-60000x784x10", X, Y


def device_windows(run, calls, windows):
    """Device milliseconds a call over ``calls`` calls, ``windows`` times, warmed."""
    run(3)
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        run(calls)
        stop.record()
        stop.synchronize()
        out.append(start.elapsed_time(stop) / calls)
    return out


def wall_windows(fit, windows):
    fit()                                  # warm-up
    out = []
    for _ in range(windows):
        t0 = time.perf_counter()
        fit()
        out.append(time.perf_counter() - t0)
    return out


def summary(values):
    return {"windows": values, "median": statistics.median(values), "min": min(values),
            "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="all", choices=["diabetes", "synthetic", "all"])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=78.6,
                    help="fp64 matrix peak of the device (MI355X: 78.6)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ridge.py needs a GPU"
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

    from sklearn.linear_model import Ridge

    from unionml_amd.ops import hip_ext
    from unionml_amd.ops.linear import DeviceRidge

    ext = hip_ext(required=True)
    result = {"device": torch.cuda.get_device_name(0),
              "cus": torch.cuda.get_device_properties(0).multi_processor_count,
              "peak_tflops": args.peak_tflops, "shapes": {}}
    f64 = dict(dtype=torch.float64, device="cuda")
    for name, X, y in shapes(args.shape):
        Y = y.reshape(len(y), -1)
        (N, F), T = X.shape, Y.shape[1]
        Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        slices, stride, moment_rows = ext.ridge_launch_shape(N, F, T, 0)
        mean, A, Xy = torch.empty(F + T, **f64), torch.empty(F, F, **f64), torch.empty(F, T, **f64)
        slabs = torch.empty(slices * stride, **f64)
        moment_slabs = torch.empty(moment_rows, F + T + 1, **f64)

        def kernel(n):
            for _ in range(n):
                ext.ridge_gram(Xd, Yd, None, 1.0, True, mean, A, Xy, slabs, moment_slabs, 0)

        def prepared():
            X64, Y64 = Xd.double(), Yd
            return X64 - X64.mean(dim=0), Y64 - Y64.mean(dim=0)

        Xc, Yc = prepared()

        def product(n):
            for _ in range(n):
                Xc.T @ Xc
                Xc.T @ Yc

        def product_with_copy(n):
            for _ in range(n):
                xc, yc = prepared()
                xc.T @ xc
                xc.T @ yc

        entry = {"rows": N, "features": F, "targets": T, "row_slices": slices,
                 "ridge_gram_ms": summary(device_windows(kernel, args.calls, args.windows)),
                 "torch_product_ms": summary(device_windows(product, args.calls, args.windows)),
                 "torch_product_with_copy_ms": summary(
                     device_windows(product_with_copy, args.calls, args.windows))}
        macs = N * F * (F + 64) / 2 + N * F * T
        tflops = 2 * macs / (entry["ridge_gram_ms"]["median"] * 1e-3) / 1e12
        entry["ridge_gram_tflops"] = tflops
        entry["share_of_peak"] = tflops / args.peak_tflops
        ref = Ridge(solver="cholesky").fit(X.astype(np.float64), y)
        kernel(1)
        diff = float((A.cpu() - torch.from_numpy(ref.alpha * np.eye(F))
                      - (Xc.T @ Xc).cpu()).abs().max())
        entry["max_abs_A_minus_torch"] = diff
        del Xc, Yc, slabs
        X64 = X.astype(np.float64)
        entry["fit_s"] = {
            "device": summary(wall_windows(lambda: DeviceRidge().fit(X, y), args.windows)),
            "sklearn": summary(wall_windows(lambda: Ridge(solver="cholesky").fit(X64, y),
                                            args.windows))}
        dev = DeviceRidge().fit(X, y)
        entry["max_abs_coef_minus_sklearn"] = float(np.abs(dev.coef_ - ref.coef_).max())
        result["shapes"][name] = entry
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text)
    if args.md:
        rows = ["| shape | row slices | `ridge_gram` ms | torch fp64 product ms | the same with "
                "its copy ms | `DeviceRidge.fit` s | sklearn cholesky s | fp64 TFLOP/s "
                "(share of peak) |", "|---|---|---|---|---|---|---|---|"]
        cell = lambda s, d: f"{s['median']:.{d}f} ({s['min']:.{d}f}–{s['max']:.{d}f})"
        for name, e in result["shapes"].items():
            rows.append(f"| {name} | {e['row_slices']} | {cell(e['ridge_gram_ms'], 4)} | "
                        f"{cell(e['torch_product_ms'], 4)} | "
                        f"{cell(e['torch_product_with_copy_ms'], 4)} | "
                        f"{cell(e['fit_s']['device'], 4)} | {cell(e['fit_s']['sklearn'], 4)} | "
                        f"{e['ridge_gram_tflops']:.2f} ({100 * e['share_of_peak']:.1f} %) |")
        Path(args.md).write_text("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
