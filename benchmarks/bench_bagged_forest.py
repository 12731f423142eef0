#!/usr/bin/env python3
"""Bagged-forest inference: the random-forest app's digits forest (100 trees,
10 classes) and one deep forest (extra-trees regressor, 10 trees grown out on
50,000 x 20 random rows) scored by ``bagged_forest_predict_kernel`` and by
sklearn on the host.

Per forest and batch size (1, 64, 1,797 and 262,144 rows: the training rows,
repeated):

  * kernel_us: device time of one ``BaggedForestPredictor`` call on rows
    already on the device, from events around a warmed window of calls;
    median, min and max of ``--windows`` windows;
  * kernel_no_prefix_us: the same with ``prefix_nodes=0`` (every node visit
    reads global memory), i.e. what the LDS prefix buys;
  * sklearn_us: wall time of ``est.predict_proba`` / ``est.predict`` on the
    same rows with ``n_jobs`` = ``--jobs`` (best of three);
  * rows/s and node visits/s of the kernel. The visit count (nodes read,
    leaves included) comes from sklearn's ``decision_path``.

The kernel's result is first held equal to sklearn's at ``n_jobs=None``, bit
for bit. Needs a GPU; prints one JSON line.

  python benchmarks/bench_bagged_forest.py [--windows 7] [--jobs 16] [--out FILE]
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

BATCHES = (1, 64, 1797, 262144)


def device_window(fn, calls):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / calls


def measure(name, est, X0, args):
    import numpy as np
    import torch

    from unionml_amd.ops.forest import BaggedForestPredictor

    forest = BaggedForestPredictor.from_sklearn(est, device="cuda")
    public = "predict_proba" if hasattr(est, "classes_") else "predict"
    sample = X0[:1797]
    visits_per_row = sum(int(e.decision_path(sample).nnz) for e in est.estimators_) / len(sample)
    result = {"forest": name, "trees": forest.n_trees, "nodes": int(len(forest._nodes_np)),
              "max_tree_nodes": forest.max_tree_nodes, "rows_per_wg": forest.rows_per_wg,
              "visits_per_row": visits_per_row, "batches": {}}
    for B in BATCHES:
        X = np.tile(X0, (-(-B // len(X0)), 1))[:B]
        Xd = torch.from_numpy(X).cuda()
        est.set_params(n_jobs=None)
        want = np.asarray(getattr(est, public)(X), dtype=np.float64).reshape(B, -1)
        got = forest._score(Xd)[0]
        assert torch.equal(got.cpu(), torch.from_numpy(want)), "the kernel disagrees"
        assert torch.equal(forest._score(Xd, prefix_nodes=0)[0], got)
        calls = 20 if B > 10000 else 300
        timed = {}
        for key, prefix in (("kernel_us", -1), ("kernel_no_prefix_us", 0)):
            device_window(lambda: forest._score(Xd, prefix_nodes=prefix), calls)      # warm
            w = [device_window(lambda: forest._score(Xd, prefix_nodes=prefix), calls)
                 for _ in range(args.windows)]
            timed[key] = {"median": statistics.median(w), "min": min(w), "max": max(w)}
        est.set_params(n_jobs=args.jobs)
        host = []
        for _ in range(3):
            t = time.perf_counter()
            getattr(est, public)(X)
            host.append((time.perf_counter() - t) * 1e6)
        med = timed["kernel_us"]["median"]
        result["batches"][str(B)] = {
            **timed, "sklearn_us": {"best": min(host), "runs": host, "n_jobs": args.jobs},
            "rows_per_s": B / (med * 1e-6),
            "visits_per_s": visits_per_row * B / (med * 1e-6),
            "sklearn_over_kernel": min(host) / med}
    return result


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--jobs", type=int, default=16, help="n_jobs of the sklearn timing")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    args = p.parse_args()
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

    import numpy as np
    import torch
    from sklearn.datasets import load_digits
    from sklearn.ensemble import ExtraTreesRegressor, RandomForestClassifier

    assert torch.cuda.is_available(), "needs a GPU"
    digits = load_digits()
    X0 = digits.data.astype(np.float32)
    app = RandomForestClassifier(n_estimators=100, random_state=0, n_jobs=args.jobs).fit(
        X0, digits.target)
    rng = np.random.RandomState(0)
    X1 = rng.randn(50000, 20).astype(np.float32)
    deep = ExtraTreesRegressor(n_estimators=10, random_state=0, n_jobs=args.jobs).fit(
        X1, X1[:, :5].sum(axis=1) + rng.randn(50000))
    result = {"device": torch.cuda.get_device_name(0),
              "forests": [measure("digits_rf100", app, X0, args),
                          measure("deep_et10", deep, X1, args)]}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
