#!/usr/bin/env python3
"""Forest inference: the boosting app's digits forest (100 iterations x 10
classes) scored by ``forest_predict_kernel`` and by sklearn on the host.

Per batch size (1, 64, 1,797 and 262,144 rows: sklearn's digits, repeated):

  * kernel_us: device time of one ``ForestPredictor.decision_function`` call
    on rows already on the device, from events around a warmed window of
    calls; median, min and max of ``--windows`` windows;
  * sklearn_us: wall time of ``est.decision_function`` on the same rows on
    this machine's CPUs (best of three; the thread count is the
    environment's);
  * rows/s and node visits/s of the kernel. The visit count (nodes read,
    leaves included) comes from walking the packed forest on the host.

The kernel's scores are first held equal to sklearn's, bit for bit. Needs a
GPU; prints one JSON line.

  python benchmarks/bench_forest.py [--windows 7] [--out FILE]
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--iterations", type=int, default=100)
    p.add_argument("--out", default=None, help="also write the JSON line here")
    args = p.parse_args()
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

    import numpy as np
    import torch
    from sklearn.datasets import load_digits
    from sklearn.ensemble import HistGradientBoostingClassifier

    from unionml_amd.ops.forest import ForestPredictor

    assert torch.cuda.is_available(), "needs a GPU"
    digits = load_digits()
    X0 = digits.data.astype(np.float32)
    est = HistGradientBoostingClassifier(max_iter=args.iterations, random_state=0).fit(
        X0, digits.target)
    forest = ForestPredictor.from_sklearn(est, device="cuda")
    _, visits0 = forest._walk_cpu(X0)
    result = {"device": torch.cuda.get_device_name(0), "trees": forest.n_trees,
              "nodes": int(len(forest._nodes_np)), "max_tree_nodes": forest.max_tree_nodes,
              "rows_per_wg": forest.rows_per_wg,
              "visits_per_row": visits0 / len(X0), "batches": {}}
    for B in BATCHES:
        reps = -(-B // len(X0))
        X = np.tile(X0, (reps, 1))[:B]
        rest = B % len(X0)
        visits = visits0 * (B // len(X0)) + (forest._walk_cpu(X0[:rest])[1] if rest else 0)
        Xd = torch.from_numpy(X).cuda()
        want = est.decision_function(X)
        got = forest.decision_function(Xd)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), "the kernel disagrees"
        calls = 20 if B > 10000 else 500
        device_window(lambda: forest.decision_function(Xd), calls)        # warm
        windows = [device_window(lambda: forest.decision_function(Xd), calls)
                   for _ in range(args.windows)]
        host = []
        for _ in range(3):
            t = time.perf_counter()
            est.decision_function(X)
            host.append((time.perf_counter() - t) * 1e6)
        med = statistics.median(windows)
        result["batches"][str(B)] = {
            "kernel_us": {"median": med, "min": min(windows), "max": max(windows)},
            "sklearn_us": {"best": min(host), "runs": host},
            "rows_per_s": B / (med * 1e-6), "visits": visits,
            "visits_per_s": visits / (med * 1e-6),
            "sklearn_over_kernel": min(host) / med}
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
