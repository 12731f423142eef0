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

``--walk chunked|split`` forces ``forest_predict_kernel`` or the split walk
(docs/kernels.md "Split walk"); without it the predictor chooses, as the apps'
calls do. ``--grown`` scores a regressor of three trees grown to one sample a
leaf on 3,000 x 6 rows (5,999 nodes a tree) instead, which only the split
walk serves; it has no visit counts.

  python benchmarks/bench_forest.py [--windows 7] [--walk split] [--grown] [--rows 1,64]
      [--out FILE]
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
    p.add_argument("--walk", choices=("chunked", "split"), default=None,
                   help="force a path (default: the predictor's choice)")
    p.add_argument("--grown", action="store_true", help="the 5,999-node regressor")
    p.add_argument("--rows", default=",".join(map(str, BATCHES)),
                   help="batch sizes, comma-separated")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    args = p.parse_args()
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

    import numpy as np
    import torch
    from sklearn.datasets import load_digits
    from sklearn.ensemble import HistGradientBoostingClassifier, HistGradientBoostingRegressor

    from unionml_amd.ops.forest import ForestPredictor

    assert torch.cuda.is_available(), "needs a GPU"
    digits = load_digits()
    X0 = digits.data.astype(np.float32)
    if args.grown:
        rng = np.random.RandomState(17)
        X0 = rng.randn(3000, 6).astype(np.float32)
        est = HistGradientBoostingRegressor(max_iter=3, max_leaf_nodes=None,
                                            min_samples_leaf=1).fit(
            X0, X0[:, :3].sum(axis=1) + 0.3 * rng.randn(3000))
        sklearn_scores = lambda X: est.predict(X).reshape(-1, 1)          # noqa: E731
    else:
        est = HistGradientBoostingClassifier(max_iter=args.iterations, random_state=0).fit(
            X0, digits.target)
        sklearn_scores = est.decision_function
    forest = ForestPredictor.from_sklearn(est, device="cuda")
    # node visits are counted on the 16-byte packing, which the grown forest lacks
    count = (lambda X: forest._walk_cpu(X)[1]) if forest._nodes_np is not None else (lambda X: 0)
    visits0 = count(X0)
    result = {"device": torch.cuda.get_device_name(0), "trees": forest.n_trees,
              "nodes": int(len(forest._split_nodes_np)), "max_tree_nodes": forest.max_tree_nodes,
              "rows_per_wg": forest.rows_per_wg,
              "visits_per_row": visits0 / len(X0), "batches": {}}
    if args.walk or args.grown:
        result["walk"] = args.walk or forest.walk_for(1)
    score = lambda Xd: forest.decision_function(Xd, walk=args.walk)       # noqa: E731
    for B in map(int, args.rows.split(",")):
        reps = -(-B // len(X0))
        X = np.tile(X0, (reps, 1))[:B]
        rest = B % len(X0)
        visits = visits0 * (B // len(X0)) + (count(X0[:rest]) if rest else 0)
        Xd = torch.from_numpy(X).cuda()
        want = sklearn_scores(X)
        got = score(Xd)
        assert torch.equal(got.cpu(), torch.from_numpy(want)), "the kernel disagrees"
        calls = 20 if B > 10000 else 500
        device_window(lambda: score(Xd), calls)        # warm
        windows = [device_window(lambda: score(Xd), calls) for _ in range(args.windows)]
        host = []
        for _ in range(3):
            t = time.perf_counter()
            sklearn_scores(X)
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
