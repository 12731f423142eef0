#!/usr/bin/env python3
"""Step time of the regression head against the classifier head on one
geometry: hipGraph-replayed fused steps (step kernel + reduce/Adam), timed
with device events, the two heads ALTERNATED window by window in one process
so that drift hits both alike. Prints one JSON line with every window.

  python benchmarks/bench_reg_step.py --shape 256x64x16 --batch 512

``--tree DIR`` imports unionml_amd from another checkout (one that carries
its own built extension), e.g. the parent commit's; a tree without
TabularMLPRegressor is timed on the classifier alone.
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

GRAPH_STEPS = 16   # optimizer steps captured per graph, one per minibatch


def make_runner(model, Xbf, targets, B):
    """Capture GRAPH_STEPS fused steps over distinct minibatches; returns
    replay()"""
    import torch

    g = model.g
    rpw = model._rows_per_wg(B)
    model._ensure_slabs((B + rpw - 1) // rpw)
    loss_out = model.grads[g.nparam : g.nparam + 1]

    def epoch():
        for i in range(GRAPH_STEPS):
            off = i * B
            model._fused_adam_step(Xbf[off : off + B], targets[off : off + B], 1.0 / B,
                                   1e-3, loss_out)

    epoch()   # eager warm-up: code objects, LDS attribute
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        epoch()
    return gph.replay


def window(replay, replays):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / (replays * GRAPH_STEPS)   # us/step


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shape", default="256x64x16")
    p.add_argument("--batch", type=int, default=512)
    p.add_argument("--replays", type=int, default=2000, help="graph replays per window")
    p.add_argument("--windows", type=int, default=7, help="timed windows per head")
    p.add_argument("--tree", default=None, help="import unionml_amd from this checkout")
    args = p.parse_args()
    sys.path.insert(0, args.tree or str(Path(__file__).resolve().parent.parent))

    import torch

    import unionml_amd.ops.tabular as tab

    inf, hid, out = (int(x) for x in args.shape.split("x"))
    B, n = args.batch, args.batch * GRAPH_STEPS
    gen = torch.Generator().manual_seed(0)
    X = torch.randn(n, inf, generator=gen) * torch.linspace(0.5, 2.0, inf) + 0.3

    runners = {}
    clf = tab.TabularMLP(in_features=inf, hidden=hid, classes=out, device="cuda:0", seed=0)
    clf.fit_standardizer(X)
    y = torch.randint(0, out, (n,), generator=gen, dtype=torch.int32).to(clf.device)
    runners["classifier"] = make_runner(clf, clf.stage(X), y, B)
    if hasattr(tab, "TabularMLPRegressor"):
        reg = tab.TabularMLPRegressor(in_features=inf, hidden=hid, targets=out,
                                      device="cuda:0", seed=0)
        Y = torch.randn(n, out, generator=gen) * torch.linspace(0.5, 2.0, out)
        reg.fit_standardizer(X)
        reg.fit_target_standardizer(Y)
        runners["regression"] = make_runner(reg, reg.stage(X), reg.stage_targets(Y), B)

    times = {name: [] for name in runners}
    for name, replay in runners.items():   # warm every shape the windows use
        window(replay, max(1, args.replays // 4))
    for _ in range(args.windows):
        for name, replay in runners.items():
            times[name].append(round(window(replay, args.replays), 3))

    res = {"shape": args.shape, "batch": B, "graph_steps": GRAPH_STEPS,
           "steps_per_window": args.replays * GRAPH_STEPS,
           "rows_per_wg": clf._rows_per_wg(B), "tree": args.tree or "."}
    for name, ts in times.items():
        res[name] = {"us_per_step_median": round(statistics.median(ts), 3),
                     "min": min(ts), "max": max(ts), "windows": ts}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
