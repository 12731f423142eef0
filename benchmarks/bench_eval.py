#!/usr/bin/env python3
"""Device-side evaluation against the way the apps scored a model before
it (predict, every prediction copied to the host as a Python int, numpy
compare), and the cost of a validation pass inside a training epoch.

Per shape (digits 1,797 x 64->32->10 and MNIST 60,000 x 784->128->10):

  * eval_device_us / predict_device_us: hipGraph replays of the
    evaluation's launches (for the digits shape including the rebuild of
    the generalized weight image) and of the predict kernel on the same
    rows, timed with device events, windows alternated;
  * evaluate_wall_us / old_wall_us: ``evaluate(Xbf, y)`` and the old
    predictor + numpy path, each timed end to end on the host clock after
    a device sync (the old path's time is almost all host work);
  * epoch_us / epoch_val_us: the captured epoch of ``train_epochs``
    without and with ``validation`` on a 10 % split, replayed and timed
    with device events, windows alternated.

Prints one JSON line: the median and range of every figure over the
windows, and the windows themselves.

  python benchmarks/bench_eval.py [--windows 7] [--out FILE]
"""

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

SHAPES = {"digits": (1797, (64, 32, 10), 512), "mnist": (60000, (784, 128, 10), 512)}


def captured(fn):
    import torch

    fn()                      # eager warm-up: code objects, LDS attribute, buffers
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        fn()
    return gph.replay


def device_window(replay, replays):
    import torch

    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / replays


def wall_window(fn, reps):
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "windows": xs}


def bench_shape(name, n, shape, batch, windows):
    import numpy as np
    import torch

    from unionml_amd.ops.tabular import TabularMLP, split_validation

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    inf, hid, cls = shape
    y = torch.randint(0, cls, (n,), generator=gen, dtype=torch.int32)
    X = (torch.randn(cls, inf, generator=gen)[y.long()] + torch.randn(n, inf, generator=gen))
    X, y = X.to(dev), y.to(dev)
    y_np = y.cpu().numpy()

    clf = TabularMLP(*shape, device=dev, seed=0)
    clf.fit_standardizer(X)
    Xbf = clf.stage(X)
    clf.train_epochs(Xbf, y, epochs=2, batch_size=batch, lr=2e-3)

    # -- the same number two ways --------------------------------------------
    def old_way():
        preds = [int(i) for i in clf.predict(X).cpu()]
        return float((np.asarray(preds) == y_np).mean())

    new = clf.evaluate(Xbf, y)
    assert new["accuracy"] == old_way(), "the two ways disagree"

    clf._ensure_eval(n)
    hist, slot = clf._eval_one
    eval_replay = captured(lambda: clf._eval_launch(Xbf, y, hist, slot))
    predict_replay = captured(lambda: clf.predict(X))
    reps = 200 if n > 10000 else 2000
    out = {k: [] for k in ("eval_device_us", "predict_device_us", "evaluate_wall_us",
                           "old_wall_us")}
    for _ in range(windows):
        out["eval_device_us"].append(device_window(eval_replay, reps))
        out["predict_device_us"].append(device_window(predict_replay, reps))
        out["evaluate_wall_us"].append(wall_window(lambda: clf.evaluate(Xbf, y), 20))
        out["old_wall_us"].append(wall_window(old_way, 3 if n > 10000 else 10))

    # -- an epoch with and without validation on a 10 % split -----------------
    tr, va = split_validation(n, 0.1)
    tr, va = tr.to(dev), va.to(dev)
    Xt, yt, Xv, yv = Xbf[tr].contiguous(), y[tr].contiguous(), Xbf[va].contiguous(), \
        y[va].contiguous()
    plain = TabularMLP(*shape, device=dev, seed=0)
    withv = TabularMLP(*shape, device=dev, seed=0)
    for m in (plain, withv):
        m.mean.copy_(clf.mean)
        m.invstd.copy_(clf.invstd)
    plain.train_epochs(Xt, yt, epochs=2, batch_size=batch, lr=2e-3)
    withv.train_epochs(Xt, yt, epochs=2, batch_size=batch, lr=2e-3, validation=(Xv, yv))
    assert plain._graph is not None and withv._graph is not None
    out["epoch_us"], out["epoch_val_us"] = [], []
    ereps = 20 if n > 10000 else 200
    for _ in range(windows):
        out["epoch_us"].append(device_window(plain._graph.replay, ereps))
        out["epoch_val_us"].append(device_window(withv._graph.replay, ereps))

    res = {k: summary(v) for k, v in out.items()}
    res.update(rows=n, shape=list(shape), batch=batch, val_rows=int(len(va)),
               steps_per_epoch=-(-int(len(tr)) // batch), accuracy=new["accuracy"])
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--out", default=None, help="also write the JSON line here")
    args = p.parse_args()

    import torch

    assert torch.cuda.is_available(), "needs a GPU"
    result = {"device": torch.cuda.get_device_name(0)}
    for name, (n, shape, batch) in SHAPES.items():
        result[name] = bench_shape(name, n, shape, batch, args.windows)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
