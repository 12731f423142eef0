#!/usr/bin/env python3
"""Shuffled epochs: what the shuffle launch costs, and what it buys.

``--mode kernel`` (GPU). Per shape (digits 1,797 x 64 and MNIST 60,000 x
784, staged bf16 rows plus int32 labels), hipGraph replays timed with device
events, windows alternated:

  * shuffle_us: the ``shuffle_rows`` launch;
  * copy_us: plain device-to-device ``copy_`` of the same bytes (features
    and labels, two launches);
  * index_select_us: ``torch.index_select`` of both by a permutation already
    on the device (two launches);

and the achieved GB/s of each, counting every byte once read and once
written.

``--mode epoch`` (GPU). The captured epoch of ``train_epochs`` at both
shapes, replayed and timed with device events: ``shuffle`` off and on
(``--variants``), windows alternated. ``--tree DIR`` imports unionml_amd from
another checkout that carries its own built extension, e.g. the parent
commit's (timed with ``shuffle`` off alone); run the two trees in
alternating processes, each with ``--variants off``, to see the repeat
spread: a second model in the process competes for the Infinity Cache,
which holds the whole MNIST-shaped set between replays when it is alone.

``--mode accuracy`` (CPU path, runs anywhere). Held-out accuracy (digits
classifier, on sklearn's digits as they come and sorted by label; an
MNIST-shaped 784->128->10 classifier on synthetic clusters) and held-out R2
(the regressor on synthetic targets), five init seeds each, ``shuffle`` off
and on. A report, no threshold.

Prints one JSON line.

  python benchmarks/bench_shuffle.py --mode kernel [--windows 7] [--out FILE]
"""

import argparse
import json
import statistics
import sys
from pathlib import Path

SHAPES = {"digits": (1797, (64, 32, 10), 512), "mnist": (60000, (784, 128, 10), 512)}


def captured(fn):
    import torch

    fn()                      # eager warm-up: code objects, buffers
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


def summary(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "windows": xs}


def synthetic(n, shape, dev):
    import torch

    gen = torch.Generator().manual_seed(0)
    inf, _, cls = shape
    y = torch.randint(0, cls, (n,), generator=gen, dtype=torch.int32)
    X = torch.randn(cls, inf, generator=gen)[y.long()] + torch.randn(n, inf, generator=gen)
    return X.to(dev), y.to(dev)


# ---------------------------------------------------------------------------
# kernel
# ---------------------------------------------------------------------------


def bench_kernel(n, shape, windows):
    import torch

    from unionml_amd.ops import hip_ext
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import TabularMLP

    dev = torch.device("cuda:0")
    ext = hip_ext(required=True)
    X, y = synthetic(n, shape, dev)
    clf = TabularMLP(*shape, device=dev, seed=0)
    clf.fit_standardizer(X)
    Xbf = clf.stage(X)
    Xs, ys = torch.empty_like(Xbf), torch.empty_like(y)
    t_dev = torch.tensor([3], dtype=torch.int32, device=dev)
    perm = ref.shuffle_perm(n, 0, 3).to(dev)

    def shuffle():
        ext.shuffle_rows(Xbf, y, Xs, ys, t_dev, 0)

    def copy():
        Xs.copy_(Xbf)
        ys.copy_(y)

    def index_select():
        torch.index_select(Xbf, 0, perm, out=Xs)
        torch.index_select(y, 0, perm, out=ys)

    index_select()
    want = (Xs.clone(), ys.clone())
    shuffle()
    torch.cuda.synchronize()
    assert torch.equal(Xs, want[0]) and torch.equal(ys, want[1]), "the kernel disagrees"

    replays = {"shuffle_us": captured(shuffle), "copy_us": captured(copy),
               "index_select_us": captured(index_select)}
    reps = 200 if n > 10000 else 2000
    out = {k: [] for k in replays}
    for _ in range(windows):
        for k, replay in replays.items():
            out[k].append(device_window(replay, reps))
    res = {k: summary(v) for k, v in out.items()}
    moved = 2 * (Xbf.numel() * 2 + y.numel() * 4)     # read once, written once
    res["bytes_moved"] = moved
    for k in replays:
        res[k.replace("_us", "_GBps")] = moved / (res[k]["median"] * 1e-6) / 1e9
    res["shuffle_over_copy"] = res["shuffle_us"]["median"] / res["copy_us"]["median"]
    res["shuffle_over_index_select"] = (
        res["shuffle_us"]["median"] / res["index_select_us"]["median"])
    res.update(rows=n, inp=int(Xbf.shape[1]))
    return res


# ---------------------------------------------------------------------------
# epoch
# ---------------------------------------------------------------------------


def bench_epoch(n, shape, batch, windows, variants):
    import torch

    from unionml_amd.ops.tabular import TabularMLP

    dev = torch.device("cuda:0")
    X, y = synthetic(n, shape, dev)
    models = {}
    for name in variants:
        m = TabularMLP(*shape, device=dev, seed=0)
        m.fit_standardizer(X)
        Xbf = m.stage(X)
        kw = dict(shuffle=True, shuffle_seed=1) if name == "on" else {}
        m.train_epochs(Xbf, y, epochs=2, batch_size=batch, lr=2e-3, **kw)
        assert m._graph is not None
        models[name] = (m, Xbf)       # Xbf stays alive: the graph holds its address
    reps = 20 if n > 10000 else 200
    out = {f"epoch_{k}_us": [] for k in models}
    for _ in range(windows):
        for k, (m, _) in models.items():
            out[f"epoch_{k}_us"].append(device_window(m._graph.replay, reps))
    res = {k: summary(v) for k, v in out.items()}
    res.update(rows=n, shape=list(shape), batch=batch, steps_per_epoch=-(-n // batch))
    return res


# ---------------------------------------------------------------------------
# accuracy (CPU path)
# ---------------------------------------------------------------------------


def _split(n, seed=0):
    import torch

    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    n_test = n // 5
    return perm[n_test:].sort().values, perm[:n_test]


def _fit_classifier(shape, Xtr, ytr, Xte, yte, seed, shuffle, epochs, batch, lr):
    from unionml_amd.ops.tabular import TabularMLP

    clf = TabularMLP(*shape, device="cpu", seed=seed)
    clf.fit_standardizer(Xtr)
    clf.train_epochs(clf.stage(Xtr), ytr, epochs=epochs, batch_size=batch, lr=lr,
                     shuffle=shuffle, shuffle_seed=seed)
    return clf.evaluate_raw(Xte, yte)["accuracy"]


def bench_accuracy(seeds):
    import torch

    from unionml_amd.ops.tabular import TabularMLPRegressor

    out = {}

    def both(name, run):
        out[name] = {}
        for shuffle in (False, True):
            vals = [run(seed, shuffle) for seed in range(seeds)]
            out[name]["on" if shuffle else "off"] = {
                "mean": statistics.mean(vals), "min": min(vals), "max": max(vals),
                "runs": vals}

    # digits app: sklearn's digits, as they come and sorted by label
    from sklearn.datasets import load_digits

    d = load_digits()
    X = torch.tensor(d.data, dtype=torch.float32)
    y = torch.tensor(d.target, dtype=torch.int32)
    tr, te = _split(len(X))
    for name, order in (("digits", tr), ("digits_label_sorted",
                                         tr[torch.argsort(y[tr], stable=True)])):
        both(name, lambda seed, sh, order=order: _fit_classifier(
            (64, 32, 10), X[order], y[order], X[te], y[te], seed, sh, 30, 512, 2e-3))

    # MNIST app's geometry on synthetic clusters (no dataset download)
    Xm, ym = synthetic(6000, (784, 128, 10), "cpu")
    Xm = Xm + 10.0 * torch.randn(Xm.shape, generator=torch.Generator().manual_seed(1))
    trm, tem = _split(len(Xm))
    both("mnist_shape_synthetic", lambda seed, sh: _fit_classifier(
        (784, 128, 10), Xm[trm], ym[trm], Xm[tem], ym[tem], seed, sh, 5, 512, 3e-3))

    # regression app: y = tanh(X w) + noise, 20 features, one target
    gen = torch.Generator().manual_seed(2)
    Xr = torch.randn(2000, 20, generator=gen)
    Yr = torch.tanh(Xr @ torch.randn(20, 1, generator=gen)) \
        + 0.1 * torch.randn(2000, 1, generator=gen)
    trr, ter = _split(len(Xr))

    def fit_reg(seed, shuffle):
        reg = TabularMLPRegressor(20, 32, 1, device="cpu", seed=seed)
        reg.fit_standardizer(Xr[trr])
        reg.fit_target_standardizer(Yr[trr])
        reg.train_epochs(reg.stage(Xr[trr]), reg.stage_targets(Yr[trr]), epochs=60,
                         batch_size=128, lr=5e-3, shuffle=shuffle, shuffle_seed=seed)
        return reg.evaluate_raw(Xr[ter], Yr[ter])["r2_mean"]

    both("regression_r2", fit_reg)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--mode", choices=("kernel", "epoch", "accuracy"), default="kernel")
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--seeds", type=int, default=5)
    p.add_argument("--variants", choices=("off", "on", "both"), default="both",
                   help="epoch mode: which captured epochs to time")
    p.add_argument("--tree", default=None, help="import unionml_amd from this checkout")
    p.add_argument("--out", default=None, help="also write the JSON line here")
    args = p.parse_args()
    sys.path.insert(0, args.tree or str(Path(__file__).resolve().parent.parent))

    import torch

    result = {"mode": args.mode, "tree": args.tree or "."}
    if args.mode == "accuracy":
        result.update(bench_accuracy(args.seeds))
    else:
        assert torch.cuda.is_available(), "needs a GPU"
        result["device"] = torch.cuda.get_device_name(0)
        for name, (n, shape, batch) in SHAPES.items():
            if args.mode == "kernel":
                result[name] = bench_kernel(n, shape, args.windows)
            else:
                import inspect

                from unionml_amd.ops.tabular import TabularMLP

                has = "shuffle" in inspect.signature(TabularMLP.train_epochs).parameters
                variants = ("off", "on") if args.variants == "both" else (args.variants,)
                if not has:
                    variants = ("off",)
                result[name] = bench_epoch(n, shape, batch, args.windows, variants)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
