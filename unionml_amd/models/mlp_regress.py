"""Regression app: a one-hidden-layer MLP regressor on the CDNA4 tabular
hot path.

The counterpart of :mod:`unionml_amd.models.mlp` for a continuous target:
the same ``@dataset``/``@model`` decorator API, with the trainer and the
predictor running on :class:`unionml_amd.ops.tabular.TabularMLPRegressor`:
the generalized gfx950 MFMA kernels with the squared-error head on GPU,
the torch reference on CPU. The reader serves sklearn's bundled diabetes
set (10 features, 442 rows, one target; no network needed) or, with
``synthetic=True``, a seeded smooth function of 10 random features.
"""

from typing import List

import numpy as np
import pandas as pd
import torch

from unionml_amd import Dataset, Model
from unionml_amd.ops.tabular import TabularMLPRegressor, split_validation
from unionml_amd.parallel import get_world_size
from unionml_amd.serving.graph_runner import TabularGraphRunner, graphed
from unionml_amd.utils.staging import get_stager

N_FEATURES = 10
FEATURES = [f"x{i}" for i in range(N_FEATURES)]

dataset = Dataset(name="diabetes", features=FEATURES, targets=["target"], test_size=0.2)


@dataset.reader
def reader(n: int = 0, synthetic: bool = False, seed: int = 17) -> pd.DataFrame:
    """sklearn's bundled diabetes set by default; ``synthetic=True`` draws
    n rows of a noisy smooth function of 10 features (target mean ~150,
    spread ~50, like the real one)."""
    if synthetic:
        rng = np.random.RandomState(seed)
        X = rng.randn(n or 442, N_FEATURES).astype(np.float32) * 0.05
        w = rng.randn(N_FEATURES)
        s = (X / 0.05) @ w
        y = 150.0 + 50.0 * np.tanh(0.5 * s) + 5.0 * rng.randn(len(X))
    else:
        from sklearn.datasets import load_diabetes

        data = load_diabetes()
        X, y = data.data, data.target
        if n:
            X, y = X[:n], y[:n]
    frame = pd.DataFrame(np.asarray(X, dtype=np.float32), columns=FEATURES)
    frame["target"] = np.asarray(y, dtype=np.float32)
    return frame


model = Model(
    name="diabetes_mlp",
    init=lambda hyperparameters=None: TabularMLPRegressor(
        **{"in_features": N_FEATURES, "hidden": 32, "targets": 1, **(hyperparameters or {})}
    ),
    dataset=dataset,
)


@model.trainer
def trainer(
    reg: TabularMLPRegressor,
    features: pd.DataFrame,
    target: pd.DataFrame,
    *,
    epochs: int = 60,
    batch_size: int = 128,
    lr: float = 5e-3,
    use_graph: bool = True,
    validation_fraction: float = 0.0,
    patience: int = 0,
    restore_best: bool = False,
    shuffle: bool = False,
    shuffle_seed: int = 0,
) -> TabularMLPRegressor:
    """Stage features and targets into HBM, fit BOTH standardizers (the
    network learns standardized targets), then run the fused-kernel
    minibatch loop. Under DP each rank gets a row shard and gradients
    all-reduce on RCCL inside the step."""
    stager = get_stager(reg.device)
    X = stager.to_device(features.to_numpy().astype(np.float32))
    Y = stager.to_device(target.to_numpy().astype(np.float32).reshape(len(target), -1))
    validation = None
    if validation_fraction > 0:
        # hold out a seeded share of the rows; both standardizers see the
        # training rows only
        tr, va = split_validation(len(X), validation_fraction)
        Xv, Yv = X[va.to(X.device)], Y[va.to(Y.device)]
        X, Y = X[tr.to(X.device)], Y[tr.to(Y.device)]
    reg.fit_standardizer(X)
    reg.fit_target_standardizer(Y)
    if validation_fraction > 0:
        validation = (reg.stage(Xv), reg.stage_targets(Yv))
    reg.train_epochs(
        reg.stage(X),
        reg.stage_targets(Y),
        epochs=epochs,
        batch_size=batch_size,
        lr=lr,
        use_graph=use_graph,
        world_size=get_world_size(),
        validation=validation,
        patience=patience or None,
        restore_best=restore_best,
        shuffle=shuffle,
        shuffle_seed=shuffle_seed,
    )
    return reg


def _graphed_runner(reg: TabularMLPRegressor, max_batch: int):
    """The batched serving forward. TabularGraphRunner returns a
    regressor's ``[n][targets]`` matrix; this app has one target and its
    predictor answers one float per row, so the batcher must see ``[n]``
    too, or /predict would change shape with batching on."""
    runner = TabularGraphRunner(reg, max_batch)
    return lambda features: runner(features)[:, 0]


@model.predictor
@graphed(_graphed_runner)
def predictor(reg: TabularMLPRegressor, features: pd.DataFrame) -> List[float]:
    X = torch.from_numpy(np.ascontiguousarray(features.to_numpy(), dtype=np.float32))
    preds = reg.predict(X)
    return [float(v) for v in preds[:, 0].cpu()]


@model.evaluator
def evaluator(reg: TabularMLPRegressor, features: pd.DataFrame, target: pd.DataFrame) -> float:
    """Coefficient of determination R^2 (1 is exact, 0 the mean predictor)."""
    X = np.ascontiguousarray(features.to_numpy(), dtype=np.float32)
    Y = target.to_numpy().astype(np.float32).reshape(len(target), -1)
    # the squared error is summed on the device by the fused evaluation
    # kernel; this app has one target
    return float(reg.evaluate_raw(torch.from_numpy(X), torch.from_numpy(Y))["r2"][0])


@model.saver
def saver(reg: TabularMLPRegressor, hyperparameters, file, **kwargs):
    torch.save({"state": reg.state_dict(), "hyperparameters": hyperparameters}, file)
    return file


@model.loader
def loader(file, **kwargs) -> TabularMLPRegressor:
    payload = torch.load(file, map_location="cpu", weights_only=False)
    inf, hid, targets = (int(x) for x in payload["state"]["geometry"])
    reg = TabularMLPRegressor(in_features=inf, hidden=hid, targets=targets)
    reg.load_state_dict(payload["state"])
    return reg
