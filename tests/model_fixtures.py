"""Full sklearn + pytorch app fixtures assembled from fixture functions
(fixture design modeled on the reference's tests/unit/model_fixtures.py:
a synthetic 100-row frame + a complete app built by decorators)."""

from typing import List, NamedTuple, Tuple

import pandas as pd
import pytest
from sklearn.linear_model import LogisticRegression

from unionml_amd import Dataset, Model


def make_dataset(**kwargs) -> Dataset:
    ds = Dataset(
        name="ds",
        targets=["y"],
        test_size=0.2,
        shuffle=True,
        random_state=42,
        **kwargs,
    )

    @ds.reader
    def reader(n: int = 100) -> pd.DataFrame:
        from dataset_fixtures import make_frame

        return make_frame(n)

    return ds


def build_sklearn_app(custom_init: bool = False) -> Model:
    dataset = make_dataset()
    model = Model(
        name="sk_model",
        init=None if custom_init else LogisticRegression,
        dataset=dataset,
    )

    if custom_init:

        @model.init
        def init(hyperparameters: dict) -> LogisticRegression:
            return LogisticRegression(**hyperparameters)

    @model.trainer
    def trainer(
        estimator: LogisticRegression, features: pd.DataFrame, target: pd.DataFrame
    ) -> LogisticRegression:
        return estimator.fit(features, target.squeeze())

    @model.predictor
    def predictor(estimator: LogisticRegression, features: pd.DataFrame) -> List[float]:
        return [float(x) for x in estimator.predict(features)]

    @model.evaluator
    def evaluator(
        estimator: LogisticRegression, features: pd.DataFrame, target: pd.DataFrame
    ) -> float:
        from sklearn.metrics import accuracy_score

        return float(accuracy_score(target.squeeze(), estimator.predict(features)))

    return model


@pytest.fixture(params=[False, True], ids=["default_init", "custom_init"])
def sklearn_model(request) -> Model:
    return build_sklearn_app(custom_init=request.param)


def build_pytorch_app() -> Model:
    import torch

    class TinyNet(torch.nn.Module):
        def __init__(self, in_dim: int = 3, hidden: int = 8, out_dim: int = 2):
            super().__init__()
            self.net = torch.nn.Sequential(
                torch.nn.Linear(in_dim, hidden),
                torch.nn.ReLU(),
                torch.nn.Linear(hidden, out_dim),
            )

        def forward(self, x):
            return self.net(x)

    dataset = make_dataset()
    model = Model(name="pt_model", init=TinyNet, dataset=dataset)

    @model.trainer
    def trainer(
        module: TinyNet,
        features: pd.DataFrame,
        target: pd.DataFrame,
        *,
        epochs: int = 3,
        lr: float = 0.01,
    ) -> TinyNet:
        opt = torch.optim.Adam(module.parameters(), lr=lr)
        x = torch.tensor(features.to_numpy(), dtype=torch.float32)
        y = torch.tensor(target.squeeze().to_numpy(), dtype=torch.long)
        for _ in range(epochs):
            opt.zero_grad()
            loss = torch.nn.functional.cross_entropy(module(x), y)
            loss.backward()
            opt.step()
        return module

    @model.predictor
    def predictor(module: TinyNet, features: pd.DataFrame) -> List[int]:
        import torch

        x = torch.tensor(features.to_numpy(), dtype=torch.float32)
        with torch.no_grad():
            return [int(i) for i in module(x).argmax(dim=1)]

    @model.evaluator
    def evaluator(module: TinyNet, features: pd.DataFrame, target: pd.DataFrame) -> float:
        preds = predictor(module, features)
        return float((pd.Series(preds).to_numpy() == target.squeeze().to_numpy()).mean())

    return model


@pytest.fixture
def pytorch_model() -> Model:
    return build_pytorch_app()


@pytest.fixture
def gloo_cpu_only(monkeypatch):
    """Pin a multi-process gloo/CPU test to the CPU on machines that have
    GPUs too: spawned ranks inherit an empty device list, and this process
    reports none, so ``dp`` is not capped by the number of visible GPUs."""
    import torch

    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 0)
