"""What the shuffled-epoch tests share, CPU and GPU: the three models, the
seeded staged data, and the manual loop that defines a shuffled run."""

import torch

from unionml_amd.ops import reference as ref
from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor

STATE = ("master", "m", "v", "t_dev")
# (regression, constructor shape): the specialized digits shape, a
# generalized shape, and the regression head with one target
MODELS = [(False, (64, 32, 10)), (False, (100, 50, 7)), (True, (20, 32, 1))]
MODEL_IDS = ["64x32x10", "100x50x7", "reg-20x32-T1"]
N, BATCH = 300, 128      # batches of 128, 128 and a 44-row tail


def make_model(regression, shape, device="cpu"):
    cls = TabularMLPRegressor if regression else TabularMLP
    return cls(*shape, device=device, seed=3)


def make_data(model, n=N, seed=0):
    """staged features and targets of n seeded rows, on the model's device"""
    g = model.g
    gen = torch.Generator().manual_seed(seed)
    X = torch.randn(n, g.in_features, generator=gen)
    model.fit_standardizer(X)
    Xbf = model.stage(X)
    if g.head == ref.HEAD_REGRESSION:
        Y = torch.randn(n, g.classes, generator=gen)
        model.fit_target_standardizer(Y)
        return Xbf, model.stage_targets(Y)
    y = torch.randint(0, g.classes, (n,), generator=gen, dtype=torch.int32)
    return Xbf, y.to(model.device)


def manual_epochs(model, Xbf, y, epochs, seed, after_epoch=None, **kw):
    """The definition of a shuffled run: per epoch, the reference
    permutation at the current step counter, a host gather, one plain epoch."""
    for _ in range(epochs):
        perm = ref.shuffle_perm(Xbf.shape[0], seed, int(model.t_dev.item()))
        perm = perm.to(Xbf.device)
        model.train_epochs(Xbf[perm].contiguous(), y[perm].contiguous(), epochs=1,
                           shuffle=False, **kw)
        if after_epoch is not None:
            after_epoch()


def assert_same_state(a, b, names=STATE):
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
