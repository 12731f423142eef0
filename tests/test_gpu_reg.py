"""GPU tests for TabularMLPRegressor above the kernels: the engine
equivalences of tests/test_gpu_gen.py on the regression head, hipGraph
serving, and the packaged app against the CPU reference path."""

import numpy as np
import pytest
import torch

import oracle64_reg as o64r

pytestmark = pytest.mark.gpu

SHAPES = [(100, 50, 1), (64, 32, 26)]   # single target; two-tile head at 64x32
B, STEPS = 256, 3


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def make_reg(shape, dev, seed):
    from unionml_amd.ops.tabular import TabularMLPRegressor

    inf, hid, T = shape
    return TabularMLPRegressor(in_features=inf, hidden=hid, targets=T, device=dev, seed=seed)


def synth(shape, n, seed):
    return o64r.synth_reg(shape[0], shape[2], n, seed)


def fitted(shape, dev, seed, X, Y):
    reg = make_reg(shape, dev, seed)
    reg.fit_standardizer(X)
    reg.fit_target_standardizer(Y)
    return reg, reg.stage(X), reg.stage_targets(Y)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reduce_mode_matches_fused(ext, dev, shape):
    """grads_out mode (the DP pre-collective step) + adam_step_gen lands
    where the fused reduce+Adam lands; the incrementally maintained wimg
    equals a rebuild."""
    X, Y = synth(shape, B, seed=3)
    a, Xbf_a, Yt_a = fitted(shape, dev, 4, X, Y)
    b, Xbf_b, Yt_b = fitted(shape, dev, 4, X, Y)
    assert not a.use_spec and Yt_a.shape == (B, a.g.cpad)
    g = a.g
    rpw = a._rows_per_wg()
    for reg in (a, b):
        reg._ensure_slabs((B + rpw - 1) // rpw)
    loss_a = a.grads[g.nparam : g.nparam + 1]
    for _ in range(STEPS):
        a._fused_adam_step(Xbf_a, Yt_a, 1.0 / B, 1e-3, loss_a)
        b._step_reduce(Xbf_b, Yt_b, 1.0 / B, 1e-3)
        b._adam(1e-3)
    torch.cuda.synchronize()
    assert int(a.t_dev.item()) == STEPS and int(b.t_dev.item()) == STEPS
    # the step's sums are order-fixed and both paths share adam_update: same bits
    assert torch.equal(a.master, b.master), (a.master - b.master).abs().max().item()
    assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    for reg in (a, b):
        incremental = reg.wimg.clone()
        reg._build_wimg()
        torch.cuda.synchronize()
        assert torch.equal(incremental, reg.wimg)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_graph_vs_eager_and_state_roundtrip(ext, dev, shape):
    """3 steps (one batch of 256, three epochs: one eager, one captured,
    one replayed) through hipGraph equal the eager steps; a state_dict
    round trip predicts bit for bit."""
    X, Y = synth(shape, B, seed=21)
    results = {}
    for use_graph in (False, True):
        reg, Xbf, Yt = fitted(shape, dev, 1, X, Y)
        loss = reg.train_epochs(Xbf, Yt, epochs=STEPS, batch_size=B, lr=2e-3,
                                use_graph=use_graph)
        assert int(reg.t_dev.item()) == STEPS and loss == loss
        results[use_graph] = (loss, reg.master.cpu(), reg)
    # a replayed graph runs the launches the eager epochs run: same bits
    assert results[True][0] == results[False][0]
    assert torch.equal(results[True][1], results[False][1])

    reg = results[True][2]
    rebuilt = make_reg(shape, dev, seed=99)
    rebuilt.load_state_dict(reg.state_dict())
    p1, p2 = reg.predict(X[:200]), rebuilt.predict(X[:200])
    assert p1.shape == (200, shape[2]) and p1.dtype == torch.float32
    assert torch.equal(p1.cpu(), p2.cpu())

    from unionml_amd.ops.tabular import TabularMLP

    clf = TabularMLP(shape[0], shape[1], max(shape[2], 2), device=dev)
    with pytest.raises(ValueError, match="head"):
        clf.load_state_dict(reg.state_dict())


def test_graph_runner_serves_a_regressor(ext, dev):
    """Bucketed hipGraph replay returns [n][T] float32, bit for bit
    predict()'s rows, for n below, at and across a chunk."""
    from unionml_amd.serving.graph_runner import TabularGraphRunner

    shape = (64, 32, 26)
    X, Y = synth(shape, 512, seed=8)
    reg, Xbf, Yt = fitted(shape, dev, 2, X, Y)
    reg.train_epochs(Xbf, Yt, epochs=2, batch_size=256, lr=2e-3)
    runner = TabularGraphRunner(reg, max_batch_size=64)
    for n in (1, 3, 70):
        out = runner(X[:n].numpy())
        assert out.shape == (n, 26) and out.dtype == np.float32
        direct = reg.predict(X[:n]).cpu().numpy()
        assert np.array_equal(out, direct), f"n={n}"


def test_app_gpu_matches_cpu_reference_path(ext, dev):
    """The diabetes app through Model.train on the GPU: held-out R^2 beats
    the mean predictor, and does not fall below the CPU reference path's
    (same seed, data, epochs) by more than oracle64_reg.APP_R2_MARGIN =
    0.228: three times the CPU path's R^2 spread over five init seeds
    (0.0760), measured on the CPU by tests/test_tabular_reg_cpu.py."""
    from unionml_amd.models.mlp_regress import model

    seed = o64r.APP_SEEDS[0]
    _, cpu_metrics = o64r.train_app("cpu", seed)
    reg, gpu_metrics = o64r.train_app("cuda", seed)
    assert reg.use_hip and not reg.use_spec
    print(f"app held-out R2: gpu={gpu_metrics['test']:.4f} cpu={cpu_metrics['test']:.4f} "
          f"margin={o64r.APP_R2_MARGIN:.4f}")
    assert gpu_metrics["test"] > 0.0, gpu_metrics
    assert gpu_metrics["test"] >= cpu_metrics["test"] - o64r.APP_R2_MARGIN, (
        gpu_metrics, cpu_metrics)
    # batched hipGraph serving answers in the predictor's shape and values
    want = [model.predict(features=r) for r in o64r.APP_REQUESTS]
    assert all(isinstance(v, float) for w in want for v in w)
    assert o64r.batched_predict(model, o64r.APP_REQUESTS) == want
