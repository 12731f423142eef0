"""Plain fp64 oracle for the REGRESSION head of the generalized tabular
kernels, plus the case matrix its tests share (tests/test_oracle64_reg_cpu.py
validates the oracle and the cases on the CPU, tests/test_gpu_reg_oracle.py
runs the HIP kernels against it). The classifier's counterpart is
tests/oracle64.py, whose layout helpers and error measures are reused here.

Nothing here rounds: the functions take the kernel's actual inputs (the bf16
operands upcast, the fp32 biases and targets) and compute in float64. The
one exception is the predict oracle's standardized input, rounded to bf16
once, because that rounding is part of the predict kernel's contract.

No tests live in this module.
"""

from types import SimpleNamespace

import torch

import oracle64 as o64
from oracle64 import F64, real_segments
from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import HEAD_REGRESSION, Geometry

# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


def step64_reg(g: Geometry, Xbf, Yt, W1bf, W2bf, master, invB: float):
    """fp64 forward/backward of loss = 0.5 * invB * sum_{b, c<T} (z - y)^2.

    Returns (grads, Hpre, H, z): flat grads in the Geometry layout with the
    loss at [g.nparam]; only the real targets enter, the ReLU mask comes
    from Hpre > 0, pad entries are exactly 0."""
    W1, b1, W2, b2 = o64._real_operands(g, W1bf, W2bf, master)
    X = Xbf.to(F64)[:, : g.in_features]
    Y = Yt.to(F64)[:, : g.classes]

    Hpre, H, z = o64.forward64(X, W1, b1, W2, b2)
    d = z - Y
    loss = 0.5 * invB * (d * d).sum()
    dz = d * invB
    dH = (dz @ W2.T) * (Hpre > 0)

    grads = torch.zeros(g.nparam + 1, dtype=F64)
    seg = real_segments(g, grads)
    seg["W1"].copy_(X.T @ dH)
    seg["b1"].copy_(dH.sum(dim=0))
    seg["W2"].copy_(H.T @ dz)
    seg["b2"].copy_(dz.sum(dim=0))
    grads[g.nparam] = loss
    return grads, Hpre, H, z


def predict64_reg(g: Geometry, X, mean, invstd, W1bf, W2bf, master, y_mean, y_scale):
    """(out, H, z) in fp64: out = z * y_scale + y_mean over the real
    targets; only the standardized input is rounded (to bf16, once)."""
    W1, b1, W2, b2 = o64._real_operands(g, W1bf, W2bf, master)
    Xs = o64.standardized_input(X, mean, invstd).to(F64)
    _, H, z = o64.forward64(Xs, W1, b1, W2, b2)
    return z * y_scale.to(F64) + y_mean.to(F64), H, z


def loss_bound_reg(H, z, Yt, W2bf, g: Geometry, invB: float, loss64: float) -> float:
    """|loss_kernel - loss_64| bound. Rounding H to bf16 moves every z of
    row b by at most delta_b (oracle64.logit_slack); through the quadratic,
    0.5 (d + e)^2 - 0.5 d^2 = d e + 0.5 e^2 with |e| <= delta_b, summed over
    the T targets. The last term covers the fp32 accumulation."""
    T = g.classes
    delta = o64.logit_slack(H, W2bf, g)
    absd = (z - Yt.to(F64)[:, :T]).abs().sum(dim=1)
    quad = invB * (delta * absd + 0.5 * T * delta * delta).sum()
    return float(quad + 1e-5 * max(1.0, abs(loss64)))


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------


def make_case_reg(shape, B: int, seed: int):
    """Inputs for one (geometry, batch, seed) regression case, on the CPU.

    Weights as TabularMLPRegressor initialises them, NON-ZERO biases
    N(0, 0.3) on the real entries (pads stay 0), X scaled per column as in
    oracle64.make_case. Standardized targets Yt: N(0, 1) per column times a
    column scale spread over 0.5..2, zero-padded to [B][cpad]. For the
    predict cases, a target scaler FITTED on N_FIT rows whose columns have
    means up to 1e2 and scales 1e-2..1e2."""
    from unionml_amd.ops.tabular import TabularMLPRegressor

    inf, hid, T = shape
    reg = TabularMLPRegressor(in_features=inf, hidden=hid, targets=T, device="cpu", seed=seed)
    g = reg.g
    gen = torch.Generator().manual_seed(2000 + seed)
    master = reg.master.clone()
    seg = real_segments(g, master)
    seg["b1"].copy_(torch.randn(hid, generator=gen) * 0.3)
    seg["b2"].copy_(torch.randn(T, generator=gen) * 0.3)
    bfmirror = master.bfloat16()

    scale = torch.linspace(0.5, 2.0, inf)
    X = torch.randn(B, inf, generator=gen) * scale + 0.3
    Xfit = torch.randn(o64.N_FIT, inf, generator=gen) * scale + 0.3
    yscale = torch.linspace(0.5, 2.0, T)
    Yt = torch.zeros(B, g.cpad)
    Yt[:, :T] = torch.randn(B, T, generator=gen) * yscale

    # raw targets the predict cases fit their scaler on
    col_mean = torch.linspace(-100.0, 100.0, T)
    col_std = torch.logspace(-2.0, 2.0, T)
    Yfit = torch.randn(o64.N_FIT, T, generator=gen) * col_std + col_mean
    y_mean, y_invstd = ref.standardize_fit(Yfit)
    y_scale = 1.0 / y_invstd

    Xbf = torch.zeros(B, g.inp, dtype=torch.bfloat16)
    Xbf[:, :inf] = X.bfloat16()
    W1bf = bfmirror[g.off_w1 : g.off_w1 + g.inp * g.hid].view(g.inp, g.hid)
    W2bf = bfmirror[g.off_w2 : g.off_w2 + g.hid * g.cpad].view(g.hid, g.cpad)
    return SimpleNamespace(
        shape=shape, B=B, seed=seed, g=g, master=master, bfmirror=bfmirror,
        W1bf=W1bf, W2bf=W2bf, X=X, Xfit=Xfit, Xbf=Xbf, Yt=Yt, invB=1.0 / B,
        y_mean=y_mean, y_invstd=y_invstd, y_scale=y_scale,
    )


def reference_step_reg(case) -> torch.Tensor:
    """Flat grads (+loss) of the bf16-mirroring reference for a case"""
    out = torch.zeros(case.g.nparam + 1)
    ref.mlp_step_reg_g(case.g, case.Xbf, case.Yt, case.W1bf, case.W2bf, case.master,
                       out, case.invB)
    return out


# ---------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------


def _as_targets(shape):
    # the single-target case is the common one: 20x32x2 runs as 20x32x1
    return (20, 32, 1) if tuple(shape) == (20, 32, 2) else tuple(shape)


# oracle64's geometries with the class count read as T: every row of the
# instantiation table (tabular_launch.h) once, for the regression head; T
# covers 1, 16, 17 and 32
STEP_INSTANTIATIONS = [(inst, _as_targets(s)) for inst, s in o64.STEP_INSTANTIATIONS]
PRED_INSTANTIATIONS = [(inst, _as_targets(s)) for inst, s in o64.PRED_INSTANTIATIONS]

DEFAULT_SEED = 5
# (shape, B) -> seed where the default seed gives a degenerate case (a real
# segment of the ORACLE gradient with zero norm); found on the CPU by
# tests/test_oracle64_reg_cpu.py from the oracle alone, never from a kernel
SEED_OVERRIDES = {}


def case_seed(shape, B):
    return SEED_OVERRIDES.get((tuple(shape), B), DEFAULT_SEED)


def step_cases():
    """[(id, (HID, RT, CPAD), shape, B, seed)] for the regression step"""
    out = []
    for inst, shape in STEP_INSTANTIATIONS:
        for B in o64.step_batches(inst[1]):
            out.append((f"{o64.inst_id(inst)}-{o64.shape_id(shape)}-B{B}", inst, shape, B,
                        case_seed(shape, B)))
    return out


def predict_cases():
    out = []
    for inst, shape in PRED_INSTANTIATIONS:
        for B in (1, inst[1] + 1):
            out.append((f"{o64.inst_id(inst)}-{o64.shape_id(shape)}-B{B}", inst, shape, B,
                        case_seed(shape, B)))
    return out


def check_instantiation(inst, shape):
    """The geometry really selects the instantiation it is listed under."""
    g = Geometry(*shape, head=HEAD_REGRESSION)
    assert (g.hid, g.cpad) == (inst[0], inst[2]), (inst, shape)


# ---------------------------------------------------------------------------
# a learnable problem for the class-level tests
# ---------------------------------------------------------------------------


def synth_reg(inf: int, T: int, n: int, seed: int):
    """(X, Y): a smooth multi-target function of the features, the target
    columns on very different scales (0.1..100) and offsets (-50..50)"""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, inf, generator=g) * torch.linspace(0.5, 2.0, inf) + 0.3
    W = torch.randn(inf, T, generator=g) / inf ** 0.5
    Y = torch.tanh(X @ W) * torch.logspace(-1.0, 2.0, T) + torch.linspace(-50.0, 50.0, T)
    return X, Y


# ---------------------------------------------------------------------------
# the packaged app (unionml_amd/models/mlp_regress.py)
# ---------------------------------------------------------------------------

APP_SEEDS = (0, 1, 2, 3, 4)
# How far the GPU path's held-out R^2 may fall below the CPU reference
# path's for the same seed, data and epochs: three times the spread
# (max - min) of the CPU path's held-out R^2 over the five init seeds above,
# app defaults otherwise. Measured on the CPU, not chosen:
# R^2 = 0.4498 0.4994 0.4912 0.5258 0.5082, spread 0.0760
# (tests/test_tabular_reg_cpu.py re-measures it).
APP_R2_SPREAD = 0.0760
APP_R2_MARGIN = 3 * APP_R2_SPREAD


def train_app(device: str, seed: int):
    """Model.train of the diabetes app on ``device``: (regressor, metrics)"""
    from unionml_amd.models.mlp_regress import model

    model.artifact = None
    return model.train(hyperparameters={"seed": seed, "device": device})


APP_REQUESTS = [
    [{f"x{i}": 0.01 * i for i in range(10)}],
    [{f"x{i}": -0.02 for i in range(10)}, {f"x{i}": 0.03 - 0.01 * i for i in range(10)}],
    [{f"x{i}": 0.05 * (-1) ** i for i in range(10)}],
]


def batched_predict(model, requests):
    """Each request through the serving DynamicBatcher (the @graphed
    forward), all submitted at once so they share a batch: one JSON-ready
    answer per request"""
    import asyncio

    from unionml_amd.serving.batcher import DynamicBatcher

    batcher = DynamicBatcher(model, max_batch_size=64, max_delay_ms=30.0)
    batcher.start()
    try:
        async def fire():
            return await asyncio.gather(*(batcher.submit(r) for r in requests))

        return asyncio.run(fire())
    finally:
        batcher.stop()
