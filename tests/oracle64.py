"""Plain fp64 oracle for the tabular kernels, plus the case matrix the
kernel-vs-oracle tests share (tests/test_oracle64_cpu.py validates the
oracle and the cases on the CPU, tests/test_gpu_oracle.py runs the HIP
kernels against it).

Unlike unionml_amd/ops/reference.py, which mirrors the kernels' bf16 round
trips on purpose, nothing here rounds: every function takes the kernel's
actual inputs (the bf16 operands upcast, the fp32 biases from ``master``)
and computes in ``torch.float64`` on the CPU. The one exception is
``predict64``, where the standardized input is rounded to bf16 once,
because that rounding is part of the predict kernel's contract.

No tests live in this module.
"""

from types import SimpleNamespace

import torch

from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import Geometry

F64 = torch.float64
SEGMENTS = ("W1", "b1", "W2", "b2")

BF16_ULP = 2.0 ** -8      # spacing of bf16 relative to the value
BF16_HALF_ULP = 2.0 ** -9  # its unit roundoff

# ---------------------------------------------------------------------------
# flat-layout helpers
# ---------------------------------------------------------------------------


def real_segments(g: Geometry, flat: torch.Tensor):
    """The real (unpadded) blocks of a flat master/grads vector."""
    W1, b1, W2, b2 = ref.unpack_master_g(g, flat[: g.nparam])
    return {
        "W1": W1[: g.in_features, : g.hidden],
        "b1": b1[: g.hidden],
        "W2": W2[: g.hidden, : g.classes],
        "b2": b2[: g.classes],
    }


def pad_mask(g: Geometry) -> torch.Tensor:
    """bool [nparam]: True on every padded parameter."""
    real = torch.zeros(g.nparam, dtype=torch.bool)
    for blk in real_segments(g, real).values():
        blk.fill_(True)
    return ~real


def e(a: torch.Tensor, o: torch.Tensor) -> float:
    """relative L2 error of ``a`` against the oracle ``o``"""
    a, o = a.to(F64), o.to(F64)
    return float((a - o).norm() / o.norm())


def emax(a: torch.Tensor, o: torch.Tensor) -> float:
    """max-abs error relative to the oracle's largest entry"""
    a, o = a.to(F64), o.to(F64)
    return float((a - o).abs().max() / o.abs().max())


def segment_errors(g: Geometry, a: torch.Tensor, o: torch.Tensor):
    """{segment: (e, emax)} of flat grads ``a`` against the oracle's"""
    sa, so = real_segments(g, a), real_segments(g, o)
    return {s: (e(sa[s], so[s]), emax(sa[s], so[s])) for s in SEGMENTS}


# ---------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------


def _real_operands(g, W1bf, W2bf, master):
    b = real_segments(g, master.to(F64))
    W1 = W1bf.to(F64)[: g.in_features, : g.hidden]
    W2 = W2bf.to(F64)[: g.hidden, : g.classes]
    return W1, b["b1"], W2, b["b2"]


def forward64(X, W1, b1, W2, b2):
    Hpre = X @ W1 + b1
    H = torch.relu(Hpre)
    return Hpre, H, H @ W2 + b2


def step64(g: Geometry, Xbf, y, W1bf, W2bf, master, invB: float):
    """fp64 forward/backward of the mean-style cross-entropy step.

    Returns (grads, Hpre, H, logits): flat grads in the Geometry layout
    with the loss at [g.nparam]; softmax over the real classes only, the
    ReLU mask from Hpre > 0, pad entries exactly 0."""
    W1, b1, W2, b2 = _real_operands(g, W1bf, W2bf, master)
    X = Xbf.to(F64)[:, : g.in_features]
    B = X.shape[0]
    rows = torch.arange(B)
    yl = y.long()

    Hpre, H, logits = forward64(X, W1, b1, W2, b2)
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    loss = -logp[rows, yl].sum() * invB
    dlogits = torch.exp(logp)
    dlogits[rows, yl] -= 1.0
    dlogits *= invB
    dH = (dlogits @ W2.T) * (Hpre > 0)

    grads = torch.zeros(g.nparam + 1, dtype=F64)
    seg = real_segments(g, grads)
    seg["W1"].copy_(X.T @ dH)
    seg["b1"].copy_(dH.sum(dim=0))
    seg["W2"].copy_(H.T @ dlogits)
    seg["b2"].copy_(dlogits.sum(dim=0))
    grads[g.nparam] = loss
    return grads, Hpre, H, logits


def standardized_input(X, mean, invstd) -> torch.Tensor:
    """What the predict kernel feeds its first MFMA: the fp32
    standardization rounded to bf16 once (the kernel's contract)."""
    return ((X.float() - mean.float()) * invstd.float()).bfloat16()


def predict64(g: Geometry, X, mean, invstd, W1bf, W2bf, master):
    """(logits, probs, H) in fp64 over the real classes; only the
    standardized input is rounded (to bf16, once)."""
    W1, b1, W2, b2 = _real_operands(g, W1bf, W2bf, master)
    Xs = standardized_input(X, mean, invstd).to(F64)
    _, H, logits = forward64(Xs, W1, b1, W2, b2)
    return logits, torch.softmax(logits, dim=1), H


def logit_slack(H: torch.Tensor, W2bf, g: Geometry) -> torch.Tensor:
    """Per row, how far rounding H to bf16 can move any logit:
    2^-9 * max_c sum_h |H_bh| |W2_hc|."""
    W2 = W2bf.to(F64)[: g.hidden, : g.classes].abs()
    return BF16_HALF_ULP * (H.abs() @ W2).max(dim=1).values


def loss_bound(H, W2bf, g: Geometry, invB: float) -> float:
    """|loss_kernel - loss_64| bound: softmax cross-entropy is 2-Lipschitz
    in the inf-norm of the logits, which move by at most the bf16 rounding
    of H; 1e-5 covers the fp32 accumulation."""
    return float(invB * (2.0 * logit_slack(H, W2bf, g)).sum() + 1e-5)


def clear_rows(logits: torch.Tensor, H, W2bf, g: Geometry) -> torch.Tensor:
    """bool [B]: rows whose top-2 logit margin exceeds twice the logit
    slack, i.e. whose argmax no admissible rounding of H can change."""
    top = logits.topk(2, dim=1).values
    return (top[:, 0] - top[:, 1]) > 2.0 * logit_slack(H, W2bf, g)


MAX_EXCLUDED = 0.10   # share of rows the margin rule may exclude per case


def adam64(master, grads_per_step, lr, b1, b2, eps):
    """fp64 Adam from zero moments: lists of master, m and v after each
    step (textbook form, bias-corrected moments)."""
    p = master.to(F64).clone()
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    out_p, out_m, out_v = [], [], []
    for t, gr in enumerate(grads_per_step, start=1):
        gr = gr.to(F64)[: p.numel()]
        m = b1 * m + (1.0 - b1) * gr
        v = b2 * v + (1.0 - b2) * gr * gr
        mhat = m / (1.0 - b1 ** t)
        vhat = v / (1.0 - b2 ** t)
        p = p - lr * mhat / (torch.sqrt(vhat) + eps)
        out_p.append(p.clone())
        out_m.append(m.clone())
        out_v.append(v.clone())
    return out_p, out_m, out_v


# Share of a tensor's entries adam_moments32 may exempt (a condition of the
# tests that use it, not a measurement).
MAX_MIDPOINT_SHARE = 1e-3

_F32_MIN_NORMAL = 2.0 ** -126


def _fma32(a, b, c):
    """fp32 fma(a, b, c) of fp32 tensors, evaluated in fp64, and the entries
    where that evaluation cannot be trusted to the last bit.

    The product of two fp32 numbers is exact in fp64 (48 bits), so the only
    fp64 rounding is the one of the sum; casting it to fp32 rounds a second
    time. The two roundings differ from the single fp32 rounding of an fma
    only when the fp64 sum sits exactly on the midpoint of two neighbouring
    fp32 numbers: its 29 mantissa bits below fp32 precision are 1 followed
    by 28 zeros. Those entries are flagged, and so is any non-zero sum below
    the smallest normal fp32 number, where the midpoints lie elsewhere."""
    s = a.to(F64) * b.to(F64) + c.to(F64)
    low = s.view(torch.int64) & 0x1FFFFFFF
    exempt = (low == 0x10000000) | ((s != 0) & (s.abs() < _F32_MIN_NORMAL))
    return s.float(), exempt


def adam_moments32(m, v, gr, b1: float, b2: float):
    """One step of the moments as adam_update (tabular_common.h) writes them,
    from fp32 ``m``, ``v`` and gradient ``gr``; ``b1``/``b2`` are the betas
    already rounded to fp32. With rn() one fp32 rounding:

        m' = fma(1-b1, g, rn(b1*m))
        v' = fma(g, rn((1-b2)*g), rn(b2*v))

    Evaluated in fp64, where every fp32 x fp32 product is exact and rn() is
    the cast to fp32 (1-b is exact in fp64 too, so its cast is the fp32
    subtraction). Returns (m', v', exempt_m, exempt_v): the bool masks mark
    the entries whose fma may be double-rounded here (see _fma32)."""
    assert m.dtype == v.dtype == gr.dtype == torch.float32
    t = lambda x: torch.tensor(x, dtype=F64)   # noqa: E731
    rn = lambda x: x.float()                   # noqa: E731
    omb1, omb2 = rn(1.0 - t(b1)), rn(1.0 - t(b2))
    bm = rn(t(b1) * m.to(F64))
    bv = rn(t(b2) * v.to(F64))
    gs = rn(omb2.to(F64) * gr.to(F64))
    m_new, ex_m = _fma32(omb1, gr, bm)
    v_new, ex_v = _fma32(gr, gs, bv)
    return m_new, v_new, ex_m, ex_v


def standardize64(X, eps: float = 1e-5):
    """Two-pass column statistics in fp64: (mean, invstd, var)."""
    Xd = X.to(F64)
    mean = Xd.mean(dim=0)
    var = ((Xd - mean) ** 2).mean(dim=0)
    return mean, 1.0 / torch.sqrt(var + eps), var


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

N_FIT = 500   # rows the predict cases fit their standardizer on


def make_case(shape, B: int, seed: int):
    """Inputs for one (geometry, batch, seed) case, all on the CPU.

    Weights as TabularMLP initialises them, NON-ZERO biases N(0, 0.3) on
    the real entries (pads stay 0), X scaled per column like ``synth`` in
    test_gpu_gen.py. Labels cover every class the batch has room for,
    counted down from classes-1, so the last class is always present and
    is the single label at B = 1."""
    from unionml_amd.ops.tabular import TabularMLP

    inf, hid, cls = shape
    clf = TabularMLP(in_features=inf, hidden=hid, classes=cls, device="cpu", seed=seed)
    g = clf.g
    gen = torch.Generator().manual_seed(1000 + seed)
    master = clf.master.clone()
    seg = real_segments(g, master)
    seg["b1"].copy_(torch.randn(hid, generator=gen) * 0.3)
    seg["b2"].copy_(torch.randn(cls, generator=gen) * 0.3)
    bfmirror = master.bfloat16()

    scale = torch.linspace(0.5, 2.0, inf)
    X = torch.randn(B, inf, generator=gen) * scale + 0.3
    Xfit = torch.randn(N_FIT, inf, generator=gen) * scale + 0.3
    y = torch.randint(0, cls, (B,), generator=gen, dtype=torch.int32)
    n = min(B, cls)
    y[:n] = torch.arange(cls - 1, cls - 1 - n, -1, dtype=torch.int32)

    Xbf = torch.zeros(B, g.inp, dtype=torch.bfloat16)
    Xbf[:, :inf] = X.bfloat16()
    W1bf = bfmirror[g.off_w1 : g.off_w1 + g.inp * g.hid].view(g.inp, g.hid)
    W2bf = bfmirror[g.off_w2 : g.off_w2 + g.hid * g.cpad].view(g.hid, g.cpad)
    return SimpleNamespace(
        shape=shape, B=B, seed=seed, g=g, master=master, bfmirror=bfmirror,
        W1bf=W1bf, W2bf=W2bf, X=X, Xfit=Xfit, Xbf=Xbf, y=y, invB=1.0 / B,
    )


def reference_step(case) -> torch.Tensor:
    """Flat grads (+loss) of the bf16-mirroring reference for a case:
    ref.mlp_step for the specialized shape, ref.mlp_step_g otherwise."""
    g = case.g
    out = torch.zeros(g.nparam + 1)
    args = (case.Xbf, case.y, case.W1bf, case.W2bf, case.master, out, case.invB)
    if g.is_specialized:
        ref.mlp_step(*args)
    else:
        ref.mlp_step_g(g, *args)
    return out


# ---------------------------------------------------------------------------
# the case matrix (one place: the CPU and the GPU file both import it)
# ---------------------------------------------------------------------------

SPEC_SHAPE = (64, 32, 10)

# every step row of TABULAR_GEN_INSTANTIATIONS, <HID, RT, CPAD> -> one geometry. The
# instantiations TabularMLP already reaches at test batch sizes come first,
# the five only a direct rt= call reaches last. Together the geometries
# cover: inp = 32 (half a TK=64 tile / one TK=32 tile), one full tile, two
# tiles with a 32-wide tail, an odd tile count >= 3 double-buffered
# (150 -> 160 = 3 tiles of 64) and at TK = 32 (90 -> 96 = 3 tiles),
# in_features not a multiple of 32, hidden below the compiled width, and
# classes 2, 16, 17 and 32.
STEP_INSTANTIATIONS = [
    ((32, 64, 16), (64, 17, 16)),
    ((64, 64, 16), (150, 64, 10)),
    ((128, 32, 16), (96, 128, 16)),
    ((256, 32, 16), (90, 250, 5)),
    ((32, 128, 32), (32, 32, 17)),
    ((128, 64, 32), (200, 128, 32)),
    ((32, 128, 16), (20, 32, 2)),
    ((64, 128, 16), (70, 50, 7)),
    ((128, 64, 16), (33, 100, 3)),
    ((64, 128, 32), (100, 64, 26)),
    ((256, 32, 32), (30, 256, 20)),
]

# every predict row, <HID, RT, CPAD> -> geometry (the two never launched
# before come last)
PRED_INSTANTIATIONS = [
    ((32, 128, 16), (64, 17, 16)),
    ((64, 128, 16), (70, 50, 7)),
    ((128, 64, 16), (33, 100, 3)),
    ((256, 32, 16), (90, 250, 5)),
    ((32, 128, 32), (32, 32, 17)),
    ((128, 64, 32), (200, 128, 32)),
    ((64, 128, 32), (100, 64, 26)),
    ((256, 32, 32), (30, 256, 20)),
]

# ... and the benchmark's grids: 16 workgroups with a tail of one row, and 65
# (past the 64 lanes of one tag-poll round, last workgroup's stripe empty)
SPEC_STEP_BATCHES = (1, 127, 129, 273, 1921, 8197)
SPEC_RT = 128

DEFAULT_SEED = 5
# (shape, B) -> seed, where the default seed misses a condition the case
# list must meet (a segment norm degenerate by cancellation, or more than
# MAX_EXCLUDED of the rows inside the argmax slack); found on the CPU by
# tests/test_oracle64_cpu.py, never from a kernel's output
SEED_OVERRIDES = {
    # the only hidden unit is dead on the only row: W1/b1/W2 grads all 0
    ((1, 1, 2), 1): 7,
    # the single row's top-2 logits sit inside the argmax slack
    ((90, 250, 5), 1): 6,
}


def case_seed(shape, B):
    return SEED_OVERRIDES.get((tuple(shape), B), DEFAULT_SEED)


def step_batches(rt: int):
    return (1, rt - 1, rt + 1, 2 * rt + 17)


def inst_id(inst) -> str:
    return "<%d,%d,%d>" % inst


def shape_id(shape) -> str:
    return "x".join(map(str, shape))


def gen_step_cases():
    """[(id, (HID, RT, CPAD), shape, B, seed)] for the generalized step"""
    out = []
    for inst, shape in STEP_INSTANTIATIONS:
        for B in step_batches(inst[1]):
            out.append((f"{inst_id(inst)}-{shape_id(shape)}-B{B}", inst, shape, B,
                        case_seed(shape, B)))
    return out


def spec_step_cases():
    return [(f"spec-{shape_id(SPEC_SHAPE)}-B{B}", SPEC_SHAPE, B, case_seed(SPEC_SHAPE, B))
            for B in SPEC_STEP_BATCHES]


def predict_cases():
    """[(id, inst or None for the specialized kernel, shape, B, seed)]"""
    out = []
    for inst, shape in [(None, SPEC_SHAPE)] + PRED_INSTANTIATIONS:
        rt = SPEC_RT if inst is None else inst[1]
        name = "spec" if inst is None else inst_id(inst)
        for B in (1, rt + 1):
            out.append((f"{name}-{shape_id(shape)}-B{B}", inst, shape, B,
                        case_seed(shape, B)))
    return out


# smallest geometry end to end, and one full-mode step of the specialized
# kernel on 16 workgroups: (shape, B)
E2E_CASES = [((1, 1, 2), 1), ((1, 1, 2), 65), ((33, 250, 3), 1), ((33, 250, 3), 65),
             ((64, 32, 10), 1921)]


def check_instantiation(inst, shape):
    """The geometry really selects the instantiation it is listed under."""
    g = Geometry(*shape)
    assert (g.hid, g.cpad) == (inst[0], inst[2]), (inst, shape)


def header_instantiations():
    """([step <HID, RT, CPAD>], [predict <HID, RT, CPAD>]) as the one table
    macro of hip/tabular_launch.h lists them, and, checked on the way, that
    tabular_gen.hip holds no list of its own: its dispatch helpers are
    instantiated through the macro's parameters only, once per dispatcher."""
    import re
    from pathlib import Path

    hip = Path(ref.__file__).parent / "hip"
    header = (hip / "tabular_launch.h").read_text()
    macro = re.search(r"#define TABULAR_GEN_INSTANTIATIONS\(X\)((?:.*\\\n)+.*\n)", header)
    rows = [tuple(map(int, m)) for m in
            re.findall(r"X\((\d+), (\d+), (\d+), ([01])\)", macro.group(1))]
    assert len(re.findall(r"\bX\(", macro.group(1))) == len(rows)

    src = (hip / "tabular_gen.hip").read_text()
    assert len(re.findall(r"TABULAR_GEN_INSTANTIATIONS\(", src)) == 2
    assert re.findall(r"launch_step_gen_t<([^>]*)>", src) == ["H, R, C, HEAD"]
    assert re.findall(r"launch_predict_gen_t<([^>]*)>", src) == ["H, R, C, HEAD"]
    uses = re.findall(r"mlp_(?:step|predict)_gen_kernel<([^>]*)>", src)
    assert uses and set(uses) == {"HID, RT, CP, HEAD"}
    assert not re.search(r"_CASE\(", src)
    return [r[:3] for r in rows], [r[:3] for r in rows if r[3]]


# Adam bound pieces ----------------------------------------------------------


# the moments-against-the-written-formula tests (adam_moments32): kernels and
# geometries of test_gpu_oracle.py's Adam tests, their gradient seed, 4 steps
ADAM_KERNELS = [("adam_step", (64, 32, 10)), ("adam_step_gen", (100, 50, 7)),
                ("reduce_adam_gen", (100, 50, 7))]
ADAM_MOMENT_STEPS = 4
ADAM_GRAD_SEED = 17


def moment_envelopes(grads_per_step, b1, b2):
    """The Adam recurrences run on |g| and g^2 in fp64: the magnitudes the
    fp32 moment error is bounded against (4 t 2^-24 of them at step t)."""
    am = torch.zeros_like(grads_per_step[0], dtype=F64)
    av = torch.zeros_like(am)
    out = []
    for gr in grads_per_step:
        gr = gr.to(F64)
        am = b1 * am + (1.0 - b1) * gr.abs()
        av = b2 * av + (1.0 - b2) * gr * gr
        out.append((am.clone(), av.clone()))
    return out


def adam_gradients(n: int, steps: int, seed: int):
    """A fresh random gradient per step: magnitudes log-uniform over
    [1e-6, 10], random signs, ~10% exact zeros per step, and a fixed set
    of parameters (every 7th) whose gradient is zero throughout."""
    gen = torch.Generator().manual_seed(seed)
    always_zero = torch.zeros(n, dtype=torch.bool)
    always_zero[::7] = True
    out = []
    for _ in range(steps):
        mag = 10.0 ** (torch.rand(n, generator=gen) * 7.0 - 6.0)
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
        gr = (mag * sign).float()
        gr[torch.rand(n, generator=gen) < 0.1] = 0.0
        gr[always_zero] = 0.0
        out.append(gr)
    return out, always_zero


def gamma(n: int) -> float:
    """Higham's gamma_n for fp32 summation of n terms"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)
