"""The tail of the fused step (mlp_step_fused_kernel) behind its hand-off:
wave 0 only hands off, waves 1 to 7 own the stripe of the Adam-state
prefetch and of the reduce loop, and the Adam bias corrections are computed
while the tag poll waits, by waves 1 and 2, from t_dev, in fused mode only,
and reach the stripe threads through LDS.

Every check compares two model instances driven down different paths from
one state, as integers: the fused launch against a reduce-only launch
followed by adam_step_kernel. Both apply adam_update to the same slab sums
with the same adam_bias_corr(beta1, beta2, t), so there is no tolerance in
this file."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3
ROWS = 128            # rows per workgroup of the specialized kernel

# B = 128 * (n_wg - 1) + 1. Stripe iterations per thread of waves 1 to 7:
# 1 workgroup: 6, prefetch off; 2: 3; 5: 2; 6: the first single-iteration
# stripe; 16: the workload's own grid; 17: the remainder chain; 65: a second
# poll round and an empty last stripe.
N_WGS = [1, 2, 5, 6, 16, 17, 65]
# t_dev before the step: pow sees t = 1, 2 and 1000
T_PRESET = [0, 1, 999]


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _batch(n_wg):
    """Seeded asymmetric minibatch of 128 * (n_wg - 1) + 1 rows, on the
    device; computed once per grid and never written."""
    B = ROWS * (n_wg - 1) + 1
    g = torch.Generator().manual_seed(500 + n_wg)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X.to("cuda:0"), y.to("cuda:0")


@functools.lru_cache(maxsize=None)
def _primer():
    """Seeded non-zero biases and Adam moments (CPU), shared by all cases"""
    from unionml_amd.ops import reference as ref

    g = torch.Generator().manual_seed(4242)
    n = ref.NPARAM
    return {
        "b1": torch.randn(ref.DIGITS.hid, generator=g) * 0.1,
        "b2": torch.randn(ref.DIGITS.cpad, generator=g) * 0.1,
        "m": torch.randn(n, generator=g) * 1e-2,
        "v": torch.rand(n, generator=g) * 1e-3 + 1e-6,
    }


def _adam_args():
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    return LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS


def _model(dev, n_wg, t0):
    """A model with non-zero biases, non-zero m / v and t_dev preset to t0;
    two calls give identical state"""
    from unionml_amd.ops.tabular import TabularMLP

    c = TabularMLP(device=dev, seed=6)
    g, p = c.g, _primer()
    c.master[g.off_b1 : g.off_b1 + g.hid] = p["b1"].to(dev)
    c.master[g.off_b2 : g.off_b2 + g.cpad] = p["b2"].to(dev)
    c.bfmirror.copy_(c.master.bfloat16())
    c._build_wimg()
    c.m.copy_(p["m"].to(dev))
    c.v.copy_(p["v"].to(dev))
    c.t_dev.fill_(t0)
    c._ensure_slabs(n_wg)
    return c


def _loss(c):
    from unionml_amd.ops import reference as ref

    return c.grads[ref.NPARAM : ref.NPARAM + 1]


def _fused(ext, c, Xbf, y):
    assert ext.mlp_step_fused(
        Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev,
        c.slabs, c.counter, _loss(c), 1.0 / Xbf.size(0), *_adam_args(),
        grads_out=None, wimg=c.wimg,
    )


def _reduce_only(ext, c, Xbf, y):
    assert ext.mlp_step_fused(
        Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev,
        c.slabs, c.counter, _loss(c), 1.0 / Xbf.size(0), *_adam_args(),
        grads_out=c.grads, wimg=c.wimg,
    )


def _adam_step(ext, c):
    ext.adam_step(c.master, c.bfmirror, c.grads, c.m, c.v, c.t_dev, *_adam_args(), wimg=c.wimg)


def _as_int(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


def _state(c):
    return {"master": c.master, "m": c.m, "v": c.v, "bfmirror": c.bfmirror,
            "wimg": c.wimg, "t_dev": c.t_dev, "loss": _loss(c)}


def _assert_same_bits(a, b, what):
    sa, sb = _state(a), _state(b)
    for k in sa:
        assert torch.isfinite(sa[k].float()).all(), f"{what}: {k} not finite"
        diff = _as_int(sa[k]) != _as_int(sb[k])
        assert not diff.any(), (
            f"{what}: {k} differs in {int(diff.sum())} of {diff.numel()} words, "
            f"first at {int(diff.flatten().nonzero()[0])}")


@pytest.mark.parametrize("t0", T_PRESET, ids=[f"t{t}" for t in T_PRESET])
@pytest.mark.parametrize("n_wg", N_WGS, ids=[f"wg{n}" for n in N_WGS])
def test_fused_step_equals_reduce_only_plus_adam_step(ext, dev, n_wg, t0):
    """One step. Model a: the fused launch (waves 1 to 7 sum their stripe and
    apply Adam from the prefetched state, with the corrections computed beside
    the tag poll). Model b, from identical state: a reduce-only launch,
    which computes no correction, then adam_step_kernel. master, m, v,
    bfmirror, wimg, t_dev and the loss are equal as integers."""
    Xbf, y = _batch(n_wg)
    a, b = _model(dev, n_wg, t0), _model(dev, n_wg, t0)
    master0 = a.master.clone()
    _fused(ext, a, Xbf, y)
    _reduce_only(ext, b, Xbf, y)
    _adam_step(ext, b)
    torch.cuda.synchronize()
    tag = f"n_wg={n_wg} t_dev={t0}"
    assert int(a.t_dev.item()) == t0 + 1 and int(a.counter.item()) == 1, tag
    assert int(b.counter.item()) == 1, tag
    assert not torch.equal(a.master, master0), f"{tag}: the weights did not move"
    assert torch.equal(a.bfmirror, a.master.bfloat16()), tag
    _assert_same_bits(a, b, tag)


@pytest.mark.parametrize("n_wg", [2, 17], ids=["wg2", "wg17"])
def test_mixed_reduce_only_and_fused_launches(ext, dev, n_wg):
    """Eight launches on model a, reduce-only and fused in turn; model b runs
    the same sequence through the two-kernel path (a reduce-only launch whose
    sums are dropped, then a reduce-only launch and adam_step). The launch
    counter reaches 8 and t_dev 4 on both, and the states are equal as
    integers: a correction computed from the launch counter instead of t_dev
    would use t = 2, 4, 6, 8 in model a."""
    Xbf, y = _batch(n_wg)
    a, b = _model(dev, n_wg, 0), _model(dev, n_wg, 0)
    for _ in range(4):
        _reduce_only(ext, a, Xbf, y)
        _fused(ext, a, Xbf, y)
        _reduce_only(ext, b, Xbf, y)
        _reduce_only(ext, b, Xbf, y)
        _adam_step(ext, b)
    torch.cuda.synchronize()
    tag = f"n_wg={n_wg}, 8 mixed launches"
    for c in (a, b):
        assert int(c.counter.item()) == 8 and int(c.t_dev.item()) == 4, tag
    _assert_same_bits(a, b, tag)
