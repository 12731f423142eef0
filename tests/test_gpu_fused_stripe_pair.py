"""The stripe of the fused step (mlp_step_fused_kernel) at the grid sizes at
which its sum and its Adam tail take another path. A stripe lane issues the
first batch of its first pass (the first 16 slabs: two groups of eight, one
group and the remainder, or the remainder alone) from addresses it computed
before the last barrier, keeps that pass's Adam state in registers, and takes
later batches and later passes the general way, with later passes' state in
LDS.

Grids: 1, 2, 5 make several passes; 6 is the first single-pass grid; 11, 12
and 13 have one group and a remainder in the first batch (12 is where two
lanes could share a parameter, profiles/r15_fused_stripe_tail.md); 16 is the
benchmark's grid; 17 adds a remainder behind the first batch, 24 an 8-slab
batch; 33 has a stripe of 80 words, which ends inside a wave. B = 128 * n_wg
- 5: the last workgroup is partial.

Every comparison is on integers. The reduce-only expectation is rebuilt on
the host from the slabs the launch left, in the order docs/kernels.md
documents and not from the kernel's code:

  chain k (k = 0..7) sums the slabs k, k + 8, k + 16, ... of the whole groups
  of eight, in that order, starting from 0;
  the n_wg % 8 slabs behind the last whole group are added to chain 0, in order;
  g = ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)).

The Adam check drives a twin from equal state down the two-kernel path (a
reduce-only launch, then adam_step_kernel): both apply adam_update to the
same sums, so there is no tolerance. After every launch the launch counter
has advanced by one and every slab carries it as its tag."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 128
LR = 1e-3
T0 = 3
N_WGS = [1, 2, 5, 6, 11, 12, 13, 16, 17, 24, 33]


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@functools.lru_cache(maxsize=None)
def _batch(n_wg):
    """Seeded minibatch of 128 * n_wg - 5 rows on the device; never written"""
    B = ROWS * n_wg - 5
    g = torch.Generator().manual_seed(1500 + n_wg)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X.to("cuda:0"), y.to("cuda:0")


@functools.lru_cache(maxsize=None)
def _primer():
    """Seeded non-zero biases and Adam moments (CPU), shared by all cases"""
    from unionml_amd.ops import reference as ref

    g = torch.Generator().manual_seed(1515)
    n = ref.NPARAM
    return {
        "b1": torch.randn(ref.DIGITS.hid, generator=g) * 0.1,
        "b2": torch.randn(ref.DIGITS.cpad, generator=g) * 0.1,
        "m": torch.randn(n, generator=g) * 1e-2,
        "v": torch.rand(n, generator=g) * 1e-3 + 1e-6,
    }


def _model(n_wg):
    """Non-zero biases, non-zero m / v, t_dev = 3; two calls give equal state"""
    from unionml_amd.ops.tabular import TabularMLP

    dev = torch.device("cuda:0")
    c = TabularMLP(device=dev, seed=6)
    g, p = c.g, _primer()
    c.master[g.off_b1 : g.off_b1 + g.hid] = p["b1"].to(dev)
    c.master[g.off_b2 : g.off_b2 + g.cpad] = p["b2"].to(dev)
    c.bfmirror.copy_(c.master.bfloat16())
    c._build_wimg()
    c.m.copy_(p["m"].to(dev))
    c.v.copy_(p["v"].to(dev))
    c.t_dev.fill_(T0)
    c._ensure_slabs(n_wg)
    return c


def _adam_args():
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    return LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS


def _launch(ext, c, Xbf, y, loss_out, grads_out):
    assert ext.mlp_step_fused(
        Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev, c.slabs,
        c.counter, loss_out, 1.0 / Xbf.size(0), *_adam_args(), grads_out=grads_out,
        wimg=c.wimg)


def _check_launch_state(c, n_wg, launches, tag):
    """counter advanced by one per launch; every slab's tag (word NPARAM + 1,
    as an integer) equals it"""
    from unionml_amd.ops import reference as ref

    counter = int(c.counter.item())
    assert counter == launches, f"{tag}: counter {counter} after {launches} launch(es)"
    tags = c.slabs[:n_wg, ref.NPARAM + 1].contiguous().view(torch.int32).cpu().numpy()
    assert (tags == counter).all(), f"{tag}: slab tags {tags.tolist()} != {counter}"


def documented_sum(slabs: np.ndarray) -> np.ndarray:
    """slabs [n_wg][words] float32 -> the documented sum per word, float32"""
    n_wg = slabs.shape[0]
    whole = n_wg - n_wg % 8
    chains = [np.zeros(slabs.shape[1], dtype=np.float32) for _ in range(8)]
    for w in range(whole):
        chains[w % 8] = chains[w % 8] + slabs[w]
    for w in range(whole, n_wg):
        chains[0] = chains[0] + slabs[w]
    g = chains
    return ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]))


def _as_int(x):
    return x.view(torch.int16 if x.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("n_wg", N_WGS, ids=[f"wg{n}" for n in N_WGS])
def test_reduce_only_sum_is_the_documented_order(ext, n_wg):
    from unionml_amd.ops import reference as ref

    Xbf, y = _batch(n_wg)
    c = _model(n_wg)
    n = ref.NPARAM + 1                        # every parameter, then the loss
    grads = torch.full((n,), float("nan"), device=Xbf.device)
    loss_out = torch.zeros(1, device=Xbf.device)
    _launch(ext, c, Xbf, y, loss_out, grads)
    torch.cuda.synchronize()
    _check_launch_state(c, n_wg, 1, f"n_wg={n_wg}")

    slabs = c.slabs[:n_wg, :n].cpu().numpy()
    got = grads.cpu().numpy()
    assert np.isfinite(slabs).all() and np.isfinite(got).all()
    assert np.abs(slabs[:, : ref.NPARAM]).max() > 0, "the slabs hold no gradient"
    want = documented_sum(slabs)
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), (
        f"n_wg={n_wg}: {int(diff.sum())} of {n} sums differ from the documented order, "
        f"first at word {int(np.flatnonzero(diff)[0])}")
    assert int(c.t_dev.item()) == T0, "a reduce-only launch leaves t_dev alone"


@pytest.mark.parametrize("n_wg", N_WGS, ids=[f"wg{n}" for n in N_WGS])
def test_fused_adam_equals_reduce_only_plus_adam_step(ext, n_wg):
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import TabularMLP

    Xbf, y = _batch(n_wg)
    a, b = _model(n_wg), _model(n_wg)
    master0 = a.master.clone()
    loss_a = torch.zeros(1, device=Xbf.device)
    _launch(ext, a, Xbf, y, loss_a, None)
    grads = torch.full((ref.NPARAM + 1,), float("nan"), device=Xbf.device)
    _launch(ext, b, Xbf, y, torch.zeros(1, device=Xbf.device), grads)
    ext.adam_step(b.master, b.bfmirror, grads, b.m, b.v, b.t_dev, *_adam_args(), wimg=b.wimg)
    torch.cuda.synchronize()
    tag = f"n_wg={n_wg}"
    _check_launch_state(a, n_wg, 1, tag + " fused")
    _check_launch_state(b, n_wg, 1, tag + " reduce-only")

    assert int(a.t_dev.item()) == T0 + 1 and int(b.t_dev.item()) == T0 + 1, tag
    assert not torch.equal(a.master, master0), f"{tag}: the weights did not move"
    for name in ("master", "m", "v", "bfmirror", "t_dev", "wimg"):
        xa, xb = getattr(a, name), getattr(b, name)
        assert torch.isfinite(xa.float()).all(), f"{tag}: {name} not finite"
        diff = _as_int(xa) != _as_int(xb)
        assert not diff.any(), (
            f"{tag}: {name} differs in {int(diff.sum())} of {diff.numel()} words, "
            f"first at {int(diff.flatten().nonzero()[0])}")
    # the loss is word NPARAM of the reduce-only sum
    assert torch.equal(_as_int(loss_a), _as_int(grads[ref.NPARAM : ref.NPARAM + 1])), tag
    # the fused launch kept its image in step with its mirror
    assert torch.equal(a.bfmirror, a.master.bfloat16()), tag
    fresh = TabularMLP(device=Xbf.device, seed=6)
    fresh.master.copy_(a.master)       # _build_wimg rounds master as bfmirror does
    fresh._build_wimg()
    assert torch.equal(_as_int(a.wimg), _as_int(fresh.wimg)), f"{tag}: wimg != image of bfmirror"
