"""The stripe sum of the fused step (mlp_step_fused_kernel), against the order
docs/kernels.md documents for it, at every grid size at which the sum takes
another path: 16-slab batches, an 8-slab batch, the remainder's batch of up
to 7, and their combinations.

One reduce-only launch (grads_out) per grid. The slabs it leaves in memory
are the operands; the expectation is rebuilt from them on the host in float32,
from the documented order and not from the kernel's code:

  chain k (k = 0..7) sums the slabs k, k + 8, k + 16, ... of the whole groups
  of eight, in that order, starting from 0;
  the n_wg % 8 slabs behind the last whole group are added to chain 0, in order;
  g = ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)).

The comparison is on integers. How the kernel addresses and batches its
loads does not enter the expectation, so the test holds for any form of the
loads (profiles/r14_fused_instruction_diet.md tried one)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS = 128
# 1, 2, 7: remainder only. 8: one 8-batch. 9, 15: 8-batch + remainder. 16: one
# 16-batch (the benchmark's grid). 17, 23: 16 + remainder. 24: 16 + 8. 25, 31:
# 16 + 8 + remainder. 32: two 16-batches. 33: two 16-batches + remainder.
N_WGS = [1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33]


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


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


@pytest.mark.parametrize("n_wg", N_WGS, ids=[f"wg{n}" for n in N_WGS])
def test_stripe_sum_is_the_documented_order(ext, n_wg):
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import TabularMLP

    dev = torch.device("cuda:0")
    B = ROWS * n_wg - 5                      # the last workgroup is partial
    gen = torch.Generator().manual_seed(900 + n_wg)
    Xbf = (torch.randn(B, 64, generator=gen) * 1.2 + 0.1).bfloat16().to(dev)
    y = torch.randint(0, 10, (B,), generator=gen, dtype=torch.int32).to(dev)

    c = TabularMLP(device=dev, seed=6)
    c.master[c.g.off_b1 : c.g.off_b1 + c.g.hid] = (torch.randn(c.g.hid, generator=gen) * 0.1).to(dev)
    c.bfmirror.copy_(c.master.bfloat16())
    c._build_wimg()
    c._ensure_slabs(n_wg)
    n = ref.NPARAM + 1                        # every parameter, then the loss
    grads = torch.full((n,), float("nan"), device=dev)
    loss_out = torch.zeros(1, device=dev)
    assert ext.mlp_step_fused(
        Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev, c.slabs,
        c.counter, loss_out, 1.0 / B, 1e-3, 0.9, 0.999, 1e-8, grads_out=grads, wimg=c.wimg)
    torch.cuda.synchronize()

    slabs = c.slabs[:n_wg, :n].cpu().numpy()
    got = grads.cpu().numpy()
    assert np.isfinite(slabs).all() and np.isfinite(got).all()
    assert np.abs(slabs[:, : ref.NPARAM]).max() > 0, "the slabs hold no gradient"
    want = documented_sum(slabs)
    diff = got.view(np.int32) != want.view(np.int32)
    assert not diff.any(), (
        f"n_wg={n_wg}: {int(diff.sum())} of {n} sums differ from the documented order, "
        f"first at word {int(np.flatnonzero(diff)[0])}")
