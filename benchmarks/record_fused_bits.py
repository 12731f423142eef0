"""Record the fused step's output bits: SHA-256 digests of what three
mlp_step_fused launches leave behind, for tests/test_gpu_fused_bits.py.

    python benchmarks/record_fused_bits.py > tests/golden/fused_step_bits.json

Run it on the commit whose bits are to be pinned (needs the GPU). Every case
starts from TabularMLP(seed=6) and steps three times on the seeded batch of
tests/test_gpu_fused_exact.py::_batch, in full mode (Adam in the kernel) or
in reduce-only mode followed by adam_step, with the packed weight image or
without. Digested: the raw bytes of master, m, v, bfmirror, the three
steps' losses and t_dev.
"""

import hashlib
import json
import sys
from pathlib import Path

import torch

LR = 1e-3
ROWS = 128
N_STEPS = 3
MODEL_SEED = 6

# (n_wg, rows in the last workgroup): B = 128 * (n_wg - 1) + r
GRIDS = [(1, 1), (1, 127), (2, 1), (3, 128), (9, 1), (17, 1)]
MODES = ("full", "reduce+adam_step")
ARRAYS = ("master", "m", "v", "bfmirror", "loss", "t_dev")


def case_id(n_wg, r, use_wimg, mode):
    return f"wg{n_wg}-r{r}/{'wimg' if use_wimg else 'plain'}/{mode}"


def batch(B, seed):
    """tests/test_gpu_fused_exact.py::_batch"""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X.to("cuda:0"), y.to("cuda:0")


def _sha(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def run_case(ext, n_wg, r, use_wimg, mode):
    """Digests of one case's final state"""
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS, TabularMLP

    adam = (LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS)
    B = ROWS * (n_wg - 1) + r
    Xbf, y = batch(B, seed=100 + n_wg)
    c = TabularMLP(device=torch.device("cuda:0"), seed=MODEL_SEED)
    c._ensure_slabs(n_wg)
    wimg = c.wimg if use_wimg else None
    loss_slot = c.grads[ref.NPARAM : ref.NPARAM + 1]
    losses = []
    for _ in range(N_STEPS):
        ok = ext.mlp_step_fused(
            Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev,
            c.slabs, c.counter, loss_slot, 1.0 / B, *adam,
            grads_out=c.grads if mode != "full" else None, wimg=wimg)
        assert ok, "mlp_step_fused refused the launch"
        if mode != "full":
            ext.adam_step(c.master, c.bfmirror, c.grads, c.m, c.v, c.t_dev, *adam, wimg=wimg)
        losses.append(loss_slot.clone())
    torch.cuda.synchronize()
    assert int(c.t_dev.item()) == N_STEPS and int(c.counter.item()) == N_STEPS
    state = {"master": c.master, "m": c.m, "v": c.v, "bfmirror": c.bfmirror,
             "loss": torch.cat(losses), "t_dev": c.t_dev}
    return {k: _sha(state[k]) for k in ARRAYS}


def all_cases():
    return [(n_wg, r, use_wimg, mode) for n_wg, r in GRIDS for use_wimg in (False, True)
            for mode in MODES]


def main():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from unionml_amd.ops import hip_ext

    ext = hip_ext(required=True)
    out = {case_id(*case): run_case(ext, *case) for case in all_cases()}
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
