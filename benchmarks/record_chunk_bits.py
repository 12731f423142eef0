"""Record the output bits of the two other kernels built on chunk_fwd_bwd,
mlp_step and mlp_train_steps: SHA-256 digests for tests/test_gpu_chunk_bits.py.

    python benchmarks/record_chunk_bits.py > tests/golden/chunk_step_bits.json

Run it on the commit whose bits are to be pinned (needs the GPU). The fused
step has its own pins (record_fused_bits.py); these two kernels share its
fwd/bwd chunk but not its epilogue, and nothing else pins them across builds.

  mlp_step/B<n>     one launch on zeroed grads, from TabularMLP(seed=6) on the
                    seeded batch of record_fused_bits.batch. One workgroup
                    only (B <= 128): it adds once onto zeros, so the result
                    does not depend on the order in which atomics arrive.
                    Digested: grads (the loss is its last word).
  train_steps/B<n>  one launch of two optimizer steps over N = 2*B rows (each
                    step its own batch). B = 128 is one chunk per step, B = 256
                    two: the X image is refilled while the weight-grad
                    accumulators carry over. Digested: master, m, v, bfmirror,
                    loss, t_dev.
"""

import hashlib
import json
import sys
from pathlib import Path

import torch

LR = 1e-3
MODEL_SEED = 6
N_STEPS = 2

STEP_B = [1, 16, 17, 127, 128]
STEPS_B = [128, 256]
STEP_ARRAYS = ("grads",)
STEPS_ARRAYS = ("master", "m", "v", "bfmirror", "loss", "t_dev")


def case_id(kind, B):
    return f"{kind}/B{B}"


def arrays_of(kind):
    return STEP_ARRAYS if kind == "mlp_step" else STEPS_ARRAYS


def batch(B, seed):
    """benchmarks/record_fused_bits.py::batch"""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X.to("cuda:0"), y.to("cuda:0")


def _sha(t):
    raw = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
    return hashlib.sha256(raw).hexdigest()


def _model():
    """TabularMLP(seed=6) with non-zero, asymmetric biases (it starts them at
    zero, which would hide a bias read gone wrong)"""
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import TabularMLP

    c = TabularMLP(device=torch.device("cuda:0"), seed=MODEL_SEED)
    g = torch.Generator().manual_seed(MODEL_SEED + 1)
    hid, cls = ref.HID, ref.CLS   # b2's pad columns stay zero
    bias = (torch.randn(hid + cls, generator=g) * 0.3 + 0.05).to("cuda:0")
    c.master[ref.OFF_B1 : ref.OFF_B1 + hid] = bias[:hid]
    c.master[ref.OFF_B2 : ref.OFF_B2 + cls] = bias[hid:]
    return c


def run_case(ext, kind, B):
    """Digests of one case's final state"""
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    c = _model()
    if kind == "mlp_step":
        assert B <= 128, "one workgroup: more would add in arrival order"
        Xbf, y = batch(B, seed=200 + B)
        grads = torch.zeros(ref.NPARAM + 1, device="cuda:0")
        ext.mlp_step(Xbf, y, c.W1bf, c.W2bf, c.master, grads, 1.0 / B)
        torch.cuda.synchronize()
        state = {"grads": grads}
    else:
        Xbf, y = batch(N_STEPS * B, seed=300 + B)
        loss_out = torch.zeros(1, device="cuda:0")
        ok = ext.mlp_train_steps(Xbf, y, B, N_STEPS, c.master, c.bfmirror, c.m, c.v,
                                 c.t_dev, loss_out, LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS)
        assert ok, "mlp_train_steps refused the launch"
        torch.cuda.synchronize()
        assert int(c.t_dev.item()) == N_STEPS
        state = {"master": c.master, "m": c.m, "v": c.v, "bfmirror": c.bfmirror,
                 "loss": loss_out, "t_dev": c.t_dev}
    return {k: _sha(state[k]) for k in arrays_of(kind)}


def all_cases():
    return [("mlp_step", B) for B in STEP_B] + [("train_steps", B) for B in STEPS_B]


def main():
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    from unionml_amd.ops import hip_ext

    ext = hip_ext(required=True)
    out = {case_id(*case): run_case(ext, *case) for case in all_cases()}
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")


if __name__ == "__main__":
    main()
