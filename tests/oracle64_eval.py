"""Plain fp64 oracle for the evaluation kernels (mlp_eval_gen_kernel, both
heads), plus the case matrix their tests share: tests/test_eval_cpu.py
validates the oracle, the bf16-mirroring reference and the cases on the CPU,
tests/test_gpu_eval.py runs the HIP kernels against them. The forward is
tests/oracle64.py's; nothing here rounds.

No tests live in this module.
"""

from types import SimpleNamespace

import torch

import oracle64 as o64
import oracle64_reg as o64r
from oracle64 import F64

# share of a case's rows that may sit inside the argmax rounding slack (the
# rows the correct-count comparison against the oracle has to leave open)
MAX_SLACK_SHARE = 0.05


def eval64_cls(case):
    """fp64 mean cross-entropy and correct count of a classifier case
    (oracle64.make_case): loss, correct, per-row hits, logits, H."""
    g = case.g
    W1, b1, W2, b2 = o64._real_operands(g, case.W1bf, case.W2bf, case.master)
    X = case.Xbf.to(F64)[:, : g.in_features]
    _, H, logits = o64.forward64(X, W1, b1, W2, b2)
    yl = case.y.long()
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    loss = float(-logp[torch.arange(case.B), yl].mean())
    hits = logits.argmax(dim=1) == yl
    return SimpleNamespace(loss=loss, correct=int(hits.sum()), hits=hits, logits=logits, H=H)


def eval64_reg(case):
    """fp64 metrics of a regression case (oracle64_reg.make_case_reg): loss =
    mean over rows of 0.5 * sum_c (z - y)^2, mse [T] per column, H, z."""
    g = case.g
    W1, b1, W2, b2 = o64._real_operands(g, case.W1bf, case.W2bf, case.master)
    X = case.Xbf.to(F64)[:, : g.in_features]
    _, H, z = o64.forward64(X, W1, b1, W2, b2)
    d = z - case.Yt.to(F64)[:, : g.classes]
    return SimpleNamespace(loss=float(0.5 * (d * d).sum() / case.B),
                           mse=(d * d).mean(dim=0), H=H, z=z)


def count_window(case, o):
    """(lo, hi, slack_share): the correct counts the rounding of H to bf16
    admits. Rows whose top-2 margin clears the slack (oracle64.clear_rows)
    must be scored as the oracle scores them; each other row may go either
    way."""
    clear = o64.clear_rows(o.logits, o.H, case.W2bf, case.g)
    lo = int((o.hits & clear).sum())
    open_rows = int((~clear).sum())
    return lo, lo + open_rows, open_rows / case.B


# ---------------------------------------------------------------------------
# the case matrix
# ---------------------------------------------------------------------------


def eval_batches(rt: int, gpu: bool = False):
    """Around a workgroup's row count; on the GPU also ten workgroups with
    a tail (the fp64 finish over more than a handful of rows)."""
    return o64.step_batches(rt) + ((9 * rt + 5,) if gpu else ())


DEFAULT_SEED = 5
# (head, shape, B) -> seed where the default seed puts more than
# MAX_SLACK_SHARE of the rows inside the argmax slack; found on the CPU by
# tests/test_eval_cpu.py from the oracle and the mirror, never from a kernel
SEED_OVERRIDES = {
    ("cls", (64, 17, 16), 129): 6,
    ("cls", (64, 17, 16), 273): 6,
    ("cls", (200, 128, 32), 145): 6,
    ("cls", (200, 128, 32), 581): 9,
    ("cls", (100, 64, 26), 273): 6,
    ("cls", (100, 64, 26), 1157): 6,
}


def case_seed(head: str, shape, B: int) -> int:
    return SEED_OVERRIDES.get((head, tuple(shape), B), DEFAULT_SEED)


def cls_cases(gpu: bool = False):
    """[(id, (HID, RT, CPAD), shape, B, seed)], classifier head"""
    return [(f"{o64.inst_id(inst)}-{o64.shape_id(shape)}-B{B}", inst, shape, B,
             case_seed("cls", shape, B))
            for inst, shape in o64.PRED_INSTANTIATIONS for B in eval_batches(inst[1], gpu)]


def reg_cases(gpu: bool = False):
    """[(id, (HID, RT, CPAD), shape, B, seed)], regression head"""
    return [(f"{o64.inst_id(inst)}-{o64.shape_id(shape)}-B{B}", inst, shape, B,
             case_seed("reg", shape, B))
            for inst, shape in o64r.PRED_INSTANTIATIONS for B in eval_batches(inst[1], gpu)]
