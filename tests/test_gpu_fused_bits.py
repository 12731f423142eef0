"""The fused step's output bits, pinned across builds.

tests/golden/fused_step_bits.json holds SHA-256 digests of what three
mlp_step_fused launches leave behind (master, m, v, bfmirror, the three
losses, t_dev), recorded with benchmarks/record_fused_bits.py on the commit
before the kernel's prologue, bias reads, bias-grad hand-back and LDS stores
were rewritten. This test runs the same recipe (it imports it from the
recorder, so the two cannot drift apart) and compares digests: an edit to
the kernel that moves one bit of any of them fails here, where the tests
that compare two paths of ONE build would move together and pass.

Grids, as (n_wg, rows in the last workgroup), the smallest at which such an
edit can go wrong: (1, 1) one valid row, every other row on the tail path
and every bias sum a sum of zeros; (1, 127); (2, 1) Adam-state prefetch on;
(3, 128) no tail; (9, 1) and (17, 1) the unrolled chains plus a remainder.
Each with the packed weight image and without, in full mode and in
reduce-only mode followed by adam_step.
"""

import importlib.util
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "fused_step_bits.json"


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_fused_bits", REPO / "benchmarks" / "record_fused_bits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _recorder()
CASES = rec.all_cases()


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_golden_covers_exactly_the_cases(golden):
    assert sorted(golden) == sorted(rec.case_id(*c) for c in CASES)
    assert all(sorted(v) == sorted(rec.ARRAYS) for v in golden.values())


@pytest.mark.parametrize("case", CASES, ids=[rec.case_id(*c) for c in CASES])
def test_fused_step_bits_match_the_recorded_digests(ext, golden, case):
    got = rec.run_case(ext, *case)
    want = golden[rec.case_id(*case)]
    moved = [k for k in rec.ARRAYS if got[k] != want[k]]
    assert not moved, f"{rec.case_id(*case)}: bits of {moved} differ from the recorded step"
