"""The output bits of mlp_step and mlp_train_steps, pinned across builds.

Both kernels run the same fwd/bwd chunk as the fused step, whose bits
tests/test_gpu_fused_bits.py pins, but each has an epilogue of its own
(global atomics; Adam in LDS with the accumulators carried over chunks), and
the tests that compare two paths of ONE build move together when the chunk
changes. tests/golden/chunk_step_bits.json holds SHA-256 digests recorded with
benchmarks/record_chunk_bits.py on the commit before the chunk's transposed
LDS images were replaced by transposed reads. This test runs the same recipe
(imported from the recorder, so the two cannot drift apart) and compares.

Shapes, the smallest at which such an edit can go wrong: mlp_step with one
workgroup at B = 1 (one valid row), 16 (one wave's rows), 17, 127 and 128 (no
tail); one workgroup adds once onto zeroed grads, so its result is
deterministic, where a larger grid's atomics land in arrival order.
mlp_train_steps with two steps at B = 128 (one chunk per step) and B = 256
(two chunks: the X image is refilled while the accumulators carry over).
"""

import importlib.util
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / "tests" / "golden" / "chunk_step_bits.json"


def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_chunk_bits", REPO / "benchmarks" / "record_chunk_bits.py")
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
    assert all(sorted(golden[rec.case_id(*c)]) == sorted(rec.arrays_of(c[0])) for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[rec.case_id(*c) for c in CASES])
def test_chunk_step_bits_match_the_recorded_digests(ext, golden, case):
    got = rec.run_case(ext, *case)
    want = golden[rec.case_id(*case)]
    moved = [k for k in rec.arrays_of(case[0]) if got[k] != want[k]]
    assert not moved, f"{rec.case_id(*case)}: bits of {moved} differ from the recorded step"
