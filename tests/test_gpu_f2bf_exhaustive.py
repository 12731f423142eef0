"""f2bf (hip/tabular_common.h) on gfx950 is the hardware convert
v_cvt_pk_bf16_f32; everywhere else, and as the reference here, it is the
integer round-to-nearest-even form f2bf_soft. The f2bf_selftest kernel runs
all 2^32 float bit patterns through f2bf, through both halves of f2bf_pair
and through f2bf_soft in one launch.

The two forms must agree on every input that is not a NaN, denormals
included: the output bits of every kernel that rounds to bf16 rest on it. A
NaN input may give another NaN, but never a number."""

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def result():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    n_diff, examples, n_nan_lost = hip_ext(required=True).f2bf_selftest()
    print(f"f2bf_selftest: {n_diff} non-NaN inputs differ, first "
          f"{[hex(int(u)) for u in examples]}; {n_nan_lost} NaN inputs lose their NaN")
    return n_diff, examples, n_nan_lost


def test_every_non_nan_input_rounds_as_the_integer_form(result):
    n_diff, examples, _ = result
    assert n_diff == 0, (
        f"{n_diff} of the non-NaN bit patterns round differently, first "
        f"{[hex(int(u)) for u in examples]}")
    assert examples.numel() == 0


def test_a_nan_stays_a_nan(result):
    assert result[2] == 0, f"{result[2]} NaN inputs came out as a number"
