"""Shuffled epochs on the CPU path: the keyed permutation
(ops/reference.py shuffle_perm) is a bijection, is keyed by seed and step
counter, is uniform enough, and train_epochs(shuffle=True) is exactly the
manual loop "permute by the current step counter, train one epoch"."""

import pytest
import torch

from shuffle_fixtures import (
    BATCH, MODEL_IDS, MODELS, assert_same_state, make_data, make_model, manual_epochs,
)
from unionml_amd.ops import reference as ref

# ---------------------------------------------------------------------------
# the permutation
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("t", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 17, 1797, 65536, 65537])
def test_permutation_is_a_bijection(n, t):
    perm = ref.shuffle_perm(n, 0, t)
    assert perm.dtype == torch.int64 and perm.shape == (n,)
    assert torch.equal(perm.sort().values, torch.arange(n))


def test_domain_covers_n_and_stays_below_4n():
    for n in [2, 3, 4, 5, 16, 17, 1797, 60000, 65536, 65537, 2**31 - 1]:
        d = 4 ** ref.shuffle_half_bits(n)
        assert n <= d < 4 * n, n
    assert ref.shuffle_half_bits(1) == 1          # the smallest network
    assert ref.shuffle_half_bits(2**31 - 1) == 16  # still 32-bit arithmetic


def test_permutation_is_keyed_by_seed_and_step_counter():
    n = 1797
    a = ref.shuffle_perm(n, 0, 0)
    for other in (ref.shuffle_perm(n, 0, 4), ref.shuffle_perm(n, 1, 0)):
        agree = float((a == other).float().mean())
        print(f"agreement {agree:.4%}")
        assert agree < 0.01
    assert torch.equal(a, ref.shuffle_perm(n, 0, 0))
    # seed and counter are taken mod 2**32, the counter as the int32's bits
    assert torch.equal(ref.shuffle_perm(n, 5, -1), ref.shuffle_perm(n, 5, 2**32 - 1))


def test_permutation_is_uniform_over_the_step_counter():
    """N = 8, t = 0..4095: every (element, position) count within
    512 +- 128, six binomial standard deviations sqrt(4096 / 8 * 7 / 8) = 21.2."""
    counts = torch.zeros(8, 8, dtype=torch.int64)
    pos = torch.arange(8)
    for t in range(4096):
        counts[ref.shuffle_perm(8, 0, t), pos] += 1
    print(f"counts {int(counts.min())}..{int(counts.max())}")
    assert int(counts.min()) >= 512 - 128 and int(counts.max()) <= 512 + 128


def test_permutation_refuses_an_empty_or_oversized_range():
    for n in (0, -1, 2**31):
        with pytest.raises(ValueError):
            ref.shuffle_perm(n, 0, 0)


def test_host_header_equals_the_reference():
    """tabular_shuffle.h as the host compiles it against the Python copy."""
    from unionml_amd.ops import hip_ext

    ext = hip_ext(required=False)
    if ext is None:
        pytest.skip("extension not built")
    for n in [1, 2, 3, 4, 5, 17, 63, 64, 65, 1797, 65536, 65537, 100003]:
        for seed, t in [(0, 0), (0, 1), (7, 999), (2**32 - 1, 2**31 - 1), (1, -1)]:
            got = ext.shuffle_perm_host(n, seed, t)
            assert torch.equal(got.long(), ref.shuffle_perm(n, seed, t)), (n, seed, t)


# ---------------------------------------------------------------------------
# train_epochs(shuffle=True)
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("regression,shape", MODELS, ids=MODEL_IDS)
def test_shuffled_epochs_equal_the_manual_loop(regression, shape):
    a, b = make_model(regression, shape), make_model(regression, shape)
    Xbf, y = make_data(a)
    make_data(b)
    a.train_epochs(Xbf, y, epochs=3, batch_size=BATCH, lr=3e-3, shuffle=True,
                   shuffle_seed=7)
    manual_epochs(b, Xbf, y, 3, 7, batch_size=BATCH, lr=3e-3)
    assert int(a.t_dev) == 9
    assert_same_state(a, b)
    # and the order matters: the unshuffled run ends elsewhere
    c = make_model(regression, shape)
    make_data(c)
    c.train_epochs(Xbf, y, epochs=3, batch_size=BATCH, lr=3e-3)
    assert not torch.equal(a.master, c.master)


@pytest.mark.parametrize("regression,shape", MODELS, ids=MODEL_IDS)
def test_resume_continues_the_sequence_of_orders(regression, shape):
    kw = dict(batch_size=BATCH, lr=3e-3, shuffle=True, shuffle_seed=11)
    whole = make_model(regression, shape)
    Xbf, y = make_data(whole)
    whole.train_epochs(Xbf, y, epochs=4, **kw)
    first = make_model(regression, shape)
    make_data(first)
    first.train_epochs(Xbf, y, epochs=2, **kw)
    second = make_model(regression, shape)
    second.load_state_dict(first.state_dict())
    second.train_epochs(Xbf, y, epochs=2, **kw)
    assert_same_state(whole, second)


def test_shuffle_off_equals_omitting_the_argument():
    a, b = make_model(False, (100, 50, 7)), make_model(False, (100, 50, 7))
    Xbf, y = make_data(a)
    make_data(b)
    a.train_epochs(Xbf, y, epochs=2, batch_size=BATCH)
    b.train_epochs(Xbf, y, epochs=2, batch_size=BATCH, shuffle=False, shuffle_seed=5)
    assert_same_state(a, b)
    assert a._shuf is None and b._shuf is None


def test_validation_rows_are_not_shuffled():
    a, b = make_model(False, (100, 50, 7)), make_model(False, (100, 50, 7))
    Xbf, y = make_data(a)
    make_data(b)
    val = (Xbf[:50].clone(), y[:50].clone())
    a.train_epochs(Xbf, y, epochs=3, batch_size=BATCH, shuffle=True, shuffle_seed=2,
                   validation=val)
    records = []
    manual_epochs(b, Xbf, y, 3, 2, batch_size=BATCH,
                  after_epoch=lambda: records.append(b._eval_record(*val)))
    assert torch.equal(a.val_history, torch.stack(records))


def test_shuffle_refusals():
    clf = make_model(False, (64, 32, 10))
    Xbf, y = make_data(clf, n=256)
    with pytest.raises(ValueError, match="persistent"):
        clf.train_epochs(Xbf, y, epochs=1, batch_size=128, shuffle=True,
                         engine="persistent")
    with pytest.raises(ValueError, match="world_size"):
        clf.train_epochs(Xbf, y, epochs=1, shuffle=True, world_size=2)
    for seed in (-1, 2**32):
        with pytest.raises(ValueError, match="shuffle_seed"):
            clf.train_epochs(Xbf, y, epochs=1, shuffle=True, shuffle_seed=seed)
    assert int(clf.t_dev) == 0
    reg = make_model(True, (20, 32, 1))
    Xr, Yr = make_data(reg, n=64)
    with pytest.raises(ValueError):
        reg.train_epochs(Xr, Yr, epochs=1, shuffle=True, engine="persistent")


def test_pickle_drops_the_shuffle_buffers():
    import pickle

    clf = make_model(False, (100, 50, 7))
    clf._shuf = (torch.zeros(1), torch.zeros(1))
    assert pickle.loads(pickle.dumps(clf))._shuf is None
