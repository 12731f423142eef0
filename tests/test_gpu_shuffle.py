"""Shuffled epochs on the GPU: the shuffle kernel evaluates the reference
permutation and gathers exactly; a shuffled training run, captured or
eager, is bit for bit the manual loop "gather on the host by the reference
permutation at the current step counter, train one plain epoch"; and the
binding refuses a broken precondition before anything is launched.

No case relies on a kernel reading out of bounds to be noticed: an
undersized argument is a leading slice of a full-sized allocation, a wrong
dtype a reinterpreting view of one."""

import pytest
import torch

from shuffle_fixtures import (
    BATCH, MODEL_IDS, MODELS, assert_same_state, make_data, make_model, manual_epochs,
)
from unionml_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV_STATE = ("master", "m", "v", "t_dev", "bfmirror")
POISON = 7.0


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev(ext):
    return torch.device("cuda:0")


def _sources(n, inp, target, dev, seed=0):
    """staged-looking rows: Xbf [n][inp] bf16 and labels or Yt [n][cpad]"""
    gen = torch.Generator().manual_seed(seed)
    Xbf = torch.randn(n, inp, generator=gen).bfloat16().to(dev)
    if target == "labels":
        y = torch.randint(0, 10, (n,), generator=gen, dtype=torch.int32).to(dev)
    else:
        y = torch.randn(n, target, generator=gen).to(dev)
    return Xbf, y


def _destinations(Xbf, y, extra=3):
    """poisoned destinations with ``extra`` rows more than the sources"""
    n = Xbf.shape[0] + extra
    Xs = torch.full((n, Xbf.shape[1]), POISON, dtype=Xbf.dtype, device=Xbf.device)
    ys = torch.full((n, *y.shape[1:]), int(POISON), dtype=y.dtype, device=y.device)
    return Xs, ys


def _shuffle(ext, Xbf, y, Xs, ys, t_dev, seed, perm_out=None, regression=None):
    if regression is None:
        regression = y.dtype != torch.int32
    fn = ext.shuffle_rows_reg if regression else ext.shuffle_rows
    fn(Xbf, y, Xs, ys, t_dev, seed, perm_out)


# ---------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1797, 65537])
def test_perm_out_is_the_reference_permutation(ext, dev, n):
    Xbf, y = _sources(n, 32, "labels", dev)
    Xs, ys = _destinations(Xbf, y, extra=0)
    for t in (0, 1, 999):
        t_dev = torch.tensor([t], dtype=torch.int32, device=dev)
        for seed in (0, 2**32 - 1):
            perm_out = torch.full((n,), -1, dtype=torch.int32, device=dev)
            _shuffle(ext, Xbf, y, Xs, ys, t_dev, seed, perm_out)
            want = ref.shuffle_perm(n, seed, t)
            assert torch.equal(perm_out.cpu().long(), want), (t, seed)
            assert torch.equal(perm_out.cpu(), ext.shuffle_perm_host(n, seed, t))
            assert int(t_dev) == t


@pytest.mark.parametrize("target", ["labels", 16, 32], ids=["labels", "Yt16", "Yt32"])
@pytest.mark.parametrize("inp", [32, 96, 800])
def test_gather_is_exact_and_stays_inside_its_rows(ext, dev, inp, target):
    for n in (1, 65, 1797):
        Xbf, y = _sources(n, inp, target, dev, seed=n)
        X0, y0 = Xbf.clone(), y.clone()
        Xs, ys = _destinations(Xbf, y)
        t_dev = torch.tensor([5], dtype=torch.int32, device=dev)
        _shuffle(ext, Xbf, y, Xs, ys, t_dev, 3)
        perm = ref.shuffle_perm(n, 3, 5).to(dev)
        assert torch.equal(Xs[:n], X0[perm]), n
        assert torch.equal(ys[:n], y0[perm]), n
        # the three extra rows keep their poison, the sources their values
        assert bool((Xs[n:] == POISON).all()) and bool((ys[n:] == int(POISON)).all())
        assert torch.equal(Xbf, X0) and torch.equal(y, y0)
        # without perm_out the same rows arrive
        Xs2, ys2 = _destinations(Xbf, y)
        perm_out = torch.empty(n, dtype=torch.int32, device=dev)
        _shuffle(ext, Xbf, y, Xs2, ys2, t_dev, 3, perm_out)
        assert torch.equal(Xs2, Xs) and torch.equal(ys2, ys)
        assert torch.equal(perm_out.long(), perm)


# ---------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------

TRAIN = dict(batch_size=BATCH, lr=3e-3)


@pytest.fixture(scope="module")
def manual_runs(ext, dev):
    """Per model: the staged data and the state after the manual loop of 3
    shuffled epochs (seed 7), computed once."""
    out = {}
    for (regression, shape), name in zip(MODELS, MODEL_IDS):
        model = make_model(regression, shape, dev)
        Xbf, y = make_data(model)
        manual_epochs(model, Xbf, y, 3, 7, use_graph=False, **TRAIN)
        torch.cuda.synchronize()
        out[name] = (Xbf, y, model)
    return out


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("regression,shape", MODELS, ids=MODEL_IDS)
def test_shuffled_training_equals_the_manual_loop(dev, manual_runs, regression, shape,
                                                  use_graph):
    """Fails without the feature, and with a permutation frozen at capture
    time: epochs 2 and 3 are replays, whose shuffle launch must read the
    step counter the replayed Adam kernels advanced."""
    name = MODEL_IDS[MODELS.index((regression, shape))]
    Xbf, y, want = manual_runs[name]
    model = make_model(regression, shape, dev)
    make_data(model)
    X0, y0 = Xbf.clone(), y.clone()
    model.train_epochs(Xbf, y, epochs=3, shuffle=True, shuffle_seed=7,
                       use_graph=use_graph, **TRAIN)
    assert int(model.t_dev) == 9
    assert_same_state(model, want, DEV_STATE)
    assert torch.equal(Xbf, X0) and torch.equal(y, y0)
    assert (model._graph is not None) == use_graph


def test_shuffled_training_differs_from_unshuffled(dev, manual_runs):
    Xbf, y, want = manual_runs["100x50x7"]
    model = make_model(False, (100, 50, 7), dev)
    make_data(model)
    model.train_epochs(Xbf, y, epochs=3, **TRAIN)
    assert not torch.equal(model.master, want.master)
    assert model._shuf is None


@pytest.mark.parametrize("regression,shape", MODELS, ids=MODEL_IDS)
def test_resume_on_the_device(dev, regression, shape):
    kw = dict(shuffle=True, shuffle_seed=11, **TRAIN)
    whole = make_model(regression, shape, dev)
    Xbf, y = make_data(whole)
    whole.train_epochs(Xbf, y, epochs=4, **kw)
    first = make_model(regression, shape, dev)
    make_data(first)
    first.train_epochs(Xbf, y, epochs=2, **kw)
    second = make_model(regression, shape, dev)
    second.load_state_dict(first.state_dict())
    second.train_epochs(Xbf, y, epochs=2, **kw)
    assert_same_state(whole, second, DEV_STATE)


@pytest.mark.parametrize("shape", [(64, 32, 10), (100, 50, 7)], ids=MODEL_IDS[:2])
def test_validation_under_shuffle(dev, shape):
    a, b = make_model(False, shape, dev), make_model(False, shape, dev)
    Xbf, y = make_data(a)
    make_data(b)
    val = (Xbf[:50].clone(), y[:50].clone())
    a.train_epochs(Xbf, y, epochs=3, shuffle=True, shuffle_seed=2, validation=val,
                   **TRAIN)
    records = []
    manual_epochs(b, Xbf, y, 3, 2, use_graph=False,
                  after_epoch=lambda: records.append(b.evaluate(*val)), **TRAIN)
    assert a.val_history.shape[0] == 3
    assert a.val_metrics() == records
    assert_same_state(a, b, DEV_STATE)


def test_reallocation_on_a_new_shape_drops_the_graph(dev):
    model = make_model(False, (100, 50, 7), dev)
    Xbf, y = make_data(model)
    model.train_epochs(Xbf, y, epochs=2, shuffle=True, **TRAIN)
    assert model._graph is not None
    bufs = model._shuf
    model.train_epochs(Xbf, y, epochs=2, shuffle=True, **TRAIN)
    assert model._shuf is bufs                       # same shape: kept
    model._ensure_shuffle(Xbf[:200], y[:200])
    assert model._shuf is not bufs and model._shuf[0].shape[0] == 200
    assert model._graph is None and model._graph_key is None


# ---------------------------------------------------------------------------
# the argument contract
# ---------------------------------------------------------------------------

OTHER_DTYPE = {torch.float32: torch.int32, torch.int32: torch.float32,
               torch.bfloat16: torch.float16}
ARGS = ("Xbf", "y", "Xs", "ys", "t_dev", "seed", "perm_out")


def retype(t):
    return t.view(OTHER_DTYPE[t.dtype])


def on_cpu(t):
    return t.cpu()


def strided(t):
    """every second row of a buffer twice the size: not contiguous"""
    out = torch.zeros((2 * t.shape[0], *t.shape[1:]), dtype=t.dtype, device=t.device)[::2]
    out.copy_(t)
    assert not out.is_contiguous()
    return out


def unaligned(t):
    """the same values one element past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = buf[1 : 1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def rows(n):
    return lambda t: t[:n]


def value(v):
    return lambda _: v


def _valid_args(dev, regression):
    """the smallest interesting valid call: 5 rows of 64 features. Sources
    and destinations are slices of two allocations, so that an overlapping
    argument is another slice of the same one."""
    Xbf, y = _sources(5, 64, 16 if regression else "labels", dev)
    xpool = torch.full((16, 64), POISON, dtype=torch.bfloat16, device=dev)
    ypool = torch.full((16, *y.shape[1:]), int(POISON), dtype=y.dtype, device=dev)
    xpool[:5].copy_(Xbf)
    ypool[:5].copy_(y)
    return dict(
        Xbf=xpool[:5], y=ypool[:5], Xs=xpool[8:14], ys=ypool[8:14],
        t_dev=torch.tensor([4], dtype=torch.int32, device=dev), seed=9,
        perm_out=torch.full((5,), -1, dtype=torch.int32, device=dev),
    ), dict(xpool=xpool, ypool=ypool)


def _violations(regression):
    tensors = ("Xbf", "y", "Xs", "ys", "t_dev", "perm_out")
    out = []
    for n in tensors:
        out += [(f"{n}-dtype", {n: retype}), (f"{n}-cpu", {n: on_cpu})]
    for n in ("Xbf", "y", "Xs", "ys", "perm_out"):
        out.append((f"{n}-strided", {n: strided}))
    out += [
        ("N-0", {"Xbf": rows(0), "y": rows(0)}),
        ("y-short", {"y": rows(4)}),
        ("Xs-short", {"Xs": rows(4)}), ("ys-short", {"ys": rows(4)}),
        ("perm_out-short", {"perm_out": rows(4)}), ("t_dev-empty", {"t_dev": rows(0)}),
        ("Xs-width", {"Xs": lambda t: t.reshape(-1)[: 6 * 32].view(6, 32)}),
        ("inp-not-multiple-of-32", {
            "Xbf": lambda t: t.reshape(-1)[: 5 * 48].view(5, 48),
            "Xs": lambda t: t.reshape(-1)[: 6 * 48].view(6, 48)}),
        ("Xbf-unaligned", {"Xbf": unaligned}), ("Xs-unaligned", {"Xs": unaligned}),
        ("seed-negative", {"seed": value(-1)}), ("seed-2^32", {"seed": value(2**32)}),
        # equal storage, and a destination that starts inside its source
        ("Xs-is-Xbf", {"Xs": "pool:xpool:0:6"}), ("Xs-overlaps-Xbf", {"Xs": "pool:xpool:4:10"}),
        ("ys-is-y", {"ys": "pool:ypool:0:6"}), ("ys-overlaps-y", {"ys": "pool:ypool:4:10"}),
        ("perm_out-is-t_dev-storage", {"t_dev": "perm_out"}),
    ]
    if regression:
        out += [("Yt-unaligned", {"y": unaligned}), ("Yts-unaligned", {"ys": unaligned}),
                ("Yt-columns", {"y": lambda t: t.reshape(-1)[: 5 * 8].view(5, 8),
                                "ys": lambda t: t.reshape(-1)[: 6 * 8].view(6, 8)}),
                ("Yts-columns", {"ys": lambda t: t.reshape(-1)[: 3 * 32].view(3, 32)}),
                ("Yt-1d", {"y": lambda t: t.reshape(-1)})]
    return out


CASES = [(reg, label, change) for reg in (False, True)
         for label, change in _violations(reg)]
CASE_IDS = [f"{'reg' if reg else 'clf'}-{label}" for reg, label, _ in CASES]

_built = {}


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).clone()


def _valid(dev, regression):
    if regression not in _built:
        args, pools = _valid_args(dev, regression)
        torch.cuda.synchronize()
        _built[regression] = (args, pools)
    return _built[regression]


@pytest.mark.parametrize("regression", [False, True], ids=["clf", "reg"])
def test_smallest_valid_call(ext, dev, regression):
    args, pools = _valid_args(dev, regression)
    _shuffle(ext, *[args[n] for n in ARGS], regression=regression)
    torch.cuda.synchronize()
    perm = ref.shuffle_perm(5, 9, 4).to(dev)
    assert torch.equal(args["perm_out"].long(), perm)
    assert torch.equal(args["Xs"][:5], args["Xbf"][perm])
    assert torch.equal(args["ys"][:5], args["y"][perm])
    # row 5 of the destinations and the rest of the pools keep their poison
    for pool in pools.values():
        assert bool((pool[5:8] == POISON).all()) and bool((pool[13:] == POISON).all())


@pytest.mark.parametrize("regression,label,change", CASES, ids=CASE_IDS)
def test_violation_raises_before_any_launch(ext, dev, regression, label, change):
    """One precondition broken, everything else valid: the binding raises,
    and no buffer has changed."""
    args, pools = _valid(dev, regression)
    watched = dict(args, **pools)
    before = {n: _bits(t) for n, t in watched.items() if torch.is_tensor(t)}
    broken = dict(args)
    for n, fn in change.items():
        if isinstance(fn, str) and fn.startswith("pool:"):
            _, pool, lo, hi = fn.split(":")
            broken[n] = pools[pool][int(lo) : int(hi)]
        elif isinstance(fn, str):
            # t_dev as the first element of another argument's storage
            broken[n] = args[fn][:1]
        else:
            broken[n] = fn(args[n])
    with pytest.raises(RuntimeError):
        _shuffle(ext, *[broken[n] for n in ARGS], regression=regression)
    torch.cuda.synchronize()
    for n, b in before.items():
        assert torch.equal(b, _bits(watched[n])), f"{n} changed"
