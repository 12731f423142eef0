"""The host layer of the tabular kernels on the GPU: the dispatchers reach
the instantiation the table names, and every binding refuses a call that
breaks one of its preconditions before anything is launched.

No case relies on a kernel reading out of bounds to be noticed: an
undersized argument is a leading slice of a full-sized allocation, a wrong
dtype a reinterpreting view of one, so a check that went missing would
still touch allocated memory only."""

import pytest
import torch

from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import NPARAM, Geometry

pytestmark = pytest.mark.gpu

NAN = float("nan")
ADAM = (1e-3, 0.9, 0.999, 1e-8)


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _model(dev, shape, regression):
    from unionml_amd.ops.tabular import TabularMLP, TabularMLPRegressor

    cls = TabularMLPRegressor if regression else TabularMLP
    model = cls(*shape, device=dev, seed=1)
    # non-zero biases, so a predict that ran shows in every output
    model.master[model.g.off_b1 : model.g.off_b1 + model.g.hidden] = 0.25
    model.bfmirror.copy_(model.master.bfloat16())
    model._build_wimg()
    return model


def _features(B, width, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, width, generator=gen)


# ---------------------------------------------------------------------------
# dispatch reaches the named kernel
# ---------------------------------------------------------------------------

STEP_ROWS = [(h, r, c) for h, r, c, _ in ref.GEN_INSTANTIATIONS]
PRED_ROWS = [(h, r, c) for h, r, c, p in ref.GEN_INSTANTIATIONS if p]
HEADS = [False, True]


def _row_id(v):
    if isinstance(v, tuple):
        return "h%d-rt%d-c%d" % v
    return "reg" if v else "clf"


def _row_shape(row, regression):
    """20 x (HID - 3) x 2 or 17 (regression: 1 or 17 targets)"""
    hid, _, cpad = row
    small = 1 if regression else 2
    return (20, hid - 3, small if cpad == 16 else 17)


@pytest.mark.parametrize("regression", HEADS, ids=_row_id)
@pytest.mark.parametrize("row", STEP_ROWS, ids=_row_id)
def test_step_dispatch_reaches_the_row(ext, dev, row, regression):
    """B = RT + 1 at rt=RT is two workgroups: slab rows 0 and 1 are written
    on [0, nparam], row 2 stays NaN. A dispatcher that picked another RT
    writes a different number of rows."""
    hid, rt, cpad = row
    model = _model(dev, _row_shape(row, regression), regression)
    g = model.g
    assert (g.hid, g.cpad) == (hid, cpad)
    B = rt + 1
    Xbf = torch.zeros(B, g.inp, dtype=torch.bfloat16)
    Xbf[:, : g.in_features] = _features(B, g.in_features).bfloat16()
    slabs = torch.full((3, g.slab_stride), NAN, device=dev)
    if regression:
        Yt = torch.zeros(B, g.cpad)
        Yt[:, : g.classes] = _features(B, g.classes, seed=1)
        ok = ext.mlp_step_reg_gen(Xbf.to(dev), Yt.to(dev), g.hid, g.classes, rt,
                                  model.wimg, model.master, slabs, 1.0 / B)
    else:
        y = (torch.arange(B) % g.classes).int()
        ok = ext.mlp_step_gen(Xbf.to(dev), y.to(dev), g.hid, g.classes, rt,
                              model.wimg, model.master, slabs, 1.0 / B)
    torch.cuda.synchronize()
    assert ok
    slabs = slabs.cpu()
    assert torch.isfinite(slabs[:2, : g.nparam + 1]).all()
    assert torch.isnan(slabs[2]).all()


@pytest.mark.parametrize("regression", HEADS, ids=_row_id)
@pytest.mark.parametrize("row", PRED_ROWS, ids=_row_id)
def test_predict_dispatch_reaches_the_row(ext, dev, row, regression):
    """B = RT + 1 rows into sentinel-filled outputs one row too long: rows
    < B are written, the extra row is untouched."""
    hid, rt, cpad = row
    model = _model(dev, _row_shape(row, regression), regression)
    g = model.g
    assert (g.hid, g.cpad) == (hid, cpad)
    B = rt + 1
    X = _features(B, g.in_features).to(dev)
    if regression:
        out = torch.full((B + 1, g.classes), NAN, device=dev)
        ext.mlp_predict_reg_gen(X, g.inp, g.hid, g.classes, model.mean, model.invstd,
                                model.wimg, model.master, model.y_mean, model.y_scale, out)
        torch.cuda.synchronize()
        assert torch.isfinite(out[:B]).all() and torch.isnan(out[B]).all()
        return
    preds = torch.full((B + 1,), -7, dtype=torch.int32, device=dev)
    probs = torch.full((B + 1, g.classes), NAN, device=dev)
    ext.mlp_predict_gen(X, g.inp, g.hid, g.classes, model.mean, model.invstd,
                        model.wimg, model.master, preds, probs)
    torch.cuda.synchronize()
    assert ((preds[:B] >= 0) & (preds[:B] < g.classes)).all() and int(preds[B]) == -7
    assert torch.allclose(probs[:B].sum(dim=1), torch.ones(B, device=dev), atol=1e-5)
    assert torch.isnan(probs[B]).all()


# ---------------------------------------------------------------------------
# the argument contract
# ---------------------------------------------------------------------------

OTHER_DTYPE = {torch.float32: torch.int32, torch.int32: torch.float32,
               torch.bfloat16: torch.float16, torch.uint32: torch.int32}


def short(n=None):
    """the leading n elements (default: all but one), flat"""
    return lambda t: t.reshape(-1)[: t.numel() - 1 if n is None else n]


def retype(t):
    return t.view(OTHER_DTYPE[t.dtype])


def flat(t):
    return t.reshape(-1)


def empty_rows(t):
    return t[:0]


def reshaped(*shape):
    return lambda t: t.reshape(-1)[: int(torch.tensor(shape).prod())].view(*shape)


def unaligned(t):
    """the same values one element past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=t.device)
    out = buf[1 : 1 + t.numel()].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def on_cpu(t):
    return t.cpu()


def strided(t):
    """every second element of a buffer twice the size: not contiguous"""
    out = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)[::2]
    out.copy_(t.reshape(-1))
    assert not out.is_contiguous()
    return out


def value(v):
    return lambda _: v


def doubled(t):
    """zeros of twice the size: large enough for cpad 32 where the valid
    call has cpad 16"""
    return torch.zeros((*t.shape[:-1], 2 * t.shape[-1]), dtype=t.dtype, device=t.device)


def columns(n):
    """a fresh [rows][n] matrix (rows kept) or [n] vector of zeros"""
    return lambda t: torch.zeros((*t.shape[:-1], n), dtype=t.dtype, device=t.device)


def digits_args(dev, ext, names):
    clf = _model(dev, (64, 32, 10), False)
    pool = dict(
        X=(_features(2, 64) * 4).to(dev), x=_features(2, 64).to(dev),
        Xbf=_features(2, 64).bfloat16().to(dev),
        y=torch.tensor([3, 9], dtype=torch.int32, device=dev),
        W1bf=clf.W1bf, W2bf=clf.W2bf, master=clf.master, bfmirror=clf.bfmirror,
        m=clf.m, v=clf.v, t_dev=clf.t_dev, mean=clf.mean, invstd=clf.invstd,
        grads=torch.full((NPARAM + 1,), 7.0, device=dev),
        slabs=torch.zeros(1, ext.SLAB, device=dev),
        counter=torch.zeros(1, dtype=torch.uint32, device=dev),
        loss_out=torch.full((1,), 7.0, device=dev),
        grads_out=torch.full((NPARAM + 1,), 7.0, device=dev),
        wimg=clf.wimg,
        preds=torch.full((2,), -7, dtype=torch.int32, device=dev),
        probs=torch.full((2, 10), 7.0, device=dev),
        out=torch.full((2, 64), 7.0, device=dev).bfloat16(),
        invBtot=0.5, eps=1e-5, batch=2, n_steps=1,
        lr=ADAM[0], beta1=ADAM[1], beta2=ADAM[2], adam_eps=ADAM[3],
    )
    return {n: pool[n] for n in names}


def gen_args(dev, ext, names, regression=False):
    model = _model(dev, (20, 32, 1 if regression else 2), regression)
    g = model.g
    Xbf = torch.zeros(2, g.inp, dtype=torch.bfloat16)
    Xbf[:, :20] = _features(2, 20).bfloat16()
    Yt = torch.zeros(2, g.cpad)
    Yt[:, :1] = _features(2, 1, seed=1)
    pool = dict(
        X=_features(2, 20).to(dev), Xbf=Xbf.to(dev), Yt=Yt.to(dev),
        y=torch.tensor([0, 1], dtype=torch.int32, device=dev),
        inp=g.inp, hid=g.hid, cls=g.classes, targets=g.classes, cpad=g.cpad, rt=128,
        n_wg=1, wimg=model.wimg, master=model.master, bfmirror=model.bfmirror,
        m=model.m, v=model.v, t_dev=model.t_dev, mean=model.mean, invstd=model.invstd,
        grads=torch.full((g.nparam + 1,), 0.5, device=dev),
        slabs=torch.full((1, g.slab_stride), NAN, device=dev),
        # one row of a two-row allocation: n_wg = 2 stays inside it
        red_slabs=torch.full((2, g.slab_stride), 0.5, device=dev)[:1],
        counter=torch.zeros(1, dtype=torch.uint32, device=dev),
        loss_out=torch.full((1,), 7.0, device=dev),
        grads_out=torch.full((g.nparam + 1,), 7.0, device=dev),
        preds=torch.full((2,), -7, dtype=torch.int32, device=dev),
        probs=torch.full((2, g.classes), 7.0, device=dev),
        out=torch.full((2, g.classes), 7.0, device=dev),
        invBtot=0.5,
        lr=ADAM[0], beta1=ADAM[1], beta2=ADAM[2], adam_eps=ADAM[3],
    )
    if regression:
        pool.update(y_mean=model.y_mean, y_scale=model.y_scale)
    return {n: pool[n] for n in names}


def reg_args(dev, ext, names):
    return gen_args(dev, ext, names, regression=True)


ADAM_TAIL = ("lr", "beta1", "beta2", "adam_eps")
STATE = ("master", "bfmirror", "m", "v", "t_dev")

# binding -> (builder, argument names in call order). Each builder's values
# are the smallest valid call: B = 2 at 64x32x10, 20x32x2 or 20x32x1.
BINDINGS = {
    "standardize_fit": (digits_args, ("X", "mean", "invstd", "eps")),
    "standardize_apply": (digits_args, ("X", "mean", "invstd", "out")),
    "mlp_step": (digits_args, ("Xbf", "y", "W1bf", "W2bf", "master", "grads", "invBtot")),
    "mlp_step_fused": (digits_args, ("Xbf", "y", "W1bf", "W2bf") + STATE + (
        "slabs", "counter", "loss_out", "invBtot") + ADAM_TAIL + ("grads_out", "wimg")),
    "mlp_train_steps": (digits_args, ("Xbf", "y", "batch", "n_steps") + STATE + (
        "loss_out",) + ADAM_TAIL),
    "mlp_predict": (digits_args, ("X", "mean", "invstd", "W1bf", "W2bf", "master",
                                  "preds", "probs")),
    "adam_step": (digits_args, ("master", "bfmirror", "grads", "m", "v", "t_dev")
                  + ADAM_TAIL + ("wimg",)),
    "reduce_selftest": (digits_args, ("x",)),
    "mlp_step_gen": (gen_args, ("Xbf", "y", "hid", "cls", "rt", "wimg", "master",
                                "slabs", "invBtot")),
    "reduce_adam_gen": (gen_args, ("red_slabs", "n_wg", "inp", "hid", "cpad") + STATE + (
        "counter", "loss_out") + ADAM_TAIL + ("wimg", "grads_out")),
    "mlp_predict_gen": (gen_args, ("X", "inp", "hid", "cls", "mean", "invstd", "wimg",
                                   "master", "preds", "probs")),
    "adam_step_gen": (gen_args, ("master", "bfmirror", "grads", "m", "v", "t_dev",
                                 "inp", "hid", "cpad") + ADAM_TAIL + ("wimg",)),
    "mlp_step_reg_gen": (reg_args, ("Xbf", "Yt", "hid", "targets", "rt", "wimg",
                                    "master", "slabs", "invBtot")),
    "mlp_predict_reg_gen": (reg_args, ("X", "inp", "hid", "targets", "mean", "invstd",
                                       "wimg", "master", "y_mean", "y_scale", "out")),
}


def _tensor_checks(names, skip=()):
    """undersized and retyped, for each named tensor argument"""
    out = []
    for n in names:
        if n not in skip:
            out += [(f"{n}-short", {n: short()}), (f"{n}-dtype", {n: retype})]
    return out


def _digits_batch_checks():
    return [("Xbf-1d", {"Xbf": flat}), ("Xbf-width", {"Xbf": reshaped(2, 32)}),
            ("Xbf-unaligned", {"Xbf": unaligned}), ("Xbf-dtype", {"Xbf": retype}),
            ("B-0", {"Xbf": empty_rows, "y": empty_rows}),
            ("y-short", {"y": short()}), ("y-dtype", {"y": retype})]


def _scaler_checks():
    return _tensor_checks(("mean", "invstd")) + [
        ("mean-cpu", {"mean": on_cpu}), ("invstd-cpu", {"invstd": on_cpu}),
        ("mean-strided", {"mean": strided}), ("invstd-strided", {"invstd": strided})]


def _raw_x_checks(empty_with=()):
    return [("X-1d", {"X": flat}), ("X-dtype", {"X": retype}),
            ("B-0", dict({"X": empty_rows}, **{n: empty_rows for n in empty_with}))]


def _gen_step_checks(n_out, with_33):
    """with_33: what else must grow so that only n_out = 33 is wrong"""
    big = dict({n_out: value(33), "wimg": doubled, "master": doubled, "slabs": doubled},
               **with_33)
    return [("Xbf-1d", {"Xbf": flat}), ("Xbf-dtype", {"Xbf": retype}),
            ("Xbf-unaligned", {"Xbf": unaligned}),
            ("inp-not-multiple-of-32", {"Xbf": reshaped(2, 16)}),
            (f"{n_out}-0", {n_out: value(0)}), (f"{n_out}-33", big),
            ("rt-0", {"rt": value(0)}), ("rt-not-compiled", {"rt": value(96)}),
            ("hid-not-compiled", {"hid": value(16)}),
            ("wimg-unaligned", {"wimg": unaligned}), ("slabs-1d", {"slabs": flat}),
            ("slabs-stride", {"slabs": reshaped(1, Geometry(20, 32, 2).nparam + 1)}),
            ("slabs-dtype", {"slabs": retype}),
            ] + _tensor_checks(("wimg", "master"))


def _gen_predict_checks(n_out, with_0, with_33):
    """with_0 / with_33: the outputs resized so that only n_out is wrong"""
    zero = dict({n_out: value(0)}, **with_0)
    big = dict({n_out: value(33), "wimg": doubled, "master": doubled}, **with_33)
    wide = {"X": lambda t: _features(2, 40).to(t.device),
            "mean": lambda t: torch.zeros(40, device=t.device),
            "invstd": lambda t: torch.ones(40, device=t.device)}
    return _scaler_checks() + [
        ("X-wider-than-inp", wide), ("inp-not-multiple-of-32", {"inp": value(24)}),
        (f"{n_out}-0", zero), (f"{n_out}-33", big),
        ("hid-not-compiled", {"hid": value(16)}),
    ] + _tensor_checks(("wimg", "master"))


VIOLATIONS = {
    "standardize_fit": _raw_x_checks() + _scaler_checks(),
    "standardize_apply": _raw_x_checks(("out",)) + _scaler_checks() + [
        ("out-dtype", {"out": retype}), ("out-rows", {"out": reshaped(1, 64)}),
        ("out-narrow", {"out": reshaped(2, 63)})],
    "mlp_step": _digits_batch_checks() + _tensor_checks(("W1bf", "W2bf", "master")) + [
        ("grads-short", {"grads": short(NPARAM)}), ("grads-dtype", {"grads": retype})],
    "mlp_step_fused": _digits_batch_checks() + _tensor_checks(
        ("W1bf", "W2bf", "bfmirror", "m", "v", "wimg")) + [
        # master is checked for the kernel's reads and as Adam state alike
        ("master-short", {"master": short()}), ("master-dtype", {"master": retype}),
        ("t_dev-empty", {"t_dev": short(0)}), ("t_dev-dtype", {"t_dev": retype}),
        ("slabs-1d", {"slabs": flat}), ("slabs-stride", {"slabs": reshaped(2, 1312)}),
        ("slabs-dtype", {"slabs": retype}),
        ("counter-empty", {"counter": short(0)}), ("counter-dtype", {"counter": retype}),
        ("loss_out-empty", {"loss_out": short(0)}), ("loss_out-dtype", {"loss_out": retype}),
        ("grads_out-short", {"grads_out": short(NPARAM)}),
        ("grads_out-dtype", {"grads_out": retype}), ("wimg-unaligned", {"wimg": unaligned})],
    "mlp_train_steps": _digits_batch_checks() + _tensor_checks(
        ("master", "bfmirror", "m", "v")) + [
        # both guards in front of the launcher's N % batch were read: the
        # binding's batch >= 1 check, and the launcher's own B < 1 return
        ("batch-0", {"batch": value(0)}), ("batch-negative", {"batch": value(-2)}),
        ("n_steps-negative", {"n_steps": value(-1)}),
        ("t_dev-empty", {"t_dev": short(0)}), ("loss_out-empty", {"loss_out": short(0)}),
        ("loss_out-dtype", {"loss_out": retype})],
    "mlp_predict": _raw_x_checks() + [("X-width", {"X": reshaped(2, 32)})]
    + _scaler_checks() + _tensor_checks(("W1bf", "W2bf", "master", "preds")) + [
        ("probs-rows", {"probs": reshaped(1, 10)}), ("probs-columns", {"probs": reshaped(4, 5)}),
        ("probs-dtype", {"probs": retype})],
    "adam_step": _tensor_checks(("master", "bfmirror", "m", "v", "wimg")) + [
        ("grads-short", {"grads": short(NPARAM - 1)}), ("grads-dtype", {"grads": retype}),
        ("t_dev-empty", {"t_dev": short(0)})],
    "reduce_selftest": [("x-1d", {"x": flat}), ("x-dtype", {"x": retype}),
                        ("x-width", {"x": reshaped(2, 32)}), ("B-0", {"x": empty_rows})],
    "mlp_step_gen": _gen_step_checks("cls", {}) + [
        ("B-0", {"Xbf": empty_rows, "y": empty_rows}),
        ("y-short", {"y": short()}), ("y-dtype", {"y": retype})],
    "reduce_adam_gen": _tensor_checks(("master", "bfmirror", "m", "v", "wimg")) + [
        ("slabs-1d", {"red_slabs": flat}), ("slabs-dtype", {"red_slabs": retype}),
        ("slabs-stride", {"red_slabs": reshaped(1, Geometry(20, 32, 2).nparam + 1)}),
        ("n_wg-0", {"n_wg": value(0)}), ("n_wg-past-the-rows", {"n_wg": value(2)}),
        ("cpad-24", {"cpad": value(24)}), ("inp-not-multiple-of-32", {"inp": value(16)}),
        ("counter-empty", {"counter": short(0)}), ("loss_out-empty", {"loss_out": short(0)}),
        ("t_dev-empty", {"t_dev": short(0)}),
        ("grads_out-short", {"grads_out": short(Geometry(20, 32, 2).nparam)})],
    "mlp_predict_gen": _raw_x_checks() + _gen_predict_checks(
        "cls", {"probs": columns(0)}, {"probs": columns(33)})
    + _tensor_checks(("preds",)) + [
        ("probs-rows", {"probs": reshaped(1, 2)}), ("probs-columns", {"probs": reshaped(4, 1)}),
        ("probs-dtype", {"probs": retype})],
    "adam_step_gen": _tensor_checks(("master", "bfmirror", "m", "v", "wimg")) + [
        ("grads-short", {"grads": short(Geometry(20, 32, 2).nparam - 1)}),
        ("grads-dtype", {"grads": retype}), ("cpad-24", {"cpad": value(24)}),
        ("t_dev-empty", {"t_dev": short(0)})],
    "mlp_step_reg_gen": _gen_step_checks("targets", {"Yt": doubled}) + [
        ("B-0", {"Xbf": empty_rows, "Yt": empty_rows}),
        ("Yt-rows", {"Yt": reshaped(1, 16)}), ("Yt-columns", {"Yt": reshaped(2, 8)}),
        ("Yt-1d", {"Yt": flat}), ("Yt-dtype", {"Yt": retype}),
        ("Yt-unaligned", {"Yt": unaligned})],
    "mlp_predict_reg_gen": _raw_x_checks() + _gen_predict_checks(
        "targets", {"y_mean": columns(0), "y_scale": columns(0)},
        {"y_mean": columns(33), "y_scale": columns(33), "out": columns(33)})
    + _tensor_checks(("y_mean", "y_scale"), skip=()) + [
        ("out-rows", {"out": reshaped(1, 1)}), ("out-columns", {"out": lambda t: t[:, :0]}),
        ("out-1d", {"out": flat}), ("out-dtype", {"out": retype})],
}

CASES = [(b, label, change) for b, checks in VIOLATIONS.items() for label, change in checks]


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.uint8).clone()


_built = {}


def _valid(binding, dev, ext):
    """the binding's valid arguments, built once, with their bit patterns"""
    if binding not in _built:
        builder, names = BINDINGS[binding]
        args = builder(dev, ext, names)
        torch.cuda.synchronize()
        _built[binding] = (args, {n: _bits(t) for n, t in args.items() if torch.is_tensor(t)})
    return _built[binding]


@pytest.mark.parametrize("binding", list(BINDINGS))
def test_smallest_valid_call(ext, dev, binding):
    """The call every violation below departs from is accepted and writes
    its outputs."""
    builder, names = BINDINGS[binding]
    args = builder(dev, ext, names)
    before = {n: _bits(t) for n, t in args.items() if torch.is_tensor(t)}
    ret = getattr(ext, binding)(*args.values())
    torch.cuda.synchronize()
    if binding == "mlp_train_steps":
        # a batch that is no multiple of 128 rows: declined without a launch
        assert ret is False
        return
    if binding == "reduce_selftest":
        assert ret.shape == (2, 64, 2) and torch.isfinite(ret).all()
        return
    assert ret is None or ret is True
    changed = [n for n, b in before.items() if not torch.equal(b, _bits(args[n]))]
    assert changed, "the valid call wrote nothing"
    for n in changed:
        t = args[n]
        if n == "slabs":   # a slab row is written on [0, nparam]; the rest is tag and pad
            t = t[:, : (NPARAM if builder is digits_args else Geometry(20, 32, 2).nparam) + 1]
        if t.is_floating_point():
            assert torch.isfinite(t.float()).all(), n


@pytest.mark.parametrize("binding,label,change", CASES,
                         ids=[f"{b}-{label}" for b, label, _ in CASES])
def test_violation_raises_before_any_launch(ext, dev, binding, label, change):
    """One precondition broken, everything else valid: the binding raises,
    and no argument's memory has changed."""
    args, before = _valid(binding, dev, ext)
    broken = dict(args)
    for n, fn in change.items():
        broken[n] = fn(args[n])
    with pytest.raises(RuntimeError):
        getattr(ext, binding)(*broken.values())
    torch.cuda.synchronize()
    for n, b in before.items():
        assert torch.equal(b, _bits(args[n])), f"{n} changed"


@pytest.mark.parametrize("shape", [(64, 32, 10), (20, 32, 2)], ids=["digits", "gen"])
def test_empty_batch_launches_nothing(ext, dev, shape):
    """The bindings take B >= 1; an empty batch is answered in Python with
    empty outputs, and leaves no launch error behind for the next call."""
    clf = _model(dev, shape, False)
    X = torch.zeros(0, shape[0])
    assert clf.stage(X).shape == (0, clf.g.inp)
    preds, probs = clf.predict(X, return_probs=True)
    assert preds.shape == (0,) and preds.dtype == torch.int32
    assert probs.shape == (0, shape[2])
    assert clf.predict(X).shape == (0,)
    torch.cuda.synchronize()
    assert clf.predict(_features(3, shape[0])).shape == (3,)
    torch.cuda.synchronize()
