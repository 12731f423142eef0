"""CPU tests for the generalized tabular geometry: Geometry math,
parametric reference ops, and TabularMLP at non-digits shapes (the same
class that runs the gen HIP kernels on a GPU runs the parametric torch
reference here — one code path, two substrates)."""

import pickle

import pytest
import torch

from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import Geometry
from unionml_amd.ops.tabular import TabularMLP


def test_geometry_padding_math():
    g = Geometry(784, 128, 10)
    assert (g.inp, g.hid, g.cpad) == (800, 128, 16)
    assert g.off_b1 == 800 * 128
    assert g.nparam == 800 * 128 + 128 + 128 * 16 + 16
    assert not g.is_specialized

    g2 = Geometry(64, 32, 10)
    assert g2.is_specialized
    assert (g2.off_b1, g2.off_w2, g2.off_b2, g2.nparam) == (2048, 2080, 2592, 2608)

    g3 = Geometry(100, 50, 7)
    assert (g3.inp, g3.hid) == (128, 64)
    g4 = Geometry(33, 250, 3)
    assert (g4.inp, g4.hid) == (64, 256)


def test_geometry_rejects_unsupported():
    with pytest.raises(ValueError, match="classes"):
        Geometry(64, 32, 33)
    with pytest.raises(ValueError, match="hidden"):
        Geometry(64, 300, 10)
    with pytest.raises(ValueError):
        Geometry(0, 32, 10)


def test_geometry_wide_class_head():
    """17..32 classes use the two-tile classifier head (cpad 32)."""
    g = Geometry(64, 32, 26)
    assert g.cpad == 32
    assert g.off_b2 == g.off_w2 + 32 * 32
    assert g.nparam == 64 * 32 + 32 + 32 * 32 + 32
    assert Geometry(64, 32, 16).cpad == 16
    assert Geometry(64, 32, 17).cpad == 32


def test_parametric_matches_legacy_at_digits_shape():
    """mlp_step_g at the digits geometry must agree with the original
    hardcoded reference (the specialized-kernel oracle) closely — the
    only difference is one extra bf16 round of H before layer 2."""
    g = Geometry(64, 32, 10)
    torch.manual_seed(0)
    B = 128
    clf = TabularMLP(device="cpu", seed=3)
    Xbf = (torch.randn(B, 64) * 1.2).bfloat16()
    y = torch.randint(0, 10, (B,), dtype=torch.int32)

    grads_a = torch.zeros(g.nparam + 1)
    ref.mlp_step(Xbf, y, clf.W1bf, clf.W2bf, clf.master, grads_a, 1.0 / B)
    grads_b = torch.zeros(g.nparam + 1)
    ref.mlp_step_g(g, Xbf, y, clf.W1bf, clf.W2bf, clf.master, grads_b, 1.0 / B)

    scale = grads_a[: g.nparam].abs().max()
    err = (grads_a[: g.nparam] - grads_b[: g.nparam]).abs().max()
    assert err < max(2e-2 * float(scale), 2e-4)
    assert abs(grads_a[g.nparam] - grads_b[g.nparam]) < 2e-3


@pytest.mark.parametrize("shape", [(784, 128, 10), (100, 50, 7), (33, 250, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_cpu_train_predict_odd_shapes(shape):
    inf, hid, cls = shape
    clf = TabularMLP(in_features=inf, hidden=hid, classes=cls, device="cpu", seed=0)
    g = torch.Generator().manual_seed(1)
    n = 512
    centers = torch.randn(cls, inf, generator=g) * 3.0
    y = torch.randint(0, cls, (n,), generator=g, dtype=torch.int32)
    X = centers[y.long()] + torch.randn(n, inf, generator=g) * 0.5
    clf.fit_standardizer(X)
    Xbf = clf.stage(X)
    assert Xbf.shape == (n, clf.g.inp)
    if clf.g.inp > inf:
        assert (Xbf[:, inf:] == 0).all(), "staging must zero-pad"
    loss = clf.train_epochs(Xbf, y, epochs=8, batch_size=128, lr=5e-3)
    assert loss == loss  # not NaN
    preds = clf.predict(X)
    acc = (preds == y).float().mean().item()
    assert acc > 0.9, f"{shape}: accuracy {acc}, loss {loss}"
    # padded params stayed exactly zero through training
    W1, b1, W2, b2 = ref.unpack_master_g(clf.g, clf.master)
    assert (W1[inf:, :] == 0).all() and (W1[:, hid:] == 0).all()
    assert (W2[hid:, :] == 0).all() and (W2[:, cls:] == 0).all()
    assert (b1[hid:] == 0).all() and (b2[cls:] == 0).all()


def test_state_dict_roundtrip_and_geometry_guard():
    clf = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=0)
    X = torch.randn(64, 100)
    y = torch.randint(0, 7, (64,), dtype=torch.int32)
    clf.fit_standardizer(X)
    clf.train_epochs(clf.stage(X), y, epochs=2, batch_size=32, lr=1e-3)

    state = clf.state_dict()
    assert state["W1"].shape == (100, 50)
    assert state["W2"].shape == (50, 7)

    rebuilt = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=9)
    rebuilt.load_state_dict(state)
    assert torch.equal(clf.predict(X), rebuilt.predict(X))

    wrong = TabularMLP(in_features=64, hidden=32, classes=10, device="cpu")
    with pytest.raises(ValueError, match="geometry"):
        wrong.load_state_dict(state)


def test_pickle_roundtrip_gen_shape():
    clf = TabularMLP(in_features=200, hidden=96, classes=5, device="cpu", seed=0)
    X = torch.randn(32, 200)
    clf.fit_standardizer(X)
    blob = pickle.dumps(clf)
    clone = pickle.loads(blob)
    assert clone.g == clf.g
    assert torch.equal(clone.predict(X), clf.predict(X))


def test_legacy_pickle_without_geometry_loads():
    """Round-1 pickles predate the Geometry field; they must rehydrate
    as the digits shape."""
    clf = TabularMLP(device="cpu", seed=0)
    state = clf.__getstate__()
    state.pop("g")
    state.pop("use_spec")
    clone = TabularMLP.__new__(TabularMLP)
    clone.__setstate__(state)
    assert clone.g.is_specialized
    X = torch.randn(8, 64)
    assert clone.predict(X).shape == (8,)


@pytest.mark.parametrize("shape", [(64, 32, 26), (100, 60, 20)],
                         ids=lambda s: "x".join(map(str, s)))
def test_cpu_train_predict_wide_classes(shape):
    inf, hid, cls = shape
    clf = TabularMLP(in_features=inf, hidden=hid, classes=cls, device="cpu", seed=0)
    assert clf.g.cpad == 32
    g = torch.Generator().manual_seed(2)
    n = 512
    centers = torch.randn(cls, inf, generator=g) * 3.0
    y = torch.randint(0, cls, (n,), generator=g, dtype=torch.int32)
    X = centers[y.long()] + torch.randn(n, inf, generator=g) * 0.5
    clf.fit_standardizer(X)
    loss = clf.train_epochs(clf.stage(X), y, epochs=10, batch_size=128, lr=5e-3)
    assert loss == loss
    preds = clf.predict(X)
    acc = (preds == y).float().mean().item()
    assert acc > 0.9, f"{shape}: accuracy {acc}, loss {loss}"


def test_checkpoint_resumes_training_exactly():
    """Full checkpoints carry Adam state: 2+2 epochs through a
    state_dict roundtrip must be bit-identical to 4 straight epochs
    (same deterministic batch order, same moments, same step count)."""
    torch.manual_seed(11)
    X = torch.randn(128, 100) * 3
    y = torch.randint(0, 7, (128,), dtype=torch.int32)

    a = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=0)
    a.fit_standardizer(X)
    a.train_epochs(a.stage(X), y, epochs=4, batch_size=32, lr=1e-3)

    b = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=0)
    b.fit_standardizer(X)
    b.train_epochs(b.stage(X), y, epochs=2, batch_size=32, lr=1e-3)
    state = b.state_dict()

    c = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=99)
    c.load_state_dict(state)  # restores weights, standardizer, m/v/t
    c.train_epochs(c.stage(X), y, epochs=2, batch_size=32, lr=1e-3)

    assert int(c.t_dev.item()) == int(a.t_dev.item()) == 16
    assert torch.equal(a.master, c.master), (
        (a.master - c.master).abs().max()
    )


def test_weights_only_checkpoint_resets_optimizer():
    """Checkpoints from before optimizer-state support (no adam_* keys)
    still load — with fresh moments and t=0."""
    clf = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu", seed=0)
    X = torch.randn(64, 100)
    y = torch.randint(0, 7, (64,), dtype=torch.int32)
    clf.fit_standardizer(X)
    clf.train_epochs(clf.stage(X), y, epochs=2, batch_size=32, lr=1e-3)
    state = clf.state_dict()
    for k in ("adam_m", "adam_v", "adam_t"):
        state.pop(k)

    fresh = TabularMLP(in_features=100, hidden=50, classes=7, device="cpu")
    fresh.load_state_dict(state)
    assert int(fresh.t_dev.item()) == 0
    assert fresh.m.abs().max() == 0 and fresh.v.abs().max() == 0
    assert torch.equal(fresh.predict(X), clf.predict(X))


# ---------------------------------------------------------------------------
# the host layer's single sources: the instantiation table and the geometry
# ---------------------------------------------------------------------------


def test_python_table_equals_header():
    """reference.GEN_INSTANTIATIONS is the table macro of tabular_launch.h,
    row for row, and what is derived from it is what was written out before."""
    import re
    from pathlib import Path

    header = (Path(ref.__file__).parent / "hip" / "tabular_launch.h").read_text()
    macro = re.search(r"#define TABULAR_GEN_INSTANTIATIONS\(X\)((?:.*\\\n)+.*\n)", header)
    rows = [(int(h), int(r), int(c), p == "1") for h, r, c, p in
            re.findall(r"X\((\d+), (\d+), (\d+), ([01])\)", macro.group(1))]
    assert len(rows) == 11 and sum(p for _, _, _, p in rows) == 8
    assert list(ref.GEN_INSTANTIATIONS) == rows
    assert len(set(r[:3] for r in rows)) == 11
    assert ref.SUPPORTED_HID == (32, 64, 128, 256)
    # PREDICT marks exactly the largest RT of each (HID, CPAD)
    for h, r, c, p in rows:
        assert p == (r == ref.compiled_rts(h, c)[-1]), (h, r, c)


# {(inp, hid, cpad): (off_b1, off_w2, off_b2, nparam, image W2T offset, image
# size)} for every padded geometry tests/oracle64.py runs. tabular_launch.h
# holds its GenGeometry to the lines marked "header" in a static_assert, so
# the C++ and the Python formulas meet in those numbers.
HOST_GEOMETRY_LITERALS = {
    (32, 32, 16): (1024, 1056, 1568, 1584, 2048, 2560),   # header
    (32, 32, 32): (1024, 1056, 2080, 2112, 2048, 3072),   # header
    (64, 32, 16): (2048, 2080, 2592, 2608, 3072, 3584),
    (96, 64, 16): (6144, 6208, 7232, 7248, 8192, 9216),
    (128, 64, 16): (8192, 8256, 9280, 9296, 10240, 11264),
    (128, 64, 32): (8192, 8256, 10304, 10336, 10240, 12288),
    (160, 64, 16): (10240, 10304, 11328, 11344, 12288, 13312),
    (64, 128, 16): (8192, 8320, 10368, 10384, 12288, 14336),
    (96, 128, 16): (12288, 12416, 14464, 14480, 16384, 18432),
    (224, 128, 32): (28672, 28800, 32896, 32928, 32768, 36864),   # header
    (32, 256, 32): (8192, 8448, 16640, 16672, 16384, 24576),
    (64, 256, 16): (16384, 16640, 20736, 20752, 24576, 28672),
    (96, 256, 16): (24576, 24832, 28928, 28944, 32768, 36864),   # header
}


def test_geometry_matches_the_host_header():
    """Every geometry tests/oracle64.py runs gives, through
    reference.Geometry, the literal numbers above, four lines of which the
    header's GenGeometry is asserted to give at compile time."""
    import oracle64 as o64

    shapes = [s for _, s in o64.STEP_INSTANTIATIONS + o64.PRED_INSTANTIATIONS]
    shapes += [s for s, _ in o64.E2E_CASES] + [o64.SPEC_SHAPE]
    shapes += [s for _, s in o64.ADAM_KERNELS]
    seen = set()
    for shape in shapes:
        g = Geometry(*shape)
        seen.add((g.inp, g.hid, g.cpad))
        want = HOST_GEOMETRY_LITERALS[(g.inp, g.hid, g.cpad)]
        o2 = g.hid * g.inp + g.hid * 32
        assert (g.off_b1, g.off_w2, g.off_b2, g.nparam, o2, g.wimg_n) == want, shape
        assert g.off_w1 == 0 and g.slab_stride >= g.nparam + 2
    assert seen == set(HOST_GEOMETRY_LITERALS)


@pytest.mark.parametrize("hid,cpad,batch,want", [
    # (hid, cpad) -> the old per-width table {32: (128, 64), 64: (128, 64),
    # 128: (64, 32), 256: (32, 32)} = (big, small): small up to 128
    # workgroups of it, big beyond; cpad 32 always big
    (32, 16, 64 * 128, 64), (32, 16, 64 * 128 + 1, 128),
    (64, 16, 64 * 128, 64), (64, 16, 64 * 128 + 1, 128),
    (128, 16, 32 * 128, 32), (128, 16, 32 * 128 + 1, 64),
    (256, 16, 32 * 128, 32), (256, 16, 32 * 128 + 1, 32),
    (32, 32, 128 * 128, 128), (32, 32, 128 * 128 + 1, 128),
    (64, 32, 128 * 128, 128), (64, 32, 128 * 128 + 1, 128),
    (128, 32, 64 * 128, 64), (128, 32, 64 * 128 + 1, 64),
    (256, 32, 32 * 128, 32), (256, 32, 32 * 128 + 1, 32),
])
def test_rows_per_wg(hid, cpad, batch, want):
    """TabularMLP._rows_per_wg on both sides of the 128-workgroup threshold
    for every compiled (hid, cpad), both heads."""
    from unionml_amd.ops.tabular import TabularMLPRegressor

    clf = TabularMLP(20, hid - 3, 2 if cpad == 16 else 17, device="cpu")
    reg = TabularMLPRegressor(20, hid - 3, 1 if cpad == 16 else 17, device="cpu")
    for model in (clf, reg):
        assert (model.g.hid, model.g.cpad) == (hid, cpad)
        assert model._rows_per_wg(batch) == want
        assert model._rows_per_wg(1) == ref.compiled_rts(hid, cpad)[0]
        assert model._rows_per_wg() == ref.compiled_rts(hid, cpad)[-1]
    assert TabularMLP(device="cpu")._rows_per_wg(batch) == 128
