"""CPU checks of the order-probe inputs (tests/order_probe.py), so that the
GPU test built on them (tests/test_gpu_gen_order.py) cannot hide behind a
bad probe: (a) nothing rounds before the sums under test, (b) the sums tell
the documented order from every order that is not provably equal to it,
(c) the rest of the step is exactly known on these inputs too."""

import numpy as np
import pytest
import torch

import oracle64 as o64
import oracle64_reg as o64r
import order_probe as op
from oracle64 import F64

CASES = op.cases()
IDS = [c[0] for c in CASES]


def _exact_in(t: torch.Tensor, dtype) -> bool:
    return torch.equal(t.to(dtype).to(F64), t.to(F64))


def test_case_list_covers_every_regression_instantiation():
    insts = op.instantiations()
    assert len(insts) == 11 and len(set(insts)) == 11
    # eight sum over 4 or 8 tiles; three over 2, which no probe can order
    assert sorted(i[1] for i in insts) == [32] * 3 + [64] * 4 + [128] * 4
    for inst in insts:
        want = (inst[1],) if inst[1] == 32 else (inst[1], inst[1] + 17)
        assert tuple(B for _, i, B in CASES if i == inst) == want
        o64r.check_instantiation(inst, op.probe_shape(inst))


# ---------------------------------------------------------------------------
# (a) exactness
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["bias", "loss"])
@pytest.mark.parametrize("cid,inst,B", CASES, ids=IDS)
def test_nothing_rounds_before_the_sums(cid, inst, B, kind):
    """The fp64 oracle's per-tile partials are the designed ones and are
    fp32 numbers; Yt is fp32-exact, dz and dh are bf16-exact (the type the
    kernel stores them in for dW2, dH and dW1); H is exactly 1 on the real
    hidden units whatever X holds."""
    case = op.make_probe(inst, B, kind)
    g, T = case.g, case.g.classes
    assert case.n_wg == (1 if B == case.rt else 2)

    _, Hpre, H, z = o64r.step64_reg(g, case.Xbf, case.Yt, case.W1bf, case.W2bf,
                                    case.master, 1.0)
    assert (Hpre == 1).all() and (H == 1).all()
    assert torch.equal(z, case.z.expand_as(z)) and (z % 2 == 0).all()
    d = z - case.Yt.to(F64)[:, :T]
    assert torch.equal(d, case.D)
    # the kernel's own d: an fp32 subtraction of two fp32 numbers
    assert torch.equal((z.float() - case.Yt[:, :T]).to(F64), case.D)
    assert _exact_in(d, torch.bfloat16)
    cmap, sgn = op.column_map(g)
    dh = d[:, cmap] * sgn
    assert torch.equal(dh, d @ o64._real_operands(g, case.W1bf, case.W2bf, case.master)[2].T)
    assert _exact_in(dh, torch.bfloat16)
    # at most one non-zero row per tile and column: the in-tile sum is exact
    for w in range(case.n_wg):
        for j in range(case.n_tiles):
            rows = op.rows_of(case, w, j)
            assert ((case.D[rows] != 0).sum(dim=0) <= 1).all()
            grads = op.oracle_rows(case, rows)
            seg = o64.real_segments(g, grads)
            assert torch.equal(seg["b2"], case.part_b2[w, j, :T])
            assert torch.equal(seg["b1"], case.part_b1[w, j, : g.hidden])
            if kind == "loss":
                assert float(grads[g.nparam]) == float(case.part_loss[w, j])
    for part in (case.part_b1, case.part_b2, case.part_loss):
        if part is not None:
            assert _exact_in(part, torch.float32)
    # pads and all-tail tiles contribute exact zeros
    assert (case.part_b2[:, :, T:] == 0).all() and (case.part_b1[:, :, g.hidden:] == 0).all()
    if case.n_wg == 2:
        assert (case.part_b2[1, 2:] == 0).all() and (case.part_b1[1, 2:] == 0).all()
        probed = slice(0, T) if kind == "bias" else slice(T - 1, T)
        assert (case.part_b2[1, :2, probed] != 0).all()


# ---------------------------------------------------------------------------
# (b) discrimination
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n", [4, 8])
def test_only_the_equivalent_orders_go_undetected(n):
    """Every order of the n tiles, summed left to right in fp32: the ones
    that reproduce the documented sum on every arrangement are the identity
    and the exchange of the first two addends, the two that are equal for
    all inputs. A condition, not a measurement. The loss probe's addends are
    non-negative, so it can only place the large one: first or second."""
    perms = op.permutations(n)
    alive = np.ones(len(perms), bool)
    for arr in op.ARRANGEMENTS[n]:
        s = op.all_order_sums(arr, perms)
        assert (s == op.all_order_sums([-v for v in arr], perms) * -1).all()
        alive &= s == s[0]
    assert (perms[0] == np.arange(n)).all()
    twin = list(range(n))
    twin[0], twin[1] = 1, 0
    assert sorted(map(tuple, perms[alive])) == sorted([tuple(range(n)), tuple(twin)])

    half_sq = [0.5 * op.LOSS_D_BIG ** 2] + [0.5 * op.LOSS_D_SMALL ** 2] * (n - 1)
    assert half_sq[:2] == [2.0 ** 25, 2.0]
    s = op.all_order_sums(half_sq, perms)
    assert s[0] == 2.0 ** 25
    big_at = np.argmax(perms == 0, axis=1)
    assert ((s == s[0]) == (big_at <= 1)).all()


@pytest.mark.parametrize("cid,inst,B", [c for c in CASES if c[1][1] != 32],
                         ids=[c[0] for c in CASES if c[1][1] != 32])
def test_every_arrangement_is_probed_by_db2_and_db1(cid, inst, B):
    """The first workgroup's db2 columns, and the db1 entries through the
    column map, carry every arrangement of the tile count (up to sign)."""
    case = op.make_probe(inst, B, "bias")
    for part in (case.part_b2[0], case.part_b1[0]):
        cols = {tuple(part[:, i].tolist()) for i in range(part.shape[1])}
        for arr in op.ARRANGEMENTS[case.n_tiles]:
            assert tuple(arr) in cols or tuple(-v for v in arr) in cols


# ---------------------------------------------------------------------------
# (c) the slab-stored products
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("cid,inst,B", CASES, ids=IDS)
def test_products_of_the_probe_inputs_are_exactly_known(cid, inst, B):
    """dW1 and dW2 per workgroup. On the loss probe every sum of the step
    but the loss is a sum of small integers: the oracle's slab is made of
    fp32 numbers, and the fp32 bf16-mirroring reference, which sums in
    another order again, gives the same bits. On the bias probe the oracle's
    dW2 is the column sum of the designed partials over the hidden units,
    its dW1 the designed dh against X, both finite."""
    for kind in ("bias", "loss"):
        case = op.make_probe(inst, B, kind)
        g = case.g
        cmap, sgn = op.column_map(g)
        for w in range(case.n_wg):
            rows = op.rows_of(case, w)
            grads = op.oracle_rows(case, rows)
            assert torch.isfinite(grads).all()
            assert (grads[: g.nparam][o64.pad_mask(g)] == 0).all()
            seg = o64.real_segments(g, grads)
            db2 = case.part_b2[w].sum(dim=0)[: g.classes]          # fp64: exact
            assert torch.equal(seg["W2"], db2.expand(g.hidden, -1))
            dh = case.D[rows][:, cmap] * sgn
            assert torch.equal(seg["W1"], case.Xbf[rows].to(F64)[:, : g.in_features].T @ dh)
            assert seg["W1"].abs().max() > 0
            if kind == "loss":
                assert _exact_in(grads[: g.nparam], torch.float32)
                sub = type(case)(**{**vars(case), "Xbf": case.Xbf[rows], "Yt": case.Yt[rows]})
                mirrored = o64r.reference_step_reg(sub)
                assert torch.equal(mirrored[: g.nparam].to(F64), grads[: g.nparam])
