"""Order-probe inputs for the generalized step kernel (mlp_step_gen_kernel,
regression head): cases in which nothing rounds before the three sums the
kernel takes over a workgroup's 16-row tiles (db1, db2, loss), every
per-tile partial is an exactly known fp32 number, and the fp32 sum of those
partials depends on the order they are added in. The kernel documents the
order, tile 0 first and left to right, ((p0 + p1) + p2) + ...; a test that
knows the partials can hold it to that order bit for bit, where comparing
two runs only shows that the waves arrived alike twice.

The construction, for an instantiation <HID, RT, CPAD> (launch with
rt=RT and invBtot = 1):

  * W1 = 0 and b1 = 1 on the real hidden units: H = 1 in every row whatever
    X holds (small integers, so that dW1 is not trivially zero), the ReLU
    mask is all ones.
  * Each real hidden unit h feeds one target column c(h) = h mod T with
    weight s(h) = +-1, every other W2 entry is 0. So z[c] is a small
    integer, made even by b2[c] in {0, 1}, and dh[h][row] =
    s(h) * dz[row][c(h)]: one non-zero product per MFMA output.
  * Yt[row][c] = z[c] - D[row][c] for designed residuals D, so the kernel's
    d = z - Yt = D and, with invBtot = 1, dz = D exactly.
  * "bias" probes: in each tile j and real column c exactly one row carries
    D = p[c][j], the rest 0. The p are +-2^24, 1 and 3: exact in bf16 (the
    type dz and dh are stored in for the products), the in-tile row sum has
    a single non-zero addend, and the tile's db2 partial is p[c][j], its
    db1 partial s(h) * p[c(h)][j].
  * "loss" probe (a launch of its own): one column, one row per tile with
    d = 2^13 in tile 0 and d = 2 in the others; tile partials 0.5 d^2 are
    2^25 and 2, and 2^25 + 2 rounds back to 2^25. Every other sum of this
    launch is a sum of small integers, exact in any order, so its whole
    slab equals the fp64 oracle's.

No tests live in this module (tests/test_order_probe_cpu.py checks the
construction on the CPU, tests/test_gpu_gen_order.py runs the kernel)."""

import itertools
from types import SimpleNamespace

import numpy as np
import torch

import oracle64 as o64
import oracle64_reg as o64r
from oracle64 import F64
from unionml_amd.ops.reference import HEAD_REGRESSION, Geometry

BIG = 2.0 ** 24
TILE = 16

# Per-column arrangements of the tile partials, by tile count RT/16. Column c
# takes ARRANGEMENTS[n][c % len], negated on every other pass through the
# list. The sets for 4 and 8 tiles are chosen so that no order but the
# documented one and its twin (first two addends exchanged: fp32 addition
# commutes) reproduces the documented sums of all of them;
# test_order_probe_cpu.py enumerates every order to show it. Two addends
# cannot discriminate: the RT = 32 cases are there for coverage only.
ARRANGEMENTS = {
    2: [(BIG, 1.0), (1.0, -BIG)],
    4: [(1.0, BIG, -BIG, 1.0), (-BIG, 1.0, 1.0, BIG)],
    8: [(-BIG, -BIG, 1.0, 1.0, 1.0, BIG, 3.0, BIG),
        (3.0, BIG, -BIG, 1.0, 1.0, 1.0, -BIG, BIG),
        (-BIG, 1.0, BIG, 1.0, BIG, -BIG, 1.0, 3.0)],
}

# loss probe: d of the carrying row, by tile; 0.5 d^2 = 2^25, 2, 2, ...
LOSS_D_BIG, LOSS_D_SMALL = 2.0 ** 13, 2.0

IN_FEATURES = 20   # one k-tile; the input width plays no part in the sums


def instantiations():
    """The regression step's (HID, RT, CPAD), as oracle64_reg lists them"""
    return [inst for inst, _ in o64r.STEP_INSTANTIATIONS]


def probe_shape(inst):
    """(in_features, hidden, targets) that selects ``inst`` with three pad
    hidden units and three pad target columns"""
    hid, _, cpad = inst
    return (IN_FEATURES, hid - 3, cpad - 3)


def batches(inst):
    """B = RT: one workgroup, every tile full. B = RT + 17: a second
    workgroup with one full tile, one tile of a single row and all-tail
    tiles after it. RT = 32: one two-tile case."""
    rt = inst[1]
    return (rt,) if rt == 32 else (rt, rt + 17)


def cases():
    """[(id, inst, B)]"""
    return [(f"{o64.inst_id(inst)}-B{B}", inst, B) for inst in instantiations()
            for B in batches(inst)]


def column_map(g: Geometry):
    """(c, s): target column and sign of each real hidden unit"""
    h = torch.arange(g.hidden)
    return h % g.classes, torch.where(h % 3 == 2, -1.0, 1.0).to(F64)


def arrangement(n_tiles: int, c: int):
    arr = ARRANGEMENTS[n_tiles]
    sign = -1.0 if (c // len(arr)) % 2 else 1.0
    return tuple(sign * v for v in arr[c % len(arr)])


def sum_in_order(parts: torch.Tensor, order=None) -> torch.Tensor:
    """fp32 sum over dim 0 of ``parts`` [n][...] taken left to right,
    ((p[o0] + p[o1]) + p[o2]) + ...: the documented order when ``order`` is
    None. One fp32 rounding per addition."""
    p = parts.to(torch.float32)
    order = range(p.shape[0]) if order is None else order
    it = iter(order)
    s = p[next(it)].clone()
    for j in it:
        s = s + p[j]
    return s


def all_order_sums(values, perms: np.ndarray) -> np.ndarray:
    """The left-to-right fp32 sum of ``values`` under every row of ``perms``"""
    a = np.asarray(values, dtype=np.float32)[perms]
    s = a[:, 0].copy()
    for j in range(1, a.shape[1]):
        s = (s + a[:, j]).astype(np.float32)
    return s


def permutations(n: int) -> np.ndarray:
    return np.array(list(itertools.permutations(range(n))))


def make_probe(inst, B: int, kind: str):
    """Inputs and designed partials of one probe launch; ``kind`` is "bias"
    or "loss". The designed per-tile partials, fp64 and exact:
    part_b1 [n_wg][RT/16][hid], part_b2 [n_wg][RT/16][cpad],
    part_loss [n_wg][RT/16] (None for "bias": its loss is not probed)."""
    assert kind in ("bias", "loss")
    hid_c, rt, cpad_c = inst
    shape = probe_shape(inst)
    g = Geometry(*shape, head=HEAD_REGRESSION)
    assert (g.hid, g.cpad) == (hid_c, cpad_c)
    T, n_tiles = g.classes, rt // TILE
    n_wg = (B + rt - 1) // rt
    cmap, sgn = column_map(g)

    master = torch.zeros(g.nparam)
    seg = o64.real_segments(g, master)
    seg["b1"].fill_(1.0)
    W2 = torch.zeros(g.hidden, T, dtype=F64)
    W2[torch.arange(g.hidden), cmap] = sgn
    acc = W2.sum(dim=0)                      # z before the bias: H = 1
    b2 = torch.remainder(acc, 2.0)           # 0 or 1: makes z even
    z = acc + b2
    seg["W2"].copy_(W2)
    seg["b2"].copy_(b2)
    bfmirror = master.bfloat16()
    assert torch.equal(bfmirror.float(), master)

    gen = torch.Generator().manual_seed(100 * hid_c + rt + cpad_c + B)
    Xbf = torch.zeros(B, g.inp, dtype=torch.bfloat16)
    Xbf[:, : g.in_features] = torch.randint(-2, 3, (B, g.in_features),
                                            generator=gen).to(torch.bfloat16)

    # designed residuals D [B][T] and per-tile db2 partials P [n_wg][tiles][T]
    D = torch.zeros(B, T, dtype=F64)
    P = torch.zeros(n_wg, n_tiles, T, dtype=F64)
    cols = range(T) if kind == "bias" else (T - 1,)
    for w in range(n_wg):
        for j in range(n_tiles):
            first = w * rt + j * TILE
            rows_here = min(TILE, B - first)
            if rows_here <= 0:
                continue                      # an all-tail tile: partial 0
            for c in cols:
                if kind == "bias":
                    p = arrangement(n_tiles, c)[j]
                else:
                    p = LOSS_D_BIG if j == 0 else LOSS_D_SMALL
                D[first + (5 * j + 3 * c) % rows_here, c] = p
                P[w, j, c] = p

    Yt64 = z - D
    Yt = torch.zeros(B, g.cpad)
    Yt[:, :T] = Yt64.float()
    assert torch.equal(Yt[:, :T].to(F64), Yt64), "a target is not an fp32 number"

    part_b2 = torch.zeros(n_wg, n_tiles, g.cpad, dtype=F64)
    part_b2[:, :, :T] = P
    part_b1 = torch.zeros(n_wg, n_tiles, g.hid, dtype=F64)
    part_b1[:, :, : g.hidden] = P[:, :, cmap] * sgn
    part_loss = 0.5 * (P * P).sum(dim=2) if kind == "loss" else None

    W1bf = bfmirror[g.off_w1 : g.off_w1 + g.inp * g.hid].view(g.inp, g.hid)
    W2bf = bfmirror[g.off_w2 : g.off_w2 + g.hid * g.cpad].view(g.hid, g.cpad)
    return SimpleNamespace(
        inst=inst, kind=kind, shape=shape, B=B, rt=rt, n_wg=n_wg, n_tiles=n_tiles, g=g,
        seed=0, master=master, bfmirror=bfmirror, W1bf=W1bf, W2bf=W2bf, Xbf=Xbf, Yt=Yt,
        invB=1.0, D=D, z=z, part_b1=part_b1, part_b2=part_b2, part_loss=part_loss,
        # what gpu_reg() of test_gpu_reg_oracle.py copies besides the weights
        y_mean=torch.zeros(T), y_invstd=torch.ones(T), y_scale=torch.ones(T),
    )


def rows_of(case, w: int, j: int = None):
    """The batch rows of workgroup ``w`` (of its tile ``j``): a slice"""
    lo = w * case.rt + (0 if j is None else j * TILE)
    hi = (w + 1) * case.rt if j is None else lo + TILE
    return slice(min(lo, case.B), min(hi, case.B))


def oracle_rows(case, rows: slice) -> torch.Tensor:
    """Flat fp64 oracle gradients (+loss) of the rows alone, invB = 1; zeros
    for an empty slice"""
    if rows.start >= rows.stop:
        return torch.zeros(case.g.nparam + 1, dtype=F64)
    return o64r.step64_reg(case.g, case.Xbf[rows], case.Yt[rows], case.W1bf, case.W2bf,
                           case.master, 1.0)[0]
