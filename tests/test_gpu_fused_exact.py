"""The fused step (mlp_step_fused_kernel) held bit for bit at the grid sizes
training runs, after its cross-workgroup hand-off: the parallel tag poll
(second round above 64 workgroups), the Adam-state prefetch (off at one
workgroup, on from two), the striped 8-chain slab reduction (with and
without its remainder loop, and with an empty last stripe at 65
workgroups), the in-kernel Adam and the packed-image upkeep.

The kernel is bit-reproducible (test_gpu_kernels.py::
test_step_kernels_reproducible_bitwise) and every Adam entry point compiles
to one arithmetic (tabular_common.h adam_update), so two model instances
driven down different paths are comparable with torch.equal: no tolerance
in this file.

Grids stay at or below 65 workgroups: all workgroups of this kernel must be
co-resident, and the suite stays far inside one workgroup per CU."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3
ROWS = 128            # rows per workgroup of the specialized kernel
N_STEPS = 3
SENTINEL = -7.0

# (n_wg, rows in the last workgroup): B = 128 * (n_wg - 1) + r. 1: no
# prefetch; 2: prefetch on; 7: remainder loop only; 8, 16, 64: unrolled
# chains only; 9, 17: both; 64: every lane of the tag poll; 65: a second
# poll round and an empty last stripe (ceil(2609 / 65) = 41, 64 * 41 > 2608).
GRIDS = [(1, 127), (2, 1), (3, 128), (7, 127), (8, 128), (9, 1), (16, 128), (17, 1),
         (64, 127), (65, 1)]
GRID_IDS = [f"wg{n}-r{r}" for n, r in GRIDS]


def rows_of(n_wg, r):
    return ROWS * (n_wg - 1) + r


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _batch(B, seed):
    """Seeded, CPU-generated minibatch (as test_gpu_fused_chain.py::_batch),
    on the device; computed once per (B, seed) and never written."""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X.to("cuda:0"), y.to("cuda:0")


def _adam_args():
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    return LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS


def _model(dev, seed=6):
    from unionml_amd.ops.tabular import TabularMLP

    return TabularMLP(device=dev, seed=seed)


def _launch(ext, c, Xbf, y, *, wimg, grads_out=None, loss_out=None):
    """One mlp_step_fused launch on model ``c``'s own slabs and counter"""
    from unionml_amd.ops import reference as ref

    if loss_out is None:
        loss_out = c.grads[ref.NPARAM : ref.NPARAM + 1]
    assert ext.mlp_step_fused(
        Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev,
        c.slabs, c.counter, loss_out, 1.0 / Xbf.size(0), *_adam_args(),
        grads_out=grads_out, wimg=wimg,
    )


def _state(c, loss):
    """Everything a step leaves behind, cloned"""
    return {
        "master": c.master.clone(), "m": c.m.clone(), "v": c.v.clone(),
        "bfmirror": c.bfmirror.clone(), "loss": loss.clone(), "t_dev": c.t_dev.clone(),
        "wimg": c.wimg.clone(),
    }


def _assert_same(got, want, what, keys=None):
    for k in keys or want:
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs"


def _rebuilt_wimg(c):
    """The packed image built afresh from c.master (c.wimg is put back)"""
    kept = c.wimg.clone()
    c._build_wimg()
    fresh = c.wimg.clone()
    c.wimg.copy_(kept)
    return fresh


# ---------------------------------------------------------------------------
# (a) full mode == reduce-only mode + adam_step
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n_wg,r", GRIDS, ids=GRID_IDS)
def test_full_mode_equals_reduce_only_plus_adam_step(ext, dev, n_wg, r):
    """Three steps from one seed. Model a: mlp_step_fused in full mode (Adam
    in the kernel, on each workgroup's stripe, from the prefetched state).
    Model b: mlp_step_fused(grads_out=) and then adam_step_kernel, the DP
    path's sequence. Same slab sums, same adam_update: master, m, v,
    bfmirror, loss and t_dev must be equal, without the packed weight image
    and with it; with it the two images are equal and are the image of the
    final master; and the plain and the image runs equal each other (the
    image holds the very bf16 weights bfmirror does)."""
    from unionml_amd.ops import reference as ref

    B = rows_of(n_wg, r)
    Xbf, y = _batch(B, seed=100 + n_wg)
    results = {}
    for use_wimg in (False, True):
        a, b = _model(dev), _model(dev)
        for c in (a, b):
            c._ensure_slabs(n_wg)
        for _ in range(N_STEPS):
            _launch(ext, a, Xbf, y, wimg=a.wimg if use_wimg else None)
            _launch(ext, b, Xbf, y, wimg=b.wimg if use_wimg else None, grads_out=b.grads)
            ext.adam_step(b.master, b.bfmirror, b.grads, b.m, b.v, b.t_dev, *_adam_args(),
                          wimg=b.wimg if use_wimg else None)
        torch.cuda.synchronize()
        sa = _state(a, a.grads[ref.NPARAM : ref.NPARAM + 1])
        sb = _state(b, b.grads[ref.NPARAM : ref.NPARAM + 1])
        tag = f"n_wg={n_wg} wimg={use_wimg}"
        assert int(a.t_dev.item()) == N_STEPS and int(a.counter.item()) == N_STEPS
        assert int(b.counter.item()) == N_STEPS
        assert all(torch.isfinite(t.float()).all() for t in sa.values()), tag
        keys = [k for k in sa if k != "wimg" or use_wimg]
        _assert_same(sa, sb, f"full vs reduce+adam_step, {tag}", keys)
        assert torch.equal(sa["bfmirror"], sa["master"].bfloat16()), tag
        if use_wimg:
            assert torch.equal(sa["wimg"], _rebuilt_wimg(a)), f"{tag}: image != image of master"
        results[use_wimg] = sa
    keys = [k for k in results[True] if k != "wimg"]
    _assert_same(results[True], results[False], f"wimg vs plain, n_wg={n_wg}", keys)


# ---------------------------------------------------------------------------
# (b) the slab reduction against a plain host sum of the same slabs
# ---------------------------------------------------------------------------


def host_slab_sum(slabs):
    """fp32 sum of the rows of ``slabs`` [n_wg][n] (CPU) in the kernel's
    order: eight chains g_k += slab[w + k] over w = 0, 8, ..., the remainder
    rows into g_0, then ((g0+g1)+(g2+g3))+((g4+g5)+(g6+g7)). The build has
    no fast-math, so the kernel's adds are these adds."""
    assert slabs.dtype == torch.float32 and slabs.device.type == "cpu"
    n_wg = slabs.size(0)
    g = [torch.zeros(slabs.size(1)) for _ in range(8)]
    w = 0
    while w + 8 <= n_wg:
        for k in range(8):
            g[k] = g[k] + slabs[w + k]
        w += 8
    while w < n_wg:
        g[0] = g[0] + slabs[w]
        w += 1
    return ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]))


def _bits(x):
    return x.contiguous().view(torch.int32)


@pytest.mark.parametrize("n_wg,r", GRIDS, ids=GRID_IDS)
def test_slab_reduction_is_the_documented_sum(ext, dev, n_wg, r):
    """Reduce-only launches leave the per-workgroup slabs in place: the
    summed gradients (+loss) handed out must be, bit for bit, the host sum
    of those slabs in the documented order. Slabs allocated by hand, 4 rows
    more than the grid, the used part NaN (every entry summed was stored in
    this launch) and the rest a sentinel: the extra rows, tag word included,
    stay untouched; every used row's tag equals the launch counter; and the
    counter counts launches, across both modes (1 reduce-only, then 1 full,
    then 1 reduce-only)."""
    from unionml_amd.ops import reference as ref

    NP = ref.NPARAM
    TAG = NP + 1
    EXTRA, GUARD = 4, 3
    B = rows_of(n_wg, r)
    Xbf, y = _batch(B, seed=100 + n_wg)
    c = _model(dev)
    c.slabs = torch.full((n_wg + EXTRA, ext.SLAB), SENTINEL, device=dev)
    c.slabs[:n_wg, : NP + 1] = float("nan")
    c.counter = torch.zeros(1, dtype=torch.uint32, device=dev)
    sentinel_bits = int(_bits(torch.tensor([SENTINEL]))[0])

    def check(launches, grads_out):
        torch.cuda.synchronize()
        tag = f"n_wg={n_wg} after {launches} launch(es)"
        assert int(c.counter.item()) == launches, tag
        slabs = c.slabs.cpu()
        assert (_bits(slabs[n_wg:]) == sentinel_bits).all(), f"{tag}: wrote past the grid's slabs"
        assert (_bits(slabs[:n_wg, TAG]) == launches).all(), f"{tag}: slab tags"
        got = grads_out.cpu()
        assert (got[NP + 1 :] == SENTINEL).all(), f"{tag}: wrote past grads_out[nparam]"
        assert torch.isfinite(got).all(), tag
        want = host_slab_sum(slabs[:n_wg, : NP + 1].contiguous())
        diff = _bits(got[: NP + 1]) != _bits(want)
        assert not diff.any(), (
            f"{tag}: {int(diff.sum())} of {NP + 1} sums differ from the host sum, "
            f"first at {int(diff.nonzero()[0])}")

    def reduce_only():
        out = torch.full((NP + 1 + GUARD,), SENTINEL, device=dev)
        _launch(ext, c, Xbf, y, wimg=c.wimg, grads_out=out)
        return out

    master0 = c.master.clone()
    check(1, reduce_only())
    assert int(c.t_dev.item()) == 0 and torch.equal(c.master, master0)
    _launch(ext, c, Xbf, y, wimg=c.wimg)          # full mode: weights move
    check(3, reduce_only())
    assert int(c.t_dev.item()) == 1 and not torch.equal(c.master, master0)


# ---------------------------------------------------------------------------
# (c) grid size changing from step to step, eager and captured
# ---------------------------------------------------------------------------

EPOCHS = 3


@pytest.mark.parametrize("N,batch_size,grids", [(2177, 2048, (16, 2)), (8193 + 130, 8193, (65, 2))],
                         ids=["16-then-2", "65-then-2"])
def test_changing_grid_eager_graph_and_dp_path_agree(ext, dev, N, batch_size, grids):
    """train_epochs whose two batches run on different grids (the slabs and
    tags of the larger grid stay behind while the smaller one runs): the
    captured-graph run, the eager run and the same batches stepped through
    _step(allreduce=False) (reduce-only + adam_step, the DP path at world
    size 1) land on the same bits."""
    Xbf, y = _batch(N, seed=7)
    batches = [(off, min(batch_size, N - off)) for off in range(0, N, batch_size)]
    assert tuple((bs + ROWS - 1) // ROWS for _, bs in batches) == grids
    n_steps = EPOCHS * len(batches)

    def trained(use_graph):
        c = _model(dev)
        loss = c.train_epochs(Xbf, y, epochs=EPOCHS, batch_size=batch_size, lr=LR,
                              use_graph=use_graph)
        torch.cuda.synchronize()
        assert int(c.t_dev.item()) == n_steps
        return _state(c, torch.tensor([loss])), c

    eager, _ = trained(False)
    graphed, c_graph = trained(True)
    assert c_graph._graph is not None, "the epoch was not captured"
    assert all(torch.isfinite(t.float()).all() for t in eager.values())
    _assert_same(graphed, eager, f"hipGraph vs eager, grids {grids}")

    c = _model(dev)
    for _ in range(EPOCHS):
        for off, bs in batches:
            loss = c._step(Xbf[off : off + bs], y[off : off + bs], 1.0 / bs, LR, False)
    torch.cuda.synchronize()
    assert int(c.t_dev.item()) == n_steps
    stepped = _state(c, torch.tensor([float(loss.item())]))
    _assert_same(stepped, eager, f"_step(allreduce=False) vs _fused_adam_step, grids {grids}")
    assert torch.equal(eager["wimg"], _rebuilt_wimg(c))


# ---------------------------------------------------------------------------
# (d) a captured epoch must not outlive its batch split
# ---------------------------------------------------------------------------


def test_graph_is_not_replayed_for_another_batch_split(ext, dev):
    """Two train_epochs calls on one model and the same tensors, batch_size
    520 and then 600 over N = 1000: both splits have two batches on at most
    5 workgroups (no slab reallocation), so a graph keyed on the NUMBER of
    batches would replay the first split, with its 1/bs, in the second call.
    Against the same two calls stepped eagerly."""
    N = 1000
    Xbf, y = _batch(N, seed=11)
    out = {}
    for use_graph in (False, True):
        c = _model(dev)
        losses = []
        for batch_size in (520, 600):
            assert len(range(0, N, batch_size)) == 2
            losses.append(c.train_epochs(Xbf, y, epochs=2, batch_size=batch_size, lr=LR,
                                         use_graph=use_graph))
        torch.cuda.synchronize()
        assert int(c.t_dev.item()) == 8
        assert c.slabs.size(0) == 5
        out[use_graph] = _state(c, torch.tensor(losses))
    _assert_same(out[True], out[False], "hipGraph vs eager over two batch splits")


def test_reallocating_slabs_drops_the_captured_graph(ext, dev):
    """A captured epoch holds the slabs' and the counter's addresses: when
    _ensure_slabs replaces them, the graph must go."""
    Xbf, y = _batch(1000, seed=11)
    c = _model(dev)
    c.train_epochs(Xbf[:256], y[:256], epochs=2, batch_size=128, lr=LR, use_graph=True)
    assert c._graph is not None and c.slabs.size(0) == 1
    c._ensure_slabs(1)
    assert c._graph is not None, "no reallocation, the graph stays"
    c._ensure_slabs(8)
    assert c.slabs.size(0) == 8
    assert c._graph is None and c._graph_key is None


# ---------------------------------------------------------------------------
# (e) gen family: full mode == reduce-only + adam_step_gen on the same slabs
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n_wg", [1, 5, 9])
@pytest.mark.parametrize("shape", [(1, 1, 2), (100, 50, 7)], ids=["1x1x2", "100x50x7"])
def test_gen_full_mode_equals_reduce_only_plus_adam_step_gen(ext, dev, shape, n_wg):
    """The slabs are written by hand (as
    test_gpu_oracle.py::test_reduce_gen_sum_vs_fp64 does), so that the two
    paths are compared on sums harder than a step kernel produces: values
    over 6 decades, mixed signs, a fresh set per step.
    reduce_adam_gen in full mode against reduce_adam_gen(grads_out=) +
    adam_step_gen, three steps."""
    from unionml_amd.ops.tabular import TabularMLP

    a = TabularMLP(*shape, device=dev, seed=4)
    b = TabularMLP(*shape, device=dev, seed=4)
    g = a.g
    gen = torch.Generator().manual_seed(1000 * n_wg + g.nparam)
    counter = torch.zeros(1, dtype=torch.uint32, device=dev)
    loss_a = torch.full((1,), SENTINEL, device=dev)
    loss_b = torch.full((1,), SENTINEL, device=dev)
    for _ in range(N_STEPS):
        mag = 10.0 ** (torch.rand(n_wg, g.slab_stride, generator=gen) * 6.0 - 3.0)
        sign = torch.where(torch.rand(n_wg, g.slab_stride, generator=gen) < 0.5, -1.0, 1.0)
        slabs = (mag * sign).float().to(dev)
        ext.reduce_adam_gen(slabs, n_wg, g.inp, g.hid, g.cpad, a.master, a.bfmirror, a.m,
                            a.v, a.t_dev, counter, loss_a, *_adam_args(), wimg=a.wimg)
        ext.reduce_adam_gen(slabs, n_wg, g.inp, g.hid, g.cpad, b.master, b.bfmirror, b.m,
                            b.v, b.t_dev, counter, loss_b, *_adam_args(), wimg=b.wimg,
                            grads_out=b.grads)
        ext.adam_step_gen(b.master, b.bfmirror, b.grads, b.m, b.v, b.t_dev, g.inp, g.hid,
                          g.cpad, *_adam_args(), wimg=b.wimg)
        torch.cuda.synchronize()
        assert int(counter.item()) == 0
    assert int(a.t_dev.item()) == N_STEPS
    assert float(loss_b.item()) == SENTINEL, "reduce-only mode wrote loss_out"
    sa = _state(a, loss_a)
    sb = _state(b, b.grads[g.nparam : g.nparam + 1])
    assert all(torch.isfinite(t.float()).all() for t in sa.values())
    _assert_same(sa, sb, f"gen full vs reduce+adam_step_gen, {shape} n_wg={n_wg}")
    assert torch.equal(sa["bfmirror"], sa["master"].bfloat16())
    assert torch.equal(sa["wimg"], _rebuilt_wimg(a))
