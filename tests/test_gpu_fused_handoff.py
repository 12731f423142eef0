"""The fused step's cross-workgroup hand-off (mlp_step_fused_kernel), tested
for STALENESS: the gradient slabs are stored write-through and loaded past
the L1 with no agent-scope fence on either side, so what could go wrong is a
workgroup summing slab bytes of an EARLIER launch. Every test here therefore
feeds consecutive launches different data (four seeded batches cycled per
grid) and checks every word a launch hands over.

Grids, in the (n_wg, rows in the last workgroup) notation of
test_gpu_fused_exact.py: (2, 1) prefetch on, remainder loop only; (9, 1) and
(17, 1) the unrolled chains together with the remainder loop; (65, 1) a
second poll round and an empty last stripe. B = 129, 1025, 2049, 8193.

Nothing here depends on timing and nothing provokes a fault: the tests run
the ordinary kernel, once on an idle device and once beside a busy copy
stream, and compare bits."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3
ROWS = 128            # rows per workgroup of the specialized kernel
N_BATCHES = 4         # distinct batches cycled per grid
GRIDS = [(2, 1), (9, 1), (17, 1), (65, 1)]
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
    """Seeded, CPU-generated minibatch (as test_gpu_fused_exact.py::_batch),
    on the device; computed once per (B, seed) and never written."""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X.to("cuda:0"), y.to("cuda:0")


def _batches(n_wg, r):
    """The grid's four batches; launch k takes batch k % 4"""
    B = rows_of(n_wg, r)
    out = [_batch(B, seed=4000 + 10 * n_wg + j) for j in range(N_BATCHES)]
    assert not torch.equal(out[0][0], out[1][0])
    return out


def _adam_args():
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    return LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS


def _model(dev, seed=6):
    from unionml_amd.ops.tabular import TabularMLP

    return TabularMLP(device=dev, seed=seed)


def _launch(ext, c, Xbf, y, *, grads_out=None):
    """One mlp_step_fused launch on model ``c``'s own slabs and counter, with
    the packed weight image (the training path's launch)"""
    from unionml_amd.ops import reference as ref

    assert ext.mlp_step_fused(
        Xbf, y, c.W1bf, c.W2bf, c.master, c.bfmirror, c.m, c.v, c.t_dev,
        c.slabs, c.counter, c.grads[ref.NPARAM : ref.NPARAM + 1], 1.0 / Xbf.size(0),
        *_adam_args(), grads_out=grads_out, wimg=c.wimg,
    )


def host_slab_sum(slabs):
    """fp32 sum of the rows of ``slabs`` [n_wg][n] (CPU) in the kernel's
    documented order: eight chains g_k += slab[w + k] over w = 0, 8, ..., the
    remainder rows into g_0, then ((g0+g1)+(g2+g3))+((g4+g5)+(g6+g7))."""
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


def _nan_slabs(c, ext, n_wg, dev):
    """Slabs for exactly ``n_wg`` workgroups, every payload word NaN and the
    tags zero, and a fresh launch counter: a word summed without having been
    stored in the launch shows as NaN, a word of an earlier launch as a
    wrong sum."""
    from unionml_amd.ops import reference as ref

    c.slabs = torch.zeros(n_wg, ext.SLAB, device=dev)
    c.slabs[:, : ref.NPARAM + 1] = float("nan")
    c.counter = torch.zeros(1, dtype=torch.uint32, device=dev)


def _reduce_only_and_check(ext, c, Xbf, y, n_wg, launches, what):
    """One reduce-only launch, then: the summed gradients (+loss) equal the
    host sum of the slabs this launch left, bit for bit; every tag equals the
    launch count; everything is finite."""
    from unionml_amd.ops import reference as ref

    NP = ref.NPARAM
    out = torch.full((NP + 1,), float("nan"), device=c.slabs.device)
    _launch(ext, c, Xbf, y, grads_out=out)
    torch.cuda.synchronize()
    tag = f"{what}, launch {launches}"
    assert int(c.counter.item()) == launches, tag
    slabs = c.slabs.cpu()
    assert (_bits(slabs[:n_wg, NP + 1]) == launches).all(), f"{tag}: slab tags"
    payload = slabs[:n_wg, : NP + 1].contiguous()
    got = out.cpu()
    assert torch.isfinite(payload).all(), f"{tag}: a slab word was not stored"
    assert torch.isfinite(got).all(), tag
    diff = _bits(got) != _bits(host_slab_sum(payload))
    assert not diff.any(), (
        f"{tag}: {int(diff.sum())} of {NP + 1} sums differ from the host sum of this "
        f"launch's slabs, first at {int(diff.nonzero()[0])}")
    return payload


# ---------------------------------------------------------------------------
# 1. every word fresh, every launch
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("n_wg,r", GRIDS, ids=GRID_IDS)
def test_every_word_fresh_every_launch(ext, dev, n_wg, r):
    """64 consecutive reduce-only launches on one model, batch k % 4 in
    launch k: the weights stay put, so the slabs change from launch to launch
    exactly as the batch does, and a stripe sum that took even one word of
    the launch before differs from the host sum of the current slabs."""
    batches = _batches(n_wg, r)
    c = _model(dev)
    _nan_slabs(c, ext, n_wg, dev)
    prev = None
    for k in range(64):
        Xbf, y = batches[k % N_BATCHES]
        payload = _reduce_only_and_check(ext, c, Xbf, y, n_wg, k + 1, f"n_wg={n_wg}")
        if prev is not None:      # the premise: consecutive launches differ
            assert not torch.equal(payload, prev)
        prev = payload
    assert int(c.t_dev.item()) == 0


# ---------------------------------------------------------------------------
# 2. under uneven load
# ---------------------------------------------------------------------------

N_STEPS = 128
COPY_ELEMS = 1 << 28      # 1 GiB of fp32 per copy
N_COPIES = 48             # tens of milliseconds of copies; the steps take a few


def _state(c):
    from unionml_amd.ops import reference as ref

    return {
        "master": c.master.clone(), "m": c.m.clone(), "v": c.v.clone(),
        "bfmirror": c.bfmirror.clone(), "wimg": c.wimg.clone(), "t_dev": c.t_dev.clone(),
        "loss": c.grads[ref.NPARAM : ref.NPARAM + 1].clone(),
    }


def _copy_buffers():
    src = torch.ones(COPY_ELEMS, device="cuda:0")
    return src, torch.empty_like(src)


@pytest.mark.parametrize("n_wg,r,use_graph", [(17, 1, True), (65, 1, False)],
                         ids=["wg17-two-graphs", "wg65-eager"])
def test_under_uneven_load_every_word_equal(ext, dev, n_wg, r, use_graph):
    """Two models from one seed take the same 128 full-mode steps (batch
    k % 4 in step k): at 17 workgroups as two replays of a 64-step captured
    graph, at 65 workgroups eagerly. One runs on an idle device, the other
    beside a side stream that was handed, BEFORE the steps, large
    device-to-device copies lasting several times as long as the steps, so
    the workgroups share their CUs and the memory system with other work and
    arrive unevenly. Every word the steps leave behind must be equal."""
    batches = _batches(n_wg, r)
    src, dst = _copy_buffers()
    side = torch.cuda.Stream(device=dev)

    def run(loaded):
        c = _model(dev)
        c._ensure_slabs(n_wg)

        def steps(n, on=c):
            for k in range(n):
                Xbf, y = batches[k % N_BATCHES]
                _launch(ext, on, Xbf, y)

        warm = _model(dev)           # the capture must not be the first launch
        warm._ensure_slabs(n_wg)
        steps(1, on=warm)

        graph = None
        if use_graph:
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):       # records, does not run
                steps(N_STEPS // 2)
        torch.cuda.synchronize()
        assert int(c.t_dev.item()) == 0
        if loaded:
            with torch.cuda.stream(side):
                for _ in range(N_COPIES):
                    dst.copy_(src, non_blocking=True)
        if use_graph:
            graph.replay()
            graph.replay()
        else:
            steps(N_STEPS)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        if loaded:                   # reported, not asserted: no timing in a test
            print(f"n_wg={n_wg}: copies still running when the steps ended: "
                  f"{not side.query()}")
        torch.cuda.synchronize()
        assert int(c.t_dev.item()) == N_STEPS and int(c.counter.item()) == N_STEPS
        return _state(c)

    idle = run(False)
    busy = run(True)
    assert all(torch.isfinite(t.float()).all() for t in idle.values())
    assert torch.isfinite(busy["loss"]).all()
    for k in idle:
        assert torch.equal(busy[k], idle[k]), f"n_wg={n_wg}: {k} differs under load"


# ---------------------------------------------------------------------------
# 3. mode mixing under the new stores
# ---------------------------------------------------------------------------


def test_alternating_modes_every_reduce_checked(ext, dev):
    """Reduce-only and full launches alternating on one model at 9
    workgroups, 32 of each, batch k % 4 in launch k. The full launches move
    the weights, so no two launches write the same slabs; after each
    reduce-only launch the handed-out sums are the host sum of that launch's
    slabs and every tag is the launch count, which counts both modes."""
    n_wg, r = 9, 1
    batches = _batches(n_wg, r)
    c = _model(dev)
    _nan_slabs(c, ext, n_wg, dev)
    for k in range(64):
        Xbf, y = batches[k % N_BATCHES]
        if k % 2 == 0:
            _reduce_only_and_check(ext, c, Xbf, y, n_wg, k + 1, "alternating, n_wg=9")
        else:
            _launch(ext, c, Xbf, y)
    torch.cuda.synchronize()
    assert int(c.counter.item()) == 64 and int(c.t_dev.item()) == 32
    assert torch.isfinite(c.master).all()
    assert torch.equal(c.bfmirror, c.master.bfloat16())
