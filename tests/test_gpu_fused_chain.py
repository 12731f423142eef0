"""GPU tests for the fused step's dependent-latency chain: the DPP row
reduction (bit-exact against the shuffle butterfly it replaced), the
single-round-trip prologue at the batch shapes where its tail handling can
go wrong, the prefetched labels of the batch tail, and the persistent
kernel's per-chunk label prefetch."""

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3


@pytest.fixture(scope="module")
def ext():
    from unionml_amd.ops import hip_ext

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    return hip_ext(required=True)  # must be the real extension on a GPU box


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _batch(B, seed):
    """Seeded, CPU-generated minibatch (asymmetric operands)."""
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(B, 64, generator=g) * 1.2 + 0.1).bfloat16()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    return X, y


def _fused_steps(ext, clf, Xbf, y, n_steps, use_wimg=False, B=None):
    """n_steps fused steps on one minibatch; returns the loss tensor."""
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS

    B = Xbf.size(0) if B is None else B
    clf._ensure_slabs((B + 127) // 128)
    loss_out = clf.grads[ref.NPARAM : ref.NPARAM + 1]
    for _ in range(n_steps):
        assert ext.mlp_step_fused(
            Xbf, y, clf.W1bf, clf.W2bf, clf.master, clf.bfmirror, clf.m, clf.v,
            clf.t_dev, clf.slabs, clf.counter, loss_out, 1.0 / B, LR,
            ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
            wimg=clf.wimg if use_wimg else None,
        )
    torch.cuda.synchronize()
    return loss_out


# ---------------------------------------------------------------------------
# row_sum16: DPP helper vs the plain shuffle butterfly
# ---------------------------------------------------------------------------


def test_reduce_selftest_bit_exact(ext, dev):
    """The DPP row reduction and the xor-1/2/4/8 shuffle butterfly pair the
    same operands in the same tree, so every lane's result has the same
    bits. Magnitudes spread over 12 decades with mixed signs make any other
    summation order show in the last bits."""
    g = torch.Generator().manual_seed(1234)
    mag = 10.0 ** (torch.rand(256, 64, generator=g) * 12.0 - 6.0)
    sign = torch.randint(0, 2, (256, 64), generator=g).float() * 2.0 - 1.0
    spread = (mag * sign).float()
    # all-equal rows: the sum of 16 equal floats is exactly 16 * v
    equal_vals = torch.tensor([1.0, -3.0, 0.1, 1e-30, -7.5e20, 0.0, 3.1415927, 1e-6])
    equal = equal_vals[:, None].expand(-1, 64).contiguous()
    # one non-zero lane per row, at every position of a row of 16 and in
    # every row group
    single = torch.zeros(64, 64)
    single[torch.arange(64), torch.arange(64)] = torch.arange(1, 65).float() * 0.37
    x = torch.cat([spread, equal, single]).to(dev)

    out = ext.reduce_selftest(x)
    torch.cuda.synchronize()
    assert out.shape == (x.size(0), 64, 2)
    new, old = out[..., 0].cpu(), out[..., 1].cpu()
    assert torch.isfinite(new).all()
    assert torch.equal(new, old), "DPP row sum differs from the shuffle butterfly"

    # and both compute the in-row sum (not merely the same wrong thing)
    exact = x.cpu().double().view(-1, 4, 16).sum(-1, keepdim=True).expand(-1, -1, 16)
    absum = x.cpu().double().abs().view(-1, 4, 16).sum(-1, keepdim=True).expand(-1, -1, 16)
    # 4 levels of fp32 adds: |error| <= gamma_4 * sum|x|, gamma_n = n*u / (1 - n*u)
    u = 2.0**-24
    gamma4 = 4 * u / (1 - 4 * u)
    assert ((new.double().view(-1, 4, 16) - exact).abs() <= gamma4 * absum).all()
    n0 = spread.size(0)
    assert torch.equal(new[n0 : n0 + 8], (equal * 16.0))
    lanes = torch.arange(64)
    want = torch.zeros(64, 64)
    for r in range(64):
        want[r, (lanes // 16) == (r // 16)] = single[r, r]
    assert torch.equal(new[n0 + 8 :], want)


# ---------------------------------------------------------------------------
# fused step vs mlp_step + adam_step at the prologue's edge shapes
# ---------------------------------------------------------------------------


@pytest.mark.parametrize("use_wimg", [False, True], ids=["plain", "wimg"])
@pytest.mark.parametrize("B", [1, 127, 129, 384])
def test_fused_step_matches_unfused_at_edge_batches(ext, dev, B, use_wimg):
    """B=1: one valid row in the grid; 127: tail inside the only workgroup;
    129: the second workgroup holds one row (tail zeros and the -1 label on
    every other lane); 384: three full workgroups. Tolerances are those of
    test_gpu_kernels.py::test_step_fused_matches_stepwise (master 1e-4,
    loss 1e-3; the atomic-order drift of the unfused path); m and v are
    held to the master's bound. bfmirror is the bf16 rounding of master, so
    across the two paths it may differ by the master's bound plus one bf16
    ulp (2^-7 relative), and within the fused path it must be exact."""
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS, TabularMLP

    n_steps = 3
    Xc, yc = _batch(B, seed=100 + B)
    Xbf, y = Xc.to(dev), yc.to(dev)

    a = TabularMLP(device=dev, seed=6)
    for _ in range(n_steps):
        a.grads.zero_()
        ext.mlp_step(Xbf, y, a.W1bf, a.W2bf, a.master, a.grads, 1.0 / B)
        ext.adam_step(a.master, a.bfmirror, a.grads, a.m, a.v, a.t_dev,
                      LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS)
    torch.cuda.synchronize()

    b = TabularMLP(device=dev, seed=6)
    loss_out = _fused_steps(ext, b, Xbf, y, n_steps, use_wimg=use_wimg)

    assert int(b.t_dev.item()) == n_steps
    assert torch.isfinite(b.master).all()
    err = (a.master - b.master).abs().max().item()
    err_m = (a.m - b.m).abs().max().item()
    err_v = (a.v - b.v).abs().max().item()
    err_loss = abs(loss_out.item() - a.grads[ref.NPARAM].item())
    print(f"B={B} wimg={use_wimg}: master {err:.3e} m {err_m:.3e} v {err_v:.3e} "
          f"loss {err_loss:.3e}")
    assert err < 1e-4, f"master mismatch {err}"
    assert err_m < 1e-4, f"m mismatch {err_m}"
    assert err_v < 1e-4, f"v mismatch {err_v}"
    assert err_loss < 1e-3, f"loss mismatch {err_loss}"
    assert torch.equal(b.bfmirror, b.master.bfloat16()), "bfmirror != bf16(master)"
    mirror_gap = (a.bfmirror.float() - b.bfmirror.float()).abs()
    # |bf(x) - bf(y)| <= |x - y| + (|x| + |y|) * 2^-8, with |y| <= |x| + 1e-4
    assert (mirror_gap <= 1e-4 * (1 + 2.0**-8) + 2.0**-7 * a.master.abs()).all()
    if use_wimg:  # the packed image the next prologue copies stays in sync
        rebuilt = TabularMLP(device=dev, seed=6)
        rebuilt.master.copy_(b.master)
        rebuilt.bfmirror.copy_(b.master.bfloat16())
        rebuilt._build_wimg()
        assert torch.equal(rebuilt.wimg, b.wimg)


# ---------------------------------------------------------------------------
# batch tail: X and y as the last B elements of their allocations
# ---------------------------------------------------------------------------


def test_tail_rows_read_nothing_beyond_batch(ext, dev):
    """B = 129 with X and y as views ending exactly at the end of larger
    tensors, against the same batch at the start of a roomy allocation whose
    rows beyond B hold NaN features and out-of-range labels: a prologue that
    touched a row or label at or beyond B would change the roomy result. The
    fused step is bit-reproducible, so the two must be equal."""
    from unionml_amd.ops.tabular import TabularMLP

    B, pad = 129, 4096
    Xc, yc = _batch(B, seed=77)

    X_end = torch.full((pad + B, 64), 3.0, dtype=torch.bfloat16, device=dev)
    y_end = torch.full((pad + B,), 5, dtype=torch.int32, device=dev)
    X_end[pad:] = Xc.to(dev)
    y_end[pad:] = yc.to(dev)
    X_tail, y_tail = X_end[pad:], y_end[pad:]
    assert X_tail.is_contiguous() and y_tail.is_contiguous()
    assert X_tail.data_ptr() + B * 64 * 2 == X_end.data_ptr() + X_end.numel() * 2
    assert y_tail.data_ptr() + B * 4 == y_end.data_ptr() + y_end.numel() * 4

    X_room = torch.full((B + 256, 64), float("nan"), dtype=torch.bfloat16, device=dev)
    y_room = torch.full((B + 256,), 1 << 20, dtype=torch.int32, device=dev)
    X_room[:B] = Xc.to(dev)
    y_room[:B] = yc.to(dev)

    results = []
    for Xv, yv in ((X_tail, y_tail), (X_room[:B], y_room[:B])):
        for use_wimg in (False, True):
            c = TabularMLP(device=dev, seed=3)
            loss = _fused_steps(ext, c, Xv, yv, 3, use_wimg=use_wimg)
            results.append([t.clone() for t in (c.master, c.m, c.v, c.bfmirror, loss)])
    tail_plain, tail_wimg, room_plain, room_wimg = results
    for got, want in ((tail_plain, room_plain), (tail_wimg, room_wimg)):
        assert all(torch.isfinite(t.float()).all() for t in got)
        assert all(torch.isfinite(t.float()).all() for t in want)
        for t0, t1 in zip(got, want):
            assert torch.equal(t0, t1), "tail placement changed the result"


# ---------------------------------------------------------------------------
# persistent kernel: per-chunk label prefetch
# ---------------------------------------------------------------------------


def test_train_steps_kernel_matches_fused_steps(ext, dev):
    """mlp_train_steps for 4 steps at B=128 over N=256 rows (two different
    chunks, each loaded with its labels) against four fused steps on the
    same minibatch slices. Tolerances: those of
    test_gpu_kernels.py::test_train_steps_kernel_matches_stepwise."""
    from unionml_amd.ops import reference as ref
    from unionml_amd.ops.tabular import ADAM_BETA1, ADAM_BETA2, ADAM_EPS, TabularMLP

    N, B, n_steps = 256, 128, 4
    Xc, yc = _batch(N, seed=55)
    Xbf, y = Xc.to(dev), yc.to(dev)

    a = TabularMLP(device=dev, seed=4)
    for s in range(n_steps):
        off = (s % (N // B)) * B
        _fused_steps(ext, a, Xbf[off : off + B], y[off : off + B], 1)

    b = TabularMLP(device=dev, seed=4)
    loss_out = b.grads[ref.NPARAM : ref.NPARAM + 1]
    assert ext.mlp_train_steps(Xbf, y, B, n_steps, b.master, b.bfmirror, b.m, b.v,
                               b.t_dev, loss_out, LR, ADAM_BETA1, ADAM_BETA2, ADAM_EPS)
    torch.cuda.synchronize()

    assert int(a.t_dev.item()) == n_steps and int(b.t_dev.item()) == n_steps
    err = (a.master - b.master).abs().max().item()
    err_m = (a.m - b.m).abs().max().item()
    print(f"persistent vs fused: master {err:.3e} m {err_m:.3e}")
    assert err < 1e-5, f"master mismatch {err}"
    assert err_m < 1e-6, f"moment mismatch {err_m}"
