"""Pure-PyTorch fp32 reference implementations of the CDNA4 kernels.

These are (a) the numerics oracle the GPU tests compare the HIP kernels
against, and (b) the CPU execution path, so the same user-facing API
runs everywhere. Layouts match the kernels exactly (flat master with
W2/b2 padded to 16 columns — tabular_kernels.hip OFF_* constants).
"""

from typing import Optional, Tuple

import torch

IN, HID, CLS, CPAD = 64, 32, 10, 16
OFF_W1, OFF_B1, OFF_W2, OFF_B2 = 0, 2048, 2080, 2592
NPARAM = 2608

# Every compiled (HID, RT, CPAD, PREDICT) instantiation of the generalized
# kernels, both heads: the copy of TABULAR_GEN_INSTANTIATIONS in
# hip/tabular_launch.h (tests/test_tabular_gen_cpu.py holds the two equal).
# RT is the rows per workgroup; PREDICT marks the row whose RT the predict
# kernel is compiled at too.
GEN_INSTANTIATIONS = (
    (32, 128, 16, True),
    (32, 64, 16, False),
    (64, 128, 16, True),
    (64, 64, 16, False),
    (128, 64, 16, True),
    (128, 32, 16, False),
    (256, 32, 16, True),
    (32, 128, 32, True),
    (64, 128, 32, True),
    (128, 64, 32, True),
    (256, 32, 32, True),
)
# hidden widths with a compiled gen-kernel instantiation
SUPPORTED_HID = tuple(sorted({h for h, _, _, _ in GEN_INSTANTIATIONS}))
MAX_CLASSES = 32


def compiled_rts(hid: int, cpad: int) -> Tuple[int, ...]:
    """The rows-per-workgroup values the step kernel is compiled at for a
    padded (hid, cpad), ascending."""
    return tuple(sorted(r for h, r, c, _ in GEN_INSTANTIATIONS if (h, c) == (hid, cpad)))

# heads of the generalized kernels: softmax + cross-entropy over classes, or
# squared error over continuous targets (TabularMLPRegressor)
HEAD_CLASSIFIER = "classifier"
HEAD_REGRESSION = "regression"


class Geometry:
    """Padded kernel geometry for an arbitrary (in_features, hidden,
    classes) tabular MLP.

    The HIP kernels run on a zero-padded image of the model: input width
    padded to a multiple of 32 (MFMA K granularity), hidden padded up to
    a compiled instantiation width, classes padded to one or two 16-wide
    MFMA tiles. Zero padding is mathematically exact under Adam-from-zero-init
    (zero init + zero gradient -> zero update), so the padded model's
    real sub-block evolves identically to the unpadded math.

    ``head="regression"`` reads the third number as the count of
    continuous targets (1..32, a single target included); it is kept in
    ``.classes`` so the flat layout is the classifier's. A regression
    geometry never takes the specialized kernels and compares unequal to
    a classifier geometry of the same numbers.
    """

    def __init__(self, in_features: int, hidden: int, classes: int,
                 head: str = HEAD_CLASSIFIER):
        if head not in (HEAD_CLASSIFIER, HEAD_REGRESSION):
            raise ValueError(f"unknown head {head!r}")
        min_out = 1 if head == HEAD_REGRESSION else 2
        if in_features < 1 or hidden < 1 or classes < min_out:
            raise ValueError(f"bad geometry ({in_features}, {hidden}, {classes})")
        if classes > MAX_CLASSES:
            if head == HEAD_REGRESSION:
                raise ValueError(
                    f"targets={classes} unsupported: the fused head spans at most "
                    f"two MFMA tiles ({MAX_CLASSES} targets max)"
                )
            raise ValueError(
                f"classes={classes} unsupported: the fused classifier head spans "
                f"at most two MFMA tiles ({MAX_CLASSES} classes max)"
            )
        if hidden > SUPPORTED_HID[-1]:
            raise ValueError(
                f"hidden={hidden} exceeds the largest compiled width {SUPPORTED_HID[-1]}"
            )
        self.head = head
        self.in_features = in_features
        self.hidden = hidden
        self.classes = classes
        self.inp = (in_features + 31) // 32 * 32
        self.hid = next(h for h in SUPPORTED_HID if h >= hidden)
        self.cpad = 16 if classes <= 16 else 32
        self.off_w1 = 0
        self.off_b1 = self.inp * self.hid
        self.off_w2 = self.off_b1 + self.hid
        self.off_b2 = self.off_w2 + self.hid * self.cpad
        self.nparam = self.off_b2 + self.cpad
        self.slab_stride = (self.nparam + 2 + 15) // 16 * 16
        # packed weight images: W1T [hid][inp] + W2s [hid][32] + W2T [cpad][hid]
        self.wimg_n = self.hid * self.inp + self.hid * 32 + self.cpad * self.hid
        # the hand-tuned specialized kernel path covers exactly this shape
        self.is_specialized = (
            head == HEAD_CLASSIFIER and (in_features, hidden, classes) == (64, 32, 10)
        )

    def __setstate__(self, state):
        state.setdefault("head", HEAD_CLASSIFIER)   # pickles from before the heads
        self.__dict__.update(state)

    def __repr__(self):
        tag = "" if self.head == HEAD_CLASSIFIER else f", head={self.head}"
        return (
            f"Geometry({self.in_features}->{self.hidden}->{self.classes}, "
            f"padded {self.inp}x{self.hid}x{self.cpad}, nparam={self.nparam}{tag})"
        )

    def __eq__(self, other):
        return isinstance(other, Geometry) and (
            (self.in_features, self.hidden, self.classes, self.head)
            == (other.in_features, other.hidden, other.classes, other.head)
        )


DIGITS = Geometry(64, 32, 10)
assert (DIGITS.off_b1, DIGITS.off_w2, DIGITS.off_b2, DIGITS.nparam) == (
    OFF_B1,
    OFF_W2,
    OFF_B2,
    NPARAM,
), "digits geometry must match the specialized kernel's layout"


def standardize_fit(X: torch.Tensor, eps: float = 1e-5) -> Tuple[torch.Tensor, torch.Tensor]:
    """Population column mean / 1/sqrt(var+eps) (fp64 accumulation like
    the kernel)."""
    Xd = X.double()
    mean = Xd.mean(dim=0)
    var = (Xd * Xd).mean(dim=0) - mean * mean
    invstd = 1.0 / torch.sqrt(torch.clamp(var, min=0) + eps)
    return mean.float(), invstd.float()


def standardize_apply(X: torch.Tensor, mean: torch.Tensor, invstd: torch.Tensor) -> torch.Tensor:
    return ((X - mean) * invstd).bfloat16()


def unpack_master(master: torch.Tensor):
    return unpack_master_g(DIGITS, master)


def mlp_step(
    Xbf: torch.Tensor,
    y: torch.Tensor,
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
    grads: torch.Tensor,
    invBtot: float,
) -> None:
    """Fused fwd+bwd reference: accumulates grads (+loss at [NPARAM])
    into ``grads`` exactly like the kernel (which atomically adds onto a
    pre-zeroed buffer)."""
    # NOT mlp_step_g(DIGITS, ...): this oracle feeds the unrounded hidden activations to layer 2
    _, b1, _, b2 = unpack_master(master)
    X = Xbf.float()
    W1 = W1bf.float()
    W2 = W2bf.float()
    Hpre = X @ W1 + b1
    H = torch.relu(Hpre)
    logits = H @ W2 + b2
    logits[:, CLS:] = -1e30
    m = logits.max(dim=1, keepdim=True).values
    e = torch.exp(logits - m)
    e[:, CLS:] = 0
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    B = X.shape[0]
    onehot = torch.zeros_like(p)
    onehot[torch.arange(B, device=X.device), y.long()] = 1.0
    dlogits = (p - onehot) * invBtot
    loss = float(-(torch.log(p[torch.arange(B, device=X.device), y.long()])).sum() * invBtot)

    # bwd — bf16 round-trips where the kernel stores intermediates in LDS bf16
    Hbf = H.bfloat16().float()
    dlogits_bf = dlogits.bfloat16().float()
    dH = dlogits_bf @ W2.T
    dH = dH * (Hbf > 0)
    dH_bf = dH.bfloat16().float()

    dW2 = Hbf.T @ dlogits_bf
    db2 = dlogits_bf.sum(dim=0)
    dW1 = X.T @ dH_bf
    db1 = dH_bf.sum(dim=0)

    grads[OFF_W1 : OFF_W1 + IN * HID] += dW1.reshape(-1)
    grads[OFF_B1 : OFF_B1 + HID] += db1
    grads[OFF_W2 : OFF_W2 + HID * CPAD] += dW2.reshape(-1)
    grads[OFF_B2 : OFF_B2 + CPAD] += db2
    grads[NPARAM] += loss


def mlp_predict(
    X: torch.Tensor,
    mean: torch.Tensor,
    invstd: torch.Tensor,
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
    return_probs: bool = False,
):
    return mlp_predict_g(DIGITS, X, mean, invstd, W1bf, W2bf, master, return_probs)


# ---------------------------------------------------------------------------
# geometry-parametric variants (oracle + CPU path for the generalized
# kernels in tabular_gen.hip; layouts match the padded Geometry exactly)
# ---------------------------------------------------------------------------


def unpack_master_g(g: Geometry, master: torch.Tensor):
    W1 = master[g.off_w1 : g.off_w1 + g.inp * g.hid].view(g.inp, g.hid)
    b1 = master[g.off_b1 : g.off_b1 + g.hid]
    W2 = master[g.off_w2 : g.off_w2 + g.hid * g.cpad].view(g.hid, g.cpad)
    b2 = master[g.off_b2 : g.off_b2 + g.cpad]
    return W1, b1, W2, b2


def mlp_step_g(
    g: Geometry,
    Xbf: torch.Tensor,  # [B][inp] staged bf16 (zero-padded)
    y: torch.Tensor,
    W1bf: torch.Tensor,  # [inp][hid] bf16 mirror
    W2bf: torch.Tensor,  # [hid][cpad] bf16 mirror
    master: torch.Tensor,
    grads: torch.Tensor,
    invBtot: float,
) -> None:
    """Parametric fused fwd+bwd reference: accumulates grads (+loss at
    [g.nparam]) into ``grads`` exactly like mlp_step_gen_kernel."""
    _, b1, _, b2 = unpack_master_g(g, master)
    X = Xbf.float()
    W1 = W1bf.float()
    W2 = W2bf.float()
    Hpre = X @ W1 + b1
    H = torch.relu(Hpre)
    logits = H.bfloat16().float() @ W2 + b2
    logits[:, g.classes :] = -1e30
    m = logits.max(dim=1, keepdim=True).values
    e = torch.exp(logits - m)
    e[:, g.classes :] = 0
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    B = X.shape[0]
    rows = torch.arange(B, device=X.device)
    onehot = torch.zeros_like(p)
    onehot[rows, y.long()] = 1.0
    dlogits = (p - onehot) * invBtot
    loss = float(-(torch.log(p[rows, y.long()])).sum() * invBtot)

    Hbf = H.bfloat16().float()
    dlogits_bf = dlogits.bfloat16().float()
    dH = dlogits_bf @ W2.T
    dH = dH * (Hbf > 0)
    dH_bf = dH.bfloat16().float()

    dW2 = Hbf.T @ dlogits_bf
    db2 = dlogits_bf.sum(dim=0)
    dW1 = X.T @ dH_bf
    db1 = dH_bf.sum(dim=0)

    grads[g.off_w1 : g.off_w1 + g.inp * g.hid] += dW1.reshape(-1)
    grads[g.off_b1 : g.off_b1 + g.hid] += db1
    grads[g.off_w2 : g.off_w2 + g.hid * g.cpad] += dW2.reshape(-1)
    grads[g.off_b2 : g.off_b2 + g.cpad] += db2
    grads[g.nparam] += loss


def mlp_predict_g(
    g: Geometry,
    X: torch.Tensor,  # [B][in_features] raw fp32
    mean: torch.Tensor,
    invstd: torch.Tensor,
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
    return_probs: bool = False,
):
    _, b1, _, b2 = unpack_master_g(g, master)
    Xs = ((X - mean) * invstd).bfloat16().float()
    if g.inp > g.in_features:  # zero-pad to the staged width
        pad = torch.zeros(X.shape[0], g.inp - g.in_features, device=X.device)
        Xs = torch.cat([Xs, pad], dim=1)
    H = torch.relu(Xs @ W1bf.float() + b1)
    logits = H.bfloat16().float() @ W2bf.float() + b2
    logits = logits[:, : g.classes]
    preds = logits.argmax(dim=1).int()
    if return_probs:
        return preds, torch.softmax(logits, dim=1)
    return preds


def mlp_step_reg_g(
    g: Geometry,
    Xbf: torch.Tensor,  # [B][inp] staged bf16 (zero-padded)
    Yt: torch.Tensor,   # [B][cpad] fp32 standardized targets (zero-padded)
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
    grads: torch.Tensor,
    invBtot: float,
) -> None:
    """Squared-error twin of mlp_step_g, mirroring the regression head of
    mlp_step_gen_kernel: loss = 0.5 * invBtot * sum_{b, c < T} (z - y)^2,
    H rounded to bf16 before layer 2, dz and dH rounded for the products
    they feed; db2 sums the unrounded dz as the kernel does."""
    _, b1, _, b2 = unpack_master_g(g, master)
    T = g.classes
    X = Xbf.float()
    W1 = W1bf.float()
    W2 = W2bf.float()
    H = torch.relu(X @ W1 + b1)
    Hbf = H.bfloat16().float()
    z = Hbf @ W2 + b2
    d = torch.zeros_like(z)
    d[:, :T] = z[:, :T] - Yt.float()[:, :T]
    dz = d * invBtot
    loss = float(0.5 * invBtot * (d * d).sum())

    dz_bf = dz.bfloat16().float()
    dH = dz_bf @ W2.T
    dH = dH * (Hbf > 0)
    dH_bf = dH.bfloat16().float()

    dW2 = Hbf.T @ dz_bf
    db2 = dz.sum(dim=0)
    dW1 = X.T @ dH_bf
    db1 = dH_bf.sum(dim=0)

    grads[g.off_w1 : g.off_w1 + g.inp * g.hid] += dW1.reshape(-1)
    grads[g.off_b1 : g.off_b1 + g.hid] += db1
    grads[g.off_w2 : g.off_w2 + g.hid * g.cpad] += dW2.reshape(-1)
    grads[g.off_b2 : g.off_b2 + g.cpad] += db2
    grads[g.nparam] += loss


def mlp_predict_reg_g(
    g: Geometry,
    X: torch.Tensor,  # [B][in_features] raw fp32
    mean: torch.Tensor,
    invstd: torch.Tensor,
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
    y_mean: torch.Tensor,   # [T]
    y_scale: torch.Tensor,  # [T]
) -> torch.Tensor:
    """fp32 [B][T] in original target units: the standardized output
    de-standardized in the epilogue, as mlp_predict_gen_kernel's
    regression head does."""
    _, b1, _, b2 = unpack_master_g(g, master)
    T = g.classes
    Xs = ((X - mean) * invstd).bfloat16().float()
    if g.inp > g.in_features:  # zero-pad to the staged width
        pad = torch.zeros(X.shape[0], g.inp - g.in_features, device=X.device)
        Xs = torch.cat([Xs, pad], dim=1)
    H = torch.relu(Xs @ W1bf.float() + b1)
    z = H.bfloat16().float() @ W2bf.float() + b2
    return z[:, :T] * y_scale + y_mean


# Evaluation record layout (fp32 entries): the copy of EVAL_REC_* in
# hip/tabular_launch.h (tests/test_eval_cpu.py holds the two equal).
# Classifier: [LOSS] mean loss, [CORRECT] the correct count, an int32 stored
# as its bits. Regression: [LOSS], then the mean squared error of column c
# at [FIRST_MSE + c], standardized units, pad columns 0.
EVAL_REC_LOSS = 0
EVAL_REC_CORRECT = 1
EVAL_REC_CLS_N = 2
EVAL_REC_FIRST_MSE = 1


def eval_rec_n(g: Geometry) -> int:
    """Entries of an evaluation record for the geometry's head"""
    return EVAL_REC_FIRST_MSE + g.cpad if g.head == HEAD_REGRESSION else EVAL_REC_CLS_N


def eval_rows_per_wg(g: Geometry) -> int:
    """Rows per workgroup of the evaluation kernel: the RT of the table's
    predict row for the padded (hid, cpad)."""
    return next(r for h, r, c, p in GEN_INSTANTIATIONS if p and (h, c) == (g.hid, g.cpad))


def _eval_logits_g(g: Geometry, Xbf, W1bf, W2bf, master) -> torch.Tensor:
    """fp32 [B][cpad] outputs of the kernels' forward: H rounded to bf16
    before layer 2"""
    _, b1, _, b2 = unpack_master_g(g, master)
    H = torch.relu(Xbf.float() @ W1bf.float() + b1)
    return H.bfloat16().float() @ W2bf.float() + b2


def mlp_eval_g(
    g: Geometry,
    Xbf: torch.Tensor,  # [B][inp] staged bf16 (zero-padded)
    y: torch.Tensor,    # [B] int labels
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
) -> torch.Tensor:
    """Forward-only classifier metrics, mirroring mlp_eval_gen_kernel and
    eval_finish_kernel: one fp32 record [EVAL_REC_CLS_N] holding the mean
    of -log softmax(z)[y] over the B rows and the count of rows with
    argmax == y (int32 bits). A label outside [0, classes) contributes
    exact zeros to both. Row sums are taken in fp64 and rounded once."""
    B = Xbf.shape[0]
    logits = _eval_logits_g(g, Xbf, W1bf, W2bf, master)[:, : g.classes]
    yl = y.long()
    scored = (yl >= 0) & (yl < g.classes)
    safe = torch.where(scored, yl, torch.zeros_like(yl))
    logp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
    row_loss = torch.where(scored, -logp.gather(1, safe[:, None])[:, 0],
                           torch.zeros(B))
    correct = int(((logits.argmax(dim=1) == yl) & scored).sum())
    rec = torch.zeros(EVAL_REC_CLS_N, dtype=torch.float32)
    rec[EVAL_REC_LOSS] = float(row_loss.double().sum() / B)
    rec.view(torch.int32)[EVAL_REC_CORRECT] = correct
    return rec


def mlp_eval_reg_g(
    g: Geometry,
    Xbf: torch.Tensor,  # [B][inp] staged bf16 (zero-padded)
    Yt: torch.Tensor,   # [B][cpad] fp32 standardized targets
    W1bf: torch.Tensor,
    W2bf: torch.Tensor,
    master: torch.Tensor,
) -> torch.Tensor:
    """Forward-only regression metrics: one fp32 record
    [EVAL_REC_FIRST_MSE + cpad] holding the mean of 0.5 * sum_{c<T} (z-y)^2
    and each column's mean squared error in standardized units. Only the
    real targets are read: a pad column of Yt can leak nothing."""
    B, T = Xbf.shape[0], g.classes
    z = _eval_logits_g(g, Xbf, W1bf, W2bf, master)
    d = z[:, :T] - Yt.float()[:, :T]
    sq = (d * d).double()
    rec = torch.zeros(EVAL_REC_FIRST_MSE + g.cpad, dtype=torch.float32)
    rec[EVAL_REC_LOSS] = float(0.5 * sq.sum() / B)
    rec[EVAL_REC_FIRST_MSE : EVAL_REC_FIRST_MSE + T] = (sq.sum(dim=0) / B).float()
    return rec


def adam_step_g(
    g: Geometry,
    master: torch.Tensor,
    bfmirror: torch.Tensor,
    grads: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    t: int,
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
) -> None:
    gr = grads[: g.nparam]
    m.mul_(beta1).add_(gr, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(gr, gr, value=1 - beta2)
    corr1 = 1.0 / (1.0 - beta1**t)
    corr2 = 1.0 / (1.0 - beta2**t)
    master[: g.nparam] -= lr * (m * corr1) / (torch.sqrt(v * corr2) + eps)
    bfmirror[: g.nparam] = master[: g.nparam].bfloat16()


def adam_step(
    master: torch.Tensor,
    bfmirror: torch.Tensor,
    grads: torch.Tensor,
    m: torch.Tensor,
    v: torch.Tensor,
    t: int,
    lr: float,
    beta1: float = 0.9,
    beta2: float = 0.999,
    eps: float = 1e-8,
) -> None:
    adam_step_g(DIGITS, master, bfmirror, grads, m, v, t, lr, beta1, beta2, eps)


# ---------------------------------------------------------------------------
# shuffled epochs: the keyed permutation of [0, N) (hip/tabular_shuffle.h holds
# the device copy; tests hold the two equal)
# ---------------------------------------------------------------------------

SHUFFLE_ROUNDS = 6
SHUFFLE_GOLDEN = 0x9E3779B9
_M32 = 0xFFFFFFFF


def _fmix32(h):
    """murmur3's 32-bit finalizer on an int, or elementwise on an int64
    tensor of values below 2**32 (int64 products wrap mod 2**64, the low 32
    bits are the uint32 product)."""
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    return h ^ (h >> 16)


def shuffle_half_bits(n: int) -> int:
    """Half the bit width of the Feistel domain that covers [0, n):
    max(1, ceil(ceil(log2 n) / 2)), so the domain 4**half is in [n, 4n)
    (n = 1: the smallest domain, 4)."""
    return max(1, ((n - 1).bit_length() + 1) // 2)


def shuffle_round_keys(seed: int, t: int) -> Tuple[int, ...]:
    """rk_r = fmix32(seed ^ fmix32(t ^ (GOLDEN * (r + 1) mod 2**32)))."""
    seed, t = seed & _M32, t & _M32
    return tuple(
        _fmix32(seed ^ _fmix32(t ^ ((SHUFFLE_GOLDEN * (r + 1)) & _M32)))
        for r in range(SHUFFLE_ROUNDS)
    )


def _shuffle_feistel(x: torch.Tensor, half: int, keys) -> torch.Tensor:
    mask = (1 << half) - 1
    L, R = x >> half, x & mask
    for rk in keys:
        L, R = R, L ^ (_fmix32(R ^ rk) & mask)
    return (L << half) | R


def shuffle_perm(n: int, seed: int, t: int) -> torch.Tensor:
    """src[i] = P(i; n, seed, t) for every i in [0, n): a bijection of
    [0, n), int64 on the CPU. A balanced 6-round Feistel network over
    2 * half bits, cycle-walked into [0, n): integer-only, stateless, the
    function the shuffle kernel evaluates per row. ``t`` is the Adam step
    counter at the start of the epoch; it and ``seed`` are taken mod 2**32.

    The walk ends: the network is a bijection of its domain and the start
    is below n, so the start's cycle comes back below n after at most
    domain - n + 1 applications."""
    if not 1 <= n <= 2**31 - 1:
        raise ValueError(f"shuffle_perm needs 1 <= n <= INT_MAX, is {n}")
    half, keys = shuffle_half_bits(n), shuffle_round_keys(seed, t)
    x = _shuffle_feistel(torch.arange(n, dtype=torch.int64), half, keys)
    while True:
        out = (x >= n).nonzero().squeeze(1)
        if not out.numel():
            return x
        x[out] = _shuffle_feistel(x[out], half, keys)
