"""TabularMLP — the framework's default tabular hot path, for ANY
(in_features, hidden, classes) geometry.

A one-hidden-layer classifier (Linear -> ReLU -> Linear -> Softmax)
whose training step (standardize, fused forward, cross-entropy
backward, fused Adam) runs as hand-written CDNA4 HIP kernels on MFMA:

* the hand-tuned specialized kernels for the 64->32->10 digits shape
  (unionml_amd/ops/hip/tabular_kernels.hip — the headline benchmark
  path, with the persistent and packed-weight-image engines), and
* the generalized templated kernels for every other shape
  (unionml_amd/ops/hip/tabular_gen.hip — input width streamed through
  LDS in k-tiles, hidden width dispatched over compiled instantiations
  {32,64,128,256}, odd sizes zero-padded exactly).

The per-epoch minibatch loop is captured ONCE into a hipGraph and
replayed per epoch — zero launch overhead in steady state. On CPU the
same class runs the pure-torch reference path
(unionml_amd/ops/reference.py): one user-visible code path, two
substrates.

TabularMLPRegressor (bottom of this module) is the same machinery with a
squared-error head over 1..32 continuous targets.

Data parallel: under an active torch.distributed process group each
rank trains its row shard and the flat gradient buffer is all-reduced
on RCCL between the reduce-only step and the Adam kernel.

Reference behavior mirrored (no code ported — the reference is pure
Python): tests/integration/pytorch_app/quickstart.py:14-70.
"""

import math
from typing import Dict, Optional

import torch

from unionml_amd._logging import logger
from unionml_amd.ops import hip_ext
from unionml_amd.ops import reference as ref
from unionml_amd.ops.reference import (
    CPAD, HEAD_CLASSIFIER, HEAD_REGRESSION, HID, IN, Geometry,
)

ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def split_validation(n: int, fraction: float, seed: int = 0):
    """(train_idx, val_idx): a seeded random split of ``n`` rows that holds
    out ``round(n * fraction)`` of them (at least one, at most n - 1), as
    the app trainers' ``validation_fraction`` does it. CPU int64 tensors."""
    if not 0.0 < fraction < 1.0:
        raise ValueError(f"validation_fraction must be in (0, 1), is {fraction}")
    if n < 2:
        raise ValueError("validation_fraction needs at least two rows")
    n_val = min(max(int(round(n * fraction)), 1), n - 1)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(seed))
    return perm[n_val:].sort().values, perm[:n_val].sort().values


class TabularMLP:
    """Device-resident parameter/optimizer state + fused train/predict."""

    #: the head the fused kernels end in; TabularMLPRegressor overrides it
    HEAD = HEAD_CLASSIFIER

    def __init__(
        self,
        in_features: int = 64,
        hidden: int = 32,
        classes: int = 10,
        device: Optional[str] = None,
        seed: int = 0,
    ):
        self.g = Geometry(in_features, hidden, classes, head=self.HEAD)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self.use_hip = self.device.type == "cuda"
        if self.use_hip:
            hip_ext(required=True)  # loud failure if the gfx950 ext is missing
        # hand-tuned specialized kernels for the digits shape; generalized
        # templated kernels for everything else
        self.use_spec = self.g.is_specialized

        g = self.g
        gen_t = torch.Generator().manual_seed(seed)
        master = torch.zeros(g.nparam, dtype=torch.float32)
        W1, b1, W2, b2 = ref.unpack_master_g(g, master)
        W1[: g.in_features, : g.hidden] = (
            torch.randn(g.in_features, g.hidden, generator=gen_t)
            * math.sqrt(2.0 / g.in_features)
        )
        W2[: g.hidden, : g.classes] = (
            torch.randn(g.hidden, g.classes, generator=gen_t) * math.sqrt(2.0 / g.hidden)
        )

        self.master = master.to(self.device)
        self.bfmirror = self.master.bfloat16()
        self.m = torch.zeros_like(self.master)
        self.v = torch.zeros_like(self.master)
        self.t_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.grads = torch.zeros(g.nparam + 1, dtype=torch.float32, device=self.device)
        self.mean = torch.zeros(g.in_features, dtype=torch.float32, device=self.device)
        self.invstd = torch.ones(g.in_features, dtype=torch.float32, device=self.device)
        self.slabs = None       # per-WG partial-grad slabs for the fused step
        self.counter = None     # G16 epoch counter (shared by both step modes)
        self._graph = None
        self._graph_key = None
        # evaluation: per-workgroup partial rows, the single-record history
        # evaluate() reads, and (digits shape only) the generalized-layout
        # weight image the evaluation kernel reads; built on first use
        self._eval_part = None
        self._eval_one = None
        self._eval_wimg = None
        self._val_buf = None
        # shuffled epochs: the destination buffers (Xs, ys) the shuffle
        # launch gathers the staged rows into; built on first use
        self._shuf = None
        #: one evaluation record per epoch of the last
        #: train_epochs(validation=...), a CPU tensor [epochs run][record]
        self.val_history = None
        self._val_n = 0
        # packed weight images (kernel-layout staging) so the training
        # prologue is a straight vectorized copy; kept in sync by the
        # Adam kernels (wimg=) and rebuilt on any host-side weight
        # mutation. Specialized and generalized kernels use different
        # packings (LDS-stride padded vs dense row-major).
        self.wimg = (
            torch.zeros(self._wimg_len(), dtype=torch.bfloat16, device=self.device)
            if self.use_hip
            else None
        )
        self._build_wimg()

    def _wimg_len(self) -> int:
        # the specialized layout's numbers come from the extension
        # (tabular_launch.h); the image exists only when it is loaded
        return hip_ext().WIMG_N if self.use_spec else self.g.wimg_n

    def _rows_per_wg(self, batch: Optional[int] = None) -> int:
        if self.use_spec:
            return 128
        # the default rows/WG and the small-batch one: the largest and the
        # smallest the step kernel is compiled at for this (hid, cpad)
        # (reference.GEN_INSTANTIATIONS; one and the same where only one
        # is). The small variant keeps >= ~16 workgroups in flight at
        # modest batch sizes — the fwd/bwd phase is bandwidth-bound and
        # achievable bandwidth scales with resident CUs.
        rts = ref.compiled_rts(self.g.hid, self.g.cpad)
        big, small = rts[-1], rts[0]
        # smaller rows/WG doubles the grid (the bandwidth-bound fwd/bwd
        # scales with resident CUs: measured -12% at B=2048, -11% at
        # B=4096 on the MNIST shape) — but every extra WG re-reads the
        # whole W1 image and adds a full-nparam gradient slab, which
        # turns pathological past ~128 WGs (B=8192: 335 vs 65 us).
        if batch is not None and (batch + small - 1) // small <= 128:
            return small
        return big

    def _build_wimg(self):
        if self.wimg is None:
            return
        g = self.g
        W1, _, W2, _ = ref.unpack_master_g(g, self.master.detach().cpu())
        if self.use_spec:
            ext = hip_ext()
            XS, WS = ext.XS, ext.WS
            img = torch.zeros(ext.WIMG_N, dtype=torch.bfloat16)
            img[: HID * XS].view(HID, XS)[:, :IN] = W1.t().bfloat16()      # W1T[h][k]
            img[HID * XS : HID * XS + HID * WS].view(HID, WS)[:, :CPAD] = W2.bfloat16()
            img[HID * XS + HID * WS :].view(CPAD, WS)[:, :HID] = W2.t().bfloat16()
        else:
            img = torch.zeros(g.wimg_n, dtype=torch.bfloat16)
            o1 = g.hid * g.inp
            o2 = o1 + g.hid * 32
            img[:o1].view(g.hid, g.inp).copy_(W1.t().bfloat16())           # W1T[h][k]
            img[o1:o2].view(g.hid, 32)[:, : g.cpad] = W2.bfloat16()        # W2s K-pad
            img[o2:].view(g.cpad, g.hid).copy_(W2.t().bfloat16())          # W2T[c][h]
        self.wimg.copy_(img.to(self.device))

    def _ensure_slabs(self, n_wg: int):
        if self.slabs is None or self.slabs.shape[0] < n_wg:
            self.slabs = torch.zeros(
                n_wg, self.g.slab_stride, dtype=torch.float32, device=self.device
            )
            self.counter = torch.zeros(1, dtype=torch.uint32, device=self.device)
            # a captured epoch holds the old slabs' and counter's addresses
            self._graph = self._graph_key = None

    # -- views ----------------------------------------------------------------

    @property
    def W1bf(self) -> torch.Tensor:
        g = self.g
        return self.bfmirror[g.off_w1 : g.off_w1 + g.inp * g.hid].view(g.inp, g.hid)

    @property
    def W2bf(self) -> torch.Tensor:
        g = self.g
        return self.bfmirror[g.off_w2 : g.off_w2 + g.hid * g.cpad].view(g.hid, g.cpad)

    # -- standardizer ----------------------------------------------------------

    def fit_standardizer(self, X: torch.Tensor, eps: float = 1e-5):
        X = X.to(self.device, torch.float32).contiguous()
        if self.use_hip:
            hip_ext().standardize_fit(X, self.mean, self.invstd, eps)
        else:
            mean, invstd = ref.standardize_fit(X, eps)
            self.mean.copy_(mean)
            self.invstd.copy_(invstd)

    def stage(self, X: torch.Tensor) -> torch.Tensor:
        """Standardize fp32 features into a device-resident bf16 matrix,
        zero-padded to the kernel's input width."""
        g = self.g
        X = X.to(self.device, torch.float32).contiguous()
        if self.use_hip:
            if g.inp == g.in_features:
                out = torch.empty(X.shape[0], g.inp, dtype=torch.bfloat16, device=self.device)
            else:
                out = torch.zeros(X.shape[0], g.inp, dtype=torch.bfloat16, device=self.device)
            if X.shape[0]:
                hip_ext().standardize_apply(X, self.mean, self.invstd, out)
            return out
        out_raw = ref.standardize_apply(X, self.mean, self.invstd)
        if g.inp == g.in_features:
            return out_raw
        out = torch.zeros(X.shape[0], g.inp, dtype=torch.bfloat16)
        out[:, : g.in_features] = out_raw
        return out

    # -- training --------------------------------------------------------------

    def _launch_step(self, Xbf, y, invBtot, lr, loss_out, grads_out=None):
        """One step's launches: a single fused launch for the specialized
        shape; for generalized shapes the slab-producing step kernel
        followed by the wide-grid reduce+Adam kernel (the kernel
        boundary is the inter-WG barrier — full-chip bandwidth for the
        large-nparam reduction instead of a handshake inside a tiny
        grid). With ``grads_out`` the launches stop after the slab
        reduction and write the summed grads (+loss) there: no Adam."""
        g = self.g
        rpw = self._rows_per_wg(Xbf.shape[0])
        n_wg = (Xbf.shape[0] + rpw - 1) // rpw
        self._ensure_slabs(n_wg)
        ext = hip_ext()
        if self.use_spec:
            ok = ext.mlp_step_fused(
                Xbf, y, self.W1bf, self.W2bf, self.master, self.bfmirror,
                self.m, self.v, self.t_dev, self.slabs, self.counter, loss_out,
                invBtot, lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
                grads_out=grads_out, wimg=self.wimg,
            )
            assert ok, "fused step slab capacity exceeded"
        else:
            ok = self._gen_step_kernel(ext, Xbf, y, rpw, invBtot)
            assert ok, "fused step slab capacity exceeded"
            ext.reduce_adam_gen(
                self.slabs, n_wg, g.inp, g.hid, g.cpad, self.master,
                self.bfmirror, self.m, self.v, self.t_dev, self.counter,
                loss_out, lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
                wimg=self.wimg, grads_out=grads_out,
            )

    def _gen_step_kernel(self, ext, Xbf, y, rpw: int, invBtot: float) -> bool:
        """The generalized family's slab-producing step kernel, by head."""
        g = self.g
        return ext.mlp_step_gen(
            Xbf, y, g.hid, g.classes, rpw, self.wimg, self.master,
            self.slabs, invBtot,
        )

    def _ref_step(self, Xbf, y, invBtot: float):
        """The CPU path's step (torch reference), by head."""
        ref.mlp_step_g(
            self.g, Xbf, y, self.W1bf, self.W2bf, self.master, self.grads, invBtot
        )

    def _prep_targets(self, y: torch.Tensor) -> torch.Tensor:
        """Targets as the step kernels read them: int32 class labels."""
        return y.to(self.device, torch.int32).contiguous()

    def _step_reduce(self, Xbf: torch.Tensor, y: torch.Tensor, invBtot: float, lr: float):
        """Reduce-only step: summed grads (+loss) into self.grads — the
        DP pre-collective kernel, no Adam."""
        g = self.g
        self._launch_step(Xbf, y, invBtot, lr, self.grads[g.nparam : g.nparam + 1], self.grads)

    def _adam(self, lr: float):
        g = self.g
        ext = hip_ext()
        if self.use_spec:
            ext.adam_step(
                self.master, self.bfmirror, self.grads, self.m, self.v, self.t_dev,
                lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, wimg=self.wimg,
            )
        else:
            ext.adam_step_gen(
                self.master, self.bfmirror, self.grads, self.m, self.v, self.t_dev,
                g.inp, g.hid, g.cpad, lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
                wimg=self.wimg,
            )

    def _step(self, Xbf: torch.Tensor, y: torch.Tensor, invBtot: float, lr: float,
              allreduce: bool):
        g = self.g
        if self.use_hip:
            self._step_reduce(Xbf, y, invBtot, lr)
        else:
            self.grads.zero_()
            self._ref_step(Xbf, y, invBtot)
        if allreduce:
            import torch.distributed as dist

            dist.all_reduce(self.grads)
        if self.use_hip:
            self._adam(lr)
        else:
            self.t_dev += 1
            ref.adam_step_g(
                g, self.master, self.bfmirror, self.grads, self.m, self.v,
                int(self.t_dev.item()), lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
            )
        return self.grads[g.nparam]

    def _fused_adam_step(self, Xbf, y, invBtot, lr, loss_out):
        """One optimizer step (fwd/bwd + slab reduction + Adam), the
        last loss into ``loss_out``."""
        self._launch_step(Xbf, y, invBtot, lr, loss_out)

    # -- shuffled epochs -------------------------------------------------------

    def _ensure_shuffle(self, Xbf, y):
        """The destination buffers of a shuffled epoch, shaped like the
        staged inputs."""
        buf = self._shuf
        if buf is None or any(
            (b.shape, b.dtype, b.device) != (t.shape, t.dtype, t.device)
            for b, t in zip(buf, (Xbf, y))
        ):
            self._shuf = (torch.empty_like(Xbf), torch.empty_like(y))
            # a captured epoch holds the old buffers' addresses
            self._graph = self._graph_key = None
        return self._shuf

    def _shuffle_kernel(self, ext, Xbf, y, Xs, ys, seed: int):
        """The shuffle launch, by head."""
        ext.shuffle_rows(Xbf, y, Xs, ys, self.t_dev, seed)

    def _shuffled(self, Xbf, y, seed: int):
        """This epoch's rows: the staged originals gathered by the keyed
        permutation P(.; N, seed, t_dev) (reference.shuffle_perm). On the
        device one launch into the model's buffers, which reads t_dev when
        it runs, so a replayed epoch re-keys itself; on the CPU the
        reference permutation."""
        if self.use_hip:
            Xs, ys = self._shuf
            self._shuffle_kernel(hip_ext(), Xbf, y, Xs, ys, seed)
            return Xs, ys
        perm = ref.shuffle_perm(Xbf.shape[0], seed, int(self.t_dev.item()))
        return Xbf[perm], y[perm]

    def _shuffle_key(self, seed: int):
        """What a captured shuffled epoch bakes in besides the sources'
        addresses (already in the key): the flag, the seed, the buffers."""
        return ("shuffle", seed) + tuple(b.data_ptr() for b in self._shuf)

    def _run_epochs(self, run_epoch, epochs: int, key, use_graph: bool,
                    after_epoch=None) -> float:
        """Device epoch driver: one eager warmup epoch (also warms the
        RCCL communicator / memory pool), then capture one epoch into a
        hipGraph once per ``key`` (capture records without executing)
        and replay the remaining epochs — or step them eagerly when
        ``use_graph`` is off or capture fails. Returns the last loss,
        which both step flavours leave in grads[nparam]. ``after_epoch(e)``
        (validation with patience or restore_best only) runs on the host
        after epoch ``e`` and returns True to stop."""
        run_epoch()
        remaining = epochs - 1
        if after_epoch is not None and after_epoch(0):
            remaining = 0
        if use_graph and self._graph_key != key:
            try:
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph):
                    run_epoch()
                self._graph, self._graph_key = gph, key
            except RuntimeError as exc:  # e.g. RCCL capture unsupported
                logger.warning("hipGraph capture failed (%s); eager stepping", exc)
                self._graph, self._graph_key = None, None
        replay = self._graph.replay if use_graph and self._graph is not None else run_epoch
        for e in range(remaining):
            replay()
            if after_epoch is not None and after_epoch(e + 1):
                break
        torch.cuda.synchronize(self.device)
        return float(self.grads[self.g.nparam].item())

    def _train_epochs_fused(self, Xbf, y, batches, *, epochs, lr, use_graph,
                            val=None, shuffle_seed=None) -> float:
        g = self.g
        self._ensure_slabs(
            max(
                (bs + self._rows_per_wg(bs) - 1) // self._rows_per_wg(bs)
                for _, bs in batches
            )
        )
        loss_out = self.grads[g.nparam : g.nparam + 1]

        def run_epoch():
            Xe, ye = (Xbf, y) if shuffle_seed is None else self._shuffled(
                Xbf, y, shuffle_seed)
            for off, bs in batches:
                self._fused_adam_step(
                    Xe[off : off + bs], ye[off : off + bs], 1.0 / bs, lr, loss_out
                )
            if val is not None:
                # same stream, after the epoch's last step: still one chain
                self._eval_launch(val.X, val.y, val.hist, val.slot)

        # the capture bakes in every batch's offset, row count and 1/bs:
        # the key is the batch list itself, not its length
        key = ("fused", tuple(batches), lr, Xbf.data_ptr(), y.data_ptr())
        if shuffle_seed is not None:
            key += self._shuffle_key(shuffle_seed)
        if val is None:
            return self._run_epochs(run_epoch, epochs, key, use_graph)
        # ... and the validation rows, the history (its row count is the
        # finish kernel's cap) and the slot
        key += ("val", val.X.data_ptr(), val.y.data_ptr(), val.X.shape[0],
                val.hist.data_ptr(), val.hist.shape[0], val.slot.data_ptr())
        return self._run_epochs(run_epoch, epochs, key, use_graph,
                                after_epoch=val.after_epoch if val.on_host else None)

    def train_epochs(
        self,
        Xbf: torch.Tensor,
        y: torch.Tensor,
        *,
        epochs: int = 10,
        batch_size: int = 512,
        lr: float = 1e-3,
        use_graph: bool = True,
        world_size: int = 1,
        engine: str = "auto",
        validation=None,
        patience: Optional[int] = None,
        min_delta: float = 0.0,
        restore_best: bool = False,
        shuffle: bool = False,
        shuffle_seed: int = 0,
    ) -> float:
        """Minibatch Adam training over the staged (bf16) features.

        Returns the last step's loss. ``world_size > 1`` means this rank
        holds a shard and gradients all-reduce over RCCL each step.

        ``validation=(Xv, yv)`` (staged like ``Xbf`` and ``y``) ends every
        epoch in a device-side evaluation of those rows, inside the
        captured epoch when ``use_graph`` is on; ``val_history`` then
        holds one record per epoch. ``patience`` stops when the validation
        loss has not improved by more than ``min_delta`` for that many
        epochs, ``restore_best`` puts back the weights and optimizer state
        of the best epoch; either costs one host sync per epoch.

        ``shuffle=True`` trains every epoch on a fresh permutation of the
        rows: one device launch at the head of the epoch gathers ``Xbf`` and
        ``y`` into buffers the model owns, inside the captured epoch. The
        order is ``reference.shuffle_perm(N, shuffle_seed, t)`` with ``t``
        the Adam step counter at the start of the epoch, so it depends on
        nothing but the row count, the seed and the checkpointed counter:
        a resumed run continues the same sequence of orders. Validation
        rows are never shuffled.
        """
        g = self.g
        if shuffle:
            if engine == "persistent":
                raise ValueError(
                    "shuffle is not supported by engine='persistent': the "
                    "persistent kernel runs all epochs in one launch"
                )
            if world_size > 1:
                raise ValueError(
                    "shuffle is not supported under data parallel (world_size > 1)"
                )
            if not 0 <= shuffle_seed < 2**32:
                raise ValueError(
                    f"shuffle_seed must be in [0, 2**32), is {shuffle_seed}"
                )
        y = self._prep_targets(y)
        val = None
        if validation is None:
            if patience is not None or restore_best:
                raise ValueError("patience and restore_best need validation=(Xv, yv)")
        else:
            if world_size > 1:
                raise ValueError(
                    "validation is not supported under data parallel (world_size > 1)"
                )
            if engine == "persistent":
                raise ValueError(
                    "validation is not supported by engine='persistent': the "
                    "persistent kernel runs all epochs in one launch"
                )
            if patience is not None and patience < 1:
                raise ValueError(f"patience must be >= 1, is {patience}")
            val = _Validation(self, validation, epochs, patience, min_delta, restore_best)
        n = Xbf.shape[0]
        batches = [
            (off, min(batch_size, n - off)) for off in range(0, n, batch_size)
        ]
        allreduce = world_size > 1
        seed = int(shuffle_seed) if shuffle and n else None
        if seed is not None and self.use_hip:
            self._ensure_shuffle(Xbf, y)

        # single-GPU flagship: the fully-fused step kernel (fwd+bwd +
        # cross-WG slab reduction + Adam in ONE launch), with the epoch's
        # minibatch loop captured into a hipGraph.
        if self.use_hip and not allreduce:
            if (
                self.use_spec
                and engine == "persistent"
                and batch_size % 128 == 0
                and n % batch_size == 0
            ):
                loss_out = self.grads[g.nparam : g.nparam + 1]
                n_steps = epochs * (n // batch_size)
                ok = hip_ext().mlp_train_steps(
                    Xbf, y, batch_size, n_steps, self.master, self.bfmirror,
                    self.m, self.v, self.t_dev, loss_out,
                    lr, ADAM_BETA1, ADAM_BETA2, ADAM_EPS,
                )
                if ok:
                    torch.cuda.synchronize(self.device)
                    # the persistent kernel updates master/bfmirror but not
                    # the packed weight images; refresh them so a later
                    # fused/adam step (wimg=) doesn't load stale weights
                    self._build_wimg()
                    return float(loss_out.item())
            if val is None:
                return self._train_epochs_fused(
                    Xbf, y, batches, epochs=epochs, lr=lr, use_graph=use_graph,
                    shuffle_seed=seed,
                )
            loss = self._train_epochs_fused(
                Xbf, y, batches, epochs=epochs, lr=lr, use_graph=use_graph, val=val,
                shuffle_seed=seed,
            )
            val.finish()
            return loss

        def run_epoch():
            last = None
            Xe, ye = (Xbf, y) if seed is None else self._shuffled(Xbf, y, seed)
            for off, bs in batches:
                last = self._step(
                    Xe[off : off + bs],
                    ye[off : off + bs],
                    1.0 / (bs * world_size),
                    lr,
                    allreduce,
                )
            return last

        if not (self.use_hip and use_graph):
            loss = None
            for e in range(epochs):
                loss = run_epoch()
                if val is not None and val.after_epoch_ref(e):
                    break
            if val is not None:
                val.finish()
            # with allreduce the stored loss is already the global mean
            return float(loss.item()) if loss is not None else float("nan")

        key = (n, batch_size, world_size, lr, Xbf.data_ptr(), y.data_ptr())
        if seed is not None:
            key += self._shuffle_key(seed)
        return self._run_epochs(run_epoch, epochs, key, use_graph=True)

    # -- evaluation ------------------------------------------------------------

    def _rec_layout(self):
        """Where the evaluation record's entries are: the extension's
        constants on the GPU, reference.py's copy on the CPU."""
        return hip_ext() if self.use_hip else ref

    def _eval_rec_n(self) -> int:
        return self._rec_layout().EVAL_REC_CLS_N

    def _ensure_eval(self, n_rows: int):
        """Device buffers of an evaluation over ``n_rows`` rows."""
        g = self.g
        rt = hip_ext().eval_rows_per_wg(g.hid, g.cpad)
        n_wg = (n_rows + rt - 1) // rt
        if self._eval_part is None or self._eval_part.shape[0] < n_wg:
            self._eval_part = torch.zeros(
                n_wg, self._eval_rec_n(), dtype=torch.float32, device=self.device
            )
            # a captured epoch holds the old buffer's address
            self._graph = self._graph_key = None
        if self._eval_one is None:
            self._eval_one = (
                torch.zeros(1, self._eval_rec_n(), dtype=torch.float32, device=self.device),
                torch.zeros(1, dtype=torch.int32, device=self.device),
            )
        if self.use_spec and self._eval_wimg is None:
            self._eval_wimg = torch.zeros(g.wimg_n, dtype=torch.bfloat16, device=self.device)
            self._graph = self._graph_key = None

    def _refresh_eval_wimg(self):
        """Digits shape: the specialized kernels keep their own image
        layout, the evaluation kernel is the generalized <32,128,16> one.
        Rebuild its image (the packing of _build_wimg's generalized branch)
        from bfmirror with device ops, capturable, before each evaluation."""
        g = self.g
        img = self._eval_wimg
        o1 = g.hid * g.inp
        o2 = o1 + g.hid * 32
        img[:o1].view(g.hid, g.inp).copy_(self.W1bf.t())               # W1T[h][k]
        img[o1:o2].view(g.hid, 32)[:, : g.cpad].copy_(self.W2bf)       # W2s K-pad
        img[o2:].view(g.cpad, g.hid).copy_(self.W2bf.t())              # W2T[c][h]

    def _eval_launch(self, Xbf, y, hist, slot):
        """The evaluation's two launches (metrics, then finish) on the
        current stream: one record into hist[min(slot, cap-1)], slot + 1."""
        wimg = self.wimg
        if self.use_spec:
            self._refresh_eval_wimg()
            wimg = self._eval_wimg
        self._eval_kernel(hip_ext(), Xbf, y, wimg, hist, slot)

    def _eval_kernel(self, ext, Xbf, y, wimg, hist, slot):
        """The generalized family's evaluation kernel, by head."""
        g = self.g
        ext.mlp_eval_gen(
            Xbf, y, g.hid, g.classes, wimg, self.master, self._eval_part, hist, slot
        )

    def _ref_eval(self, Xbf, y) -> torch.Tensor:
        """The CPU path's evaluation record (torch reference), by head."""
        return ref.mlp_eval_g(self.g, Xbf, y, self.W1bf, self.W2bf, self.master)

    def _eval_record(self, Xbf, y) -> torch.Tensor:
        """One evaluation record of the staged rows, on the CPU."""
        if not self.use_hip:
            return self._ref_eval(Xbf, y)
        self._ensure_eval(Xbf.shape[0])
        hist, slot = self._eval_one
        slot.zero_()
        self._eval_launch(Xbf, y, hist, slot)
        return hist[0].cpu()

    def _decode_record(self, rec: torch.Tensor, n: int) -> dict:
        L = self._rec_layout()
        correct = int(rec.view(torch.int32)[L.EVAL_REC_CORRECT])
        return {"loss": float(rec[L.EVAL_REC_LOSS]), "accuracy": correct / n, "n": n}

    def _empty_metrics(self) -> dict:
        return {"loss": float("nan"), "accuracy": float("nan"), "n": 0}

    def _eval_inputs(self, Xbf, y):
        Xbf = Xbf.to(self.device).contiguous()
        y = self._prep_targets(y)
        if Xbf.dim() != 2 or Xbf.shape[1] != self.g.inp or Xbf.dtype != torch.bfloat16:
            raise ValueError(
                f"Xbf must be the staged bf16 [N][{self.g.inp}] features (stage), "
                f"got {Xbf.dtype} {tuple(Xbf.shape)}"
            )
        if y.shape[0] != Xbf.shape[0]:
            raise ValueError(f"{Xbf.shape[0]} rows but {y.shape[0]} targets")
        return Xbf, y

    def evaluate(self, Xbf: torch.Tensor, y: torch.Tensor) -> dict:
        """Mean cross-entropy and accuracy of the staged rows (``stage``),
        computed on the device by the fused evaluation kernel:
        ``{"loss", "accuracy", "n"}``. A label outside ``[0, classes)``
        counts as a row that is neither scored nor correct. An empty input
        gives ``n = 0`` and NaN metrics."""
        Xbf, y = self._eval_inputs(Xbf, y)
        n = Xbf.shape[0]
        if not n:
            return self._empty_metrics()
        return self._decode_record(self._eval_record(Xbf, y), n)

    def evaluate_raw(self, X: torch.Tensor, y: torch.Tensor) -> dict:
        """``evaluate`` of raw fp32 features: stages them first."""
        return self.evaluate(self.stage(torch.as_tensor(X)), torch.as_tensor(y))

    def val_metrics(self):
        """``val_history`` as a list of dicts, one per epoch."""
        if self.val_history is None:
            return []
        return [self._decode_record(r, self._val_n) for r in self.val_history]

    # -- inference -------------------------------------------------------------

    def predict(self, X: torch.Tensor, return_probs: bool = False):
        g = self.g
        X = X.to(self.device, torch.float32).contiguous()
        if self.use_hip:
            preds = torch.empty(X.shape[0], dtype=torch.int32, device=self.device)
            probs = (
                torch.empty(X.shape[0], g.classes, dtype=torch.float32, device=self.device)
                if return_probs
                else None
            )
            if not X.shape[0]:   # the bindings take B >= 1: nothing to launch
                pass
            elif self.use_spec:
                hip_ext().mlp_predict(
                    X, self.mean, self.invstd, self.W1bf, self.W2bf, self.master,
                    preds, probs,
                )
            else:
                hip_ext().mlp_predict_gen(
                    X, g.inp, g.hid, g.classes, self.mean, self.invstd, self.wimg,
                    self.master, preds, probs,
                )
            return (preds, probs) if return_probs else preds
        return ref.mlp_predict_g(
            g, X, self.mean, self.invstd, self.W1bf, self.W2bf, self.master, return_probs
        )

    # -- persistence -----------------------------------------------------------

    def __getstate__(self):
        """Pickle CPU-portably: device caches (slabs, graphs) are
        rebuilt lazily; tensors travel as CPU copies. This is what lets
        a GPU-trained classifier cross the backend's process boundary
        and load on any machine."""
        d = dict(self.__dict__)
        d["slabs"] = d["counter"] = None
        d["_graph"] = d["_graph_key"] = None
        d["_eval_part"] = d["_eval_one"] = d["_eval_wimg"] = d["_val_buf"] = None
        d["_shuf"] = None
        d["wimg"] = None
        d["device"] = str(self.device)
        for k, v in list(d.items()):
            if torch.is_tensor(v):
                d[k] = v.detach().cpu()
        return d

    def __setstate__(self, state):
        device = torch.device(state.pop("device"))
        if device.type == "cuda" and not torch.cuda.is_available():
            device = torch.device("cpu")
        state.setdefault("g", Geometry(64, 32, 10))       # pre-geometry pickles
        state.setdefault("use_spec", state["g"].is_specialized)
        for k in ("_eval_part", "_eval_one", "_eval_wimg", "_val_buf", "val_history"):
            state.setdefault(k, None)                     # pre-evaluation pickles
        state.setdefault("_val_n", 0)
        state.setdefault("_shuf", None)                   # pre-shuffle pickles
        self.__dict__.update(state)
        self.device = device
        self.use_hip = device.type == "cuda"
        if self.use_hip:
            hip_ext(required=True)
        for k, v in list(self.__dict__.items()):
            if torch.is_tensor(v):
                setattr(self, k, v.to(device))
        if self.use_hip and self.wimg is None:
            self.wimg = torch.zeros(self._wimg_len(), dtype=torch.bfloat16, device=device)
        self._build_wimg()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """Logical (unpadded) weights + standardizer + Adam state.

        Includes the optimizer moments and step counter so a reloaded
        model RESUMES training exactly (bit-identical step sequence),
        not just serves inference. The moments are stored in the padded
        master layout — safe because load_state_dict enforces an exact
        geometry match, and the padded lanes are exact zeros by the
        Adam-from-zero-init invariant.
        """
        g = self.g
        W1, b1, W2, b2 = ref.unpack_master_g(g, self.master.cpu())
        return {
            "W1": W1[: g.in_features, : g.hidden].clone(),
            "b1": b1[: g.hidden].clone(),
            "W2": W2[: g.hidden, : g.classes].clone(),
            "b2": b2[: g.classes].clone(),
            "mean": self.mean.cpu().clone(),
            "invstd": self.invstd.cpu().clone(),
            "geometry": torch.tensor([g.in_features, g.hidden, g.classes]),
            "adam_m": self.m.cpu().clone(),
            "adam_v": self.v.cpu().clone(),
            "adam_t": self.t_dev.cpu().clone(),
        }

    def load_state_dict(self, state: Dict[str, torch.Tensor]):
        g = self.g
        head = state.get("head", HEAD_CLASSIFIER)
        if head != g.head:
            raise ValueError(f"state head {head!r} != model head {g.head!r}")
        if "geometry" in state:
            want = tuple(int(x) for x in state["geometry"])
            have = (g.in_features, g.hidden, g.classes)
            if want != have:
                raise ValueError(f"state geometry {want} != model geometry {have}")
        master = torch.zeros(g.nparam, dtype=torch.float32)
        W1, b1, W2, b2 = ref.unpack_master_g(g, master)
        W1[: g.in_features, : g.hidden] = state["W1"]
        b1[: g.hidden] = state["b1"]
        W2[: g.hidden, : g.classes] = state["W2"]
        b2[: g.classes] = state["b2"]
        self.master.copy_(master.to(self.device))
        self.bfmirror.copy_(self.master.bfloat16())
        self.mean.copy_(state["mean"].to(self.device))
        self.invstd.copy_(state["invstd"].to(self.device))
        if "adam_m" in state:  # full checkpoint: resume training exactly
            self.m.copy_(state["adam_m"].to(self.device))
            self.v.copy_(state["adam_v"].to(self.device))
            self.t_dev.copy_(state["adam_t"].to(self.device))
        else:  # weights-only (pre-resume checkpoints): fresh optimizer
            self.m.zero_()
            self.v.zero_()
            self.t_dev.zero_()
        self._graph = self._graph_key = None
        self._build_wimg()


class _Validation:
    """One train_epochs call's validation pass: the staged held-out rows,
    the per-epoch record history and its device slot, and the host-side
    early-stopping / best-snapshot bookkeeping."""

    STATE = ("master", "bfmirror", "m", "v", "t_dev")

    def __init__(self, model, validation, epochs, patience, min_delta, restore_best):
        self.model = model
        self.X, self.y = model._eval_inputs(*validation)
        if not self.X.shape[0]:
            raise ValueError("validation needs at least one row")
        self.patience, self.min_delta = patience, float(min_delta)
        self.restore_best = restore_best
        self.on_host = patience is not None or restore_best
        self.best, self.bad, self.snap, self.ran = float("inf"), 0, None, 0
        self.records = []           # CPU path
        self.hist = self.slot = None
        if model.use_hip:
            model._ensure_eval(self.X.shape[0])
            buf = model._val_buf
            if buf is None or buf[0].shape[0] != epochs:
                # cap = epochs is baked into a captured finish launch
                buf = model._val_buf = (
                    torch.empty(epochs, model._eval_rec_n(), dtype=torch.float32,
                                device=model.device),
                    torch.empty(1, dtype=torch.int32, device=model.device),
                )
            self.hist, self.slot = buf
            self.hist.zero_()
            self.slot.zero_()       # before the first epoch

    def _track(self, loss: float) -> bool:
        """Bookkeeping after an epoch whose validation loss is ``loss``:
        True to stop."""
        self.ran += 1
        if not self.on_host:
            return False
        if loss < self.best - self.min_delta:
            self.best, self.bad = loss, 0
            if self.restore_best:
                self.snap = {k: getattr(self.model, k).clone() for k in self.STATE}
        else:
            self.bad += 1
        return self.patience is not None and self.bad >= self.patience

    def after_epoch(self, e: int) -> bool:
        """Device path: read epoch ``e``'s record (one sync)."""
        L = self.model._rec_layout()
        return self._track(float(self.hist[e, L.EVAL_REC_LOSS].item()))

    def after_epoch_ref(self, e: int) -> bool:
        """CPU path: evaluate, record, track."""
        rec = self.model._ref_eval(self.X, self.y)
        self.records.append(rec)
        return self._track(float(rec[self.model._rec_layout().EVAL_REC_LOSS]))

    def finish(self):
        m = self.model
        if m.use_hip:
            ran = self.ran if self.on_host else int(self.slot.item())
            m.val_history = self.hist[:ran].cpu()
        else:
            m.val_history = torch.stack(self.records)
        m._val_n = self.X.shape[0]
        if self.restore_best and self.snap is not None:
            for k, t in self.snap.items():
                getattr(m, k).copy_(t)
            m._build_wimg()


class TabularMLPRegressor(TabularMLP):
    """TabularMLP with a regression head: Linear -> ReLU -> Linear trained
    on squared error over ``targets`` continuous outputs (1..32).

    Everything but the head is TabularMLP's: the packed weight image, the
    per-workgroup gradient slabs, the reduce+Adam kernel, hipGraph-captured
    epochs, the RCCL all-reduce path and checkpointing. The step and the
    predict kernels are the generalized family's regression instantiations
    (tabular_gen.hip) at every shape, 64x32xT included; on the CPU the same
    class runs ops/reference.py's ``mlp_step_reg_g``.

    Targets are standardized per column like the features: the network
    learns ``(Y - y_mean) * y_invstd`` and the predict kernel's epilogue
    turns its output back into target units.
    """

    HEAD = HEAD_REGRESSION

    def __init__(
        self,
        in_features: int,
        hidden: int = 32,
        targets: int = 1,
        device: Optional[str] = None,
        seed: int = 0,
    ):
        super().__init__(in_features, hidden, targets, device, seed)
        T = self.g.classes
        # target scaler: the identity until fit_target_standardizer
        self.y_mean = torch.zeros(T, dtype=torch.float32, device=self.device)
        self.y_invstd = torch.ones(T, dtype=torch.float32, device=self.device)
        self.y_scale = torch.ones(T, dtype=torch.float32, device=self.device)

    @property
    def targets(self) -> int:
        return self.g.classes

    def _targets_2d(self, Y: torch.Tensor) -> torch.Tensor:
        Y = torch.as_tensor(Y).to(self.device, torch.float32)
        if Y.dim() == 1:
            Y = Y.unsqueeze(1)
        if Y.dim() != 2 or Y.shape[1] != self.g.classes:
            raise ValueError(
                f"targets must be [N][{self.g.classes}], got {tuple(Y.shape)}"
            )
        return Y.contiguous()

    # -- target standardizer -----------------------------------------------------

    def fit_target_standardizer(self, Y: torch.Tensor, eps: float = 1e-5):
        """Column mean / inverse std of the targets (the feature
        standardizer's kernel), and ``y_scale = 1 / y_invstd`` for the
        predict epilogue."""
        Y = self._targets_2d(Y)
        if self.use_hip:
            hip_ext().standardize_fit(Y, self.y_mean, self.y_invstd, eps)
        else:
            mean, invstd = ref.standardize_fit(Y, eps)
            self.y_mean.copy_(mean)
            self.y_invstd.copy_(invstd)
        self.y_scale.copy_(1.0 / self.y_invstd)

    def stage_targets(self, Y: torch.Tensor) -> torch.Tensor:
        """Standardized fp32 targets, zero-padded to the kernel's
        [N][cpad] layout (once per fit: plain torch ops, not the hot path)."""
        g = self.g
        Y = self._targets_2d(Y)
        Yt = torch.zeros(Y.shape[0], g.cpad, dtype=torch.float32, device=self.device)
        Yt[:, : g.classes] = (Y - self.y_mean) * self.y_invstd
        return Yt

    # -- training --------------------------------------------------------------

    def _prep_targets(self, Yt: torch.Tensor) -> torch.Tensor:
        Yt = Yt.to(self.device, torch.float32).contiguous()
        if Yt.dim() != 2 or Yt.shape[1] != self.g.cpad:
            raise ValueError(
                f"Yt must be the staged [N][{self.g.cpad}] targets "
                f"(stage_targets), got {tuple(Yt.shape)}"
            )
        return Yt

    def _gen_step_kernel(self, ext, Xbf, Yt, rpw: int, invBtot: float) -> bool:
        g = self.g
        return ext.mlp_step_reg_gen(
            Xbf, Yt, g.hid, g.classes, rpw, self.wimg, self.master,
            self.slabs, invBtot,
        )

    def _shuffle_kernel(self, ext, Xbf, Yt, Xs, Yts, seed: int):
        ext.shuffle_rows_reg(Xbf, Yt, Xs, Yts, self.t_dev, seed)

    def _ref_step(self, Xbf, Yt, invBtot: float):
        ref.mlp_step_reg_g(
            self.g, Xbf, Yt, self.W1bf, self.W2bf, self.master, self.grads, invBtot
        )

    # -- evaluation ------------------------------------------------------------

    def _eval_rec_n(self) -> int:
        L = self._rec_layout()
        return L.EVAL_REC_FIRST_MSE + self.g.cpad

    def _eval_kernel(self, ext, Xbf, Yt, wimg, hist, slot):
        g = self.g
        ext.mlp_eval_reg_gen(
            Xbf, Yt, g.hid, g.classes, wimg, self.master, self._eval_part, hist, slot
        )

    def _ref_eval(self, Xbf, Yt) -> torch.Tensor:
        return ref.mlp_eval_reg_g(self.g, Xbf, Yt, self.W1bf, self.W2bf, self.master)

    def _decode_record(self, rec: torch.Tensor, n: int, sst=None) -> dict:
        """mse per target in original units (the column MSE times
        y_scale^2); with ``sst`` (per-target total sum of squares in
        standardized units) also r2 = 1 - SSE / SST."""
        L = self._rec_layout()
        T = self.g.classes
        col = rec[L.EVAL_REC_FIRST_MSE : L.EVAL_REC_FIRST_MSE + T].double()
        mse = col * self.y_scale.detach().cpu().double() ** 2
        out = {"loss": float(rec[L.EVAL_REC_LOSS]), "mse": mse.tolist(),
               "mse_mean": float(mse.mean()), "n": n}
        if sst is not None:
            r2 = 1.0 - col * n / sst
            out["r2"] = r2.tolist()
            out["r2_mean"] = float(r2.mean())
        return out

    def _empty_metrics(self) -> dict:
        nan = float("nan")
        T = self.g.classes
        return {"loss": nan, "mse": [nan] * T, "mse_mean": nan, "r2": [nan] * T,
                "r2_mean": nan, "n": 0}

    def evaluate(self, Xbf: torch.Tensor, Yt: torch.Tensor) -> dict:
        """Metrics of the staged rows against staged targets
        (``stage_targets``), on the device: ``{"loss", "mse", "r2", "n"}``
        plus ``mse_mean`` / ``r2_mean`` over the targets. ``loss`` is the
        training loss (half the squared error summed over targets, mean
        over rows, standardized units); ``mse`` and ``r2`` are per target,
        ``mse`` in original target units. The total sum of squares behind
        ``r2`` comes from ordinary torch ops on the staged targets."""
        Xbf, Yt = self._eval_inputs(Xbf, Yt)
        n = Xbf.shape[0]
        if not n:
            return self._empty_metrics()
        Yr = Yt[:, : self.g.classes].double()
        sst = ((Yr - Yr.mean(dim=0)) ** 2).sum(dim=0).cpu()
        return self._decode_record(self._eval_record(Xbf, Yt), n, sst)

    def evaluate_raw(self, X: torch.Tensor, Y: torch.Tensor) -> dict:
        """``evaluate`` of raw features and raw targets: stages both."""
        return self.evaluate(self.stage(torch.as_tensor(X)), self.stage_targets(Y))

    def train_epochs(self, Xbf: torch.Tensor, Yt: torch.Tensor, *,
                     engine: str = "auto", **kwargs) -> float:
        """TabularMLP.train_epochs over staged targets ``Yt``
        (stage_targets); returns the last step's loss, half the mean
        squared error in standardized units summed over the targets. The
        persistent engine exists for the digits classifier only."""
        if engine == "persistent":
            raise ValueError("engine='persistent' is a classifier engine")
        return super().train_epochs(Xbf, Yt, engine=engine, **kwargs)

    # -- inference -------------------------------------------------------------

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        """fp32 [B][targets] in original target units."""
        g = self.g
        X = X.to(self.device, torch.float32).contiguous()
        if self.use_hip:
            out = torch.empty(X.shape[0], g.classes, dtype=torch.float32, device=self.device)
            if X.shape[0]:
                hip_ext().mlp_predict_reg_gen(
                    X, g.inp, g.hid, g.classes, self.mean, self.invstd, self.wimg,
                    self.master, self.y_mean, self.y_scale, out,
                )
            return out
        return ref.mlp_predict_reg_g(
            g, X, self.mean, self.invstd, self.W1bf, self.W2bf, self.master,
            self.y_mean, self.y_scale,
        )

    # -- persistence -----------------------------------------------------------

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """TabularMLP's state plus the head tag and the target scaler."""
        state = super().state_dict()
        state["head"] = HEAD_REGRESSION
        state["y_mean"] = self.y_mean.cpu().clone()
        state["y_invstd"] = self.y_invstd.cpu().clone()
        return state

    def load_state_dict(self, state: Dict[str, torch.Tensor]):
        missing = [k for k in ("y_mean", "y_invstd") if k not in state]
        if state.get("head") == HEAD_REGRESSION and missing:
            # without its target scaler a regressor predicts in other units
            raise ValueError(f"regression state lacks the target scaler: {missing}")
        super().load_state_dict(state)   # raises on a classifier state
        self.y_mean.copy_(state["y_mean"].to(self.device))
        self.y_invstd.copy_(state["y_invstd"].to(self.device))
        self.y_scale.copy_(1.0 / self.y_invstd)
