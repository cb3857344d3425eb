"""Modified-CBOW trainer (reference step 4, G2Vec.py:217-286).

Model: X (multi-hot paths) @ W_ih -> H; H @ W_ho -> logit; sigmoid-CE on the
prognosis label. No biases, no nonlinearity (G2Vec.py:238-243) — the net is
LINEAR, which the MI355X fast path exploits:

  forward:   o_p = sum_{g in p} s_g      with s = W_ih @ W_ho   (one GEMV +
             a scalar segment-sum kernel instead of a [B,G]x[G,h] matmul)
  backward:  dW_ih = c (outer) W_ho,  dW_ho = W_ih^T c,
             with c = X^T dO in R^G    (rank-1 gradient: the per-epoch DP
             all-reduce message is the G floats of c, not G*h — dW_ho is
             recomputed per rank from the reduced c, so h floats never
             travel. A second 2-float metric all-reduce runs per epoch
             only under early stopping; fixed-epoch runs defer it to one
             history-sized reduce after the loop.)

The kernel-chain "general" path (gather rows -> wave reduce -> scatter-add,
SURVEY §2.10 K1-K8) computes the identical math without the collapse and is
the template for non-linear successors; both paths share Adam and early-stop.

Reference-semantics notes:
  - training is FULL-BATCH, one Adam step per epoch (G2Vec.py:262-264);
    --batch-size > 0 opts into minibatching (documented divergence)
  - accuracy is evaluated with the POST-update weights each epoch
    (sess.run(optimizer) then acc.eval, G2Vec.py:264-267)
  - early stop: first epoch whose val-ACC is strictly lower than the
    previous epoch's; the returned W_ih is the PREVIOUS epoch's
    (keep-last-good semantics, G2Vec.py:276-283)
  - Adam is TF1 AdamOptimizer (dense moments; lr_t = lr*sqrt(1-b2^t)/(1-b1^t))
  - init: truncated normal, stddev 1/sqrt(hidden), +-2 sigma (G2Vec.py:234-235)

Layout of the trainer: setup() returns a declared TrainState. Every runner
advances the fast full-batch epoch through ONE step (_step_epoch) or ONE
block replay (_replay_block), applies the dip rule through ONE StopTracker
and converts counts through accuracies(). The runners differ only in where
the last-good weights live: run_epochs_sync (W_keep; also the minibatch /
general / checkpointing runner), run_epochs_pipelined (rolling snapshots;
fixed-epoch runs take the deferred-readback _run_epochs_kblocked) and
run_epochs_kgranular (restore-and-replay). train() picks one and hands its
on_epoch callback to the one _Reporter that owns the transcript and the
TrainResult.
"""
from __future__ import annotations

import dataclasses
import operator
import time
from typing import Any, List, Optional

import torch

from .. import ops
from ..config import G2VecConfig
from ..parallel.dist import DistContext, single
from ..paths import PathSet, subset


class _CpuEvent:
    """No-op stand-in for torch.cuda.Event: lets the epoch pipeline's
    ordering/collective logic run (and be gloo-tested) on CPU hosts, where
    every launch is synchronous anyway."""
    def record(self):
        pass

    def synchronize(self):
        pass


@dataclasses.dataclass
class TrainResult:
    W_ih: torch.Tensor            # f32 [G, h] on the training device
    stop_epoch: int               # reference's reported epoch (step-1 on stop)
    acc_val: float
    acc_tr: float
    epochs_run: int
    acc_val_history: List[float]
    epoch_times_s: List[float]
    wall_to_acc_s: Optional[float]   # wall-clock until val-ACC >= 0.88 (None if never)


@dataclasses.dataclass
class TrainState:
    """Everything setup() builds and the runners mutate. The lazily filled
    fields (graphs and per-runner buffers) are declared here too, so that a
    reader — and bench.py, which looks at graph / kgraph / pipe_bufs — sees
    what a state can hold."""
    W: torch.Tensor
    who: torch.Tensor
    mW: torch.Tensor
    vW: torch.Tensor
    mO: torch.Tensor
    vO: torch.Tensor
    W_keep: torch.Tensor             # keep-last-good snapshot (sync runner)
    tr: PathSet
    vl: PathSet
    plan: Any                        # gene-sorted instance plan (backward)
    inv_b: float
    batches: list
    W16: Optional[torch.Tensor] = None      # general path, bf16/fp16 copy
    t_adam: int = 0
    epoch_idx: int = 0
    # persistent fast-path buffers (stable addresses across hipGraph replays)
    s_buf: Optional[torch.Tensor] = None
    c_buf: Optional[torch.Tensor] = None    # the GPU epoch body's c = X^T dO:
                                            # all +0.0 at every epoch boundary
                                            # (derived, so no snapshot or
                                            # checkpoint carries it)
    lrt_buf: Optional[torch.Tensor] = None
    counts_buf: Optional[torch.Tensor] = None
    dO_buf: Optional[torch.Tensor] = None   # pending dlogits of the next step
    ev_genes: Optional[torch.Tensor] = None  # concatenated train+val eval set
    ev_offsets: Optional[torch.Tensor] = None
    ev_labels: Optional[torch.Tensor] = None
    graph: Any = None                # per-epoch hipGraph (_ensure_graph)
    graph_failed: bool = False
    kbufs: Optional[tuple] = None    # (klrt [K], kcounts [K, 2])
    kparts: Optional[torch.Tensor] = None   # [K, eval grid, 2]: the block's
                                            # count partials, folded once
    kgraph: Any = None               # K-epoch block graph (_ensure_kgraph)
    kblock_k: Optional[int] = None   # K of the recorded block graph
    kgraph_failed: bool = False
    run_bufs: Optional[tuple] = None   # fixed-epoch runner: (pinned lr_t
                                       # staging, device schedule, history)
    pipe_bufs: Optional[tuple] = None  # pipelined runner: (pinned counts,
                                       # rolling snapshots | None, events)


# the tensors of the mutable epoch state: with t_adam and epoch_idx they are
# what a snapshot/restore or a train-state checkpoint has to carry
EPOCH_TENSORS = ("W", "who", "mW", "vW", "mO", "vO", "dO_buf")
_epoch_tensors = operator.attrgetter(*EPOCH_TENSORS)


def accuracies(counts, n_tr: int, n_vl: int) -> tuple:
    """(acc_tr, acc_val) from one epoch's two correct-counts (a host array
    or pinned tensor: callers read a whole history back at once, because
    per-element float(tensor[i, j]) on a fresh readback costs ~2.4 us)."""
    return float(counts[0]) / max(n_tr, 1), float(counts[1]) / max(n_vl, 1)


def capture_graph(body, log, label: str):
    """Record body() into a hipGraph (recording executes nothing). Returns
    the graph, or None after logging `label` with the error — the caller
    then sets its *_failed flag and stays on its eager path."""
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            body()
        return g
    except Exception as e:  # noqa: BLE001
        log(label % repr(e))
        return None


class StopTracker:
    """The reference dip rule with its bookkeeping (G2Vec.py:276-283): fed
    (epoch, acc_tr, acc_val) in order, feed() is True at the first epoch
    whose val-ACC is strictly below the previous one's. `hist` includes the
    dip epoch; before_val / before_tr stay the last good epoch's and
    stop_epoch is the epoch BEFORE the dip. Which weights are that epoch's
    is the runner's business."""

    def __init__(self, early_stop: bool, before_val: float = -1.0,
                 before_tr: float = -1.0, hist: Optional[list] = None):
        self.early_stop = early_stop
        self.before_val, self.before_tr = before_val, before_tr
        self.hist: List[float] = hist if hist is not None else []
        self.stop_epoch = -1

    def feed(self, epoch: int, acc_tr: float, acc_val: float) -> bool:
        self.hist.append(acc_val)
        if self.early_stop and acc_val < self.before_val:
            self.stop_epoch = epoch - 1
            return True
        self.before_val, self.before_tr = acc_val, acc_tr
        return False


class _Reporter:
    """The training transcript, the timings and the TrainResult: on_epoch
    is the runners' per-epoch callback, finish() closes the run."""

    def __init__(self, log, before_val: float = -1.0, before_tr: float = -1.0):
        self.log = log
        self.epoch_times: List[float] = []
        self.wall_to_acc = None
        self.prev = self.cur = (before_val, before_tr)
        self.log("     Start training the modified CBOW with early stopping")
        self.t0 = self.last = self.blk_t0 = time.perf_counter()

    def on_epoch(self, e: int, acc_tr: float, acc_val: float) -> None:
        now = time.perf_counter()
        self.epoch_times.append(now - self.last)
        self.last = now
        self.prev, self.cur = self.cur, (acc_val, acc_tr)
        if self.wall_to_acc is None and acc_val >= CbowTrainer.ACC_TARGET:
            self.wall_to_acc = now - self.t0
        if e % 5 == 0:
            self.log("    - Epoch: %03d\tACC[val]=%.4f\tACC[tr]=%.4f (%.3f sec)"
                     % (e, acc_val, acc_tr, now - self.blk_t0))
            self.blk_t0 = now

    def finish(self, W_ih, hist, stop_epoch: int) -> TrainResult:
        acc_val, acc_tr = self.cur
        if stop_epoch >= 0:          # the last callback was the dip epoch
            acc_val, acc_tr = self.prev
            self.log("    - Epoch(stop): %03d\tACC[val]=%.4f\tACC[tr]=%.4f (%.3f sec)"
                     % (stop_epoch, acc_val, acc_tr,
                        time.perf_counter() - self.blk_t0))
        self.log("    Optimization Finish")
        return TrainResult(W_ih=W_ih, stop_epoch=stop_epoch,
                           acc_val=acc_val, acc_tr=acc_tr,
                           epochs_run=len(hist), acc_val_history=hist,
                           epoch_times_s=self.epoch_times,
                           wall_to_acc_s=self.wall_to_acc)


class CbowTrainer:
    B1, B2, EPS = 0.9, 0.999, 1e-8   # TF1 AdamOptimizer defaults (G2Vec.py:246)
    ACC_TARGET = 0.88                # BASELINE.md headline threshold

    def __init__(self, cfg: G2VecConfig, n_genes: int,
                 device: torch.device, ctx: Optional[DistContext] = None,
                 log=print):
        cfg.validate()
        self.cfg = cfg
        self.G = n_genes
        self.h = cfg.hidden
        self.device = device
        self.ctx = ctx or single(device)
        self.log = log

    # ------------------------------------------------------------------ setup
    def _init_weights(self, gen: Optional[torch.Generator]):
        """+-2sigma truncated normal, stddev 1/sqrt(h) (G2Vec.py:234-235).
        On GPU the K9 device kernel fills W in place from a counter-based
        stream — no host-side rejection loop (which materialized multi-GB
        intermediates at 1M x 512); on CPU the seeded host sampler keeps
        its round-1 bit-exact streams. Unseeded runs derive a random seed
        (rank 0's broadcast in setup() makes ranks agree either way)."""
        std = 1.0 / (self.h ** 0.5)
        if self.device.type == "cuda":
            if self.cfg.seed is not None:
                dev_seed = int(self.cfg.seed)
            else:
                dev_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            W = torch.empty(self.G, self.h, dtype=torch.float32,
                            device=self.device)
            who = torch.empty(self.h, dtype=torch.float32,
                              device=self.device)
            ops.trunc_normal_(W, std, dev_seed)
            ops.trunc_normal_(who, std, dev_seed + 0x9E3779B9)
            return W, who
        W = torch.empty(self.G, self.h, dtype=torch.float32)
        who = torch.empty(self.h, dtype=torch.float32)
        if gen is None:
            torch.nn.init.trunc_normal_(W, std=std, a=-2 * std, b=2 * std)
            torch.nn.init.trunc_normal_(who, std=std, a=-2 * std, b=2 * std)
        else:
            with torch.no_grad():
                W.copy_(_trunc_normal(W.shape, std, gen))
                who.copy_(_trunc_normal(who.shape, std, gen))
        return W.to(self.device), who.to(self.device)

    def _split(self, ps: PathSet, pre_sharded: bool = False):
        """Seeded shuffle + 80/20 split (G2Vec.py:219-226), then DP shard.

        pre_sharded=True means `ps` is already this rank's local shard
        (weak-scaling benches): split locally, count globally."""
        P = ps.n_paths
        gen = torch.Generator()
        if self.cfg.seed is not None:
            gen.manual_seed(int(self.cfg.seed) + 12345 +
                            (self.ctx.rank if pre_sharded else 0))
        elif self.ctx.world > 1 and not pre_sharded:
            # unseeded DP: every rank must draw the SAME global shuffle or
            # the train/val shards would overlap/miss paths — agree on a
            # random seed via broadcast
            shared = torch.randint(0, 2**31 - 1, (1,),
                                   device=self.device, dtype=torch.int64)
            self.ctx.broadcast_(shared)
            gen.manual_seed(int(shared.item()))
        perm = torch.randperm(P, generator=gen).to(self.device)
        pivot = int(P * 0.8)
        tr_idx, vl_idx = perm[:pivot], perm[pivot:]
        if pre_sharded:
            counts = torch.tensor([tr_idx.numel(), vl_idx.numel()],
                                  dtype=torch.float64, device=self.device)
            self.ctx.allreduce_(counts)
            self.n_tr_global = int(counts[0].item())
            self.n_vl_global = int(counts[1].item())
        else:
            self.n_tr_global = int(tr_idx.numel())
            self.n_vl_global = int(vl_idx.numel())
            tr_idx = tr_idx[self.ctx.shard_indices(tr_idx.numel(), self.device)]
            vl_idx = vl_idx[self.ctx.shard_indices(vl_idx.numel(), self.device)]
        return subset(ps, tr_idx), subset(ps, vl_idx)

    @staticmethod
    def _locality_sort(ps: PathSet) -> PathSet:
        if ps.n_paths == 0:
            return ps
        first = ps.genes[ps.offsets[:-1].long()].long()
        order = torch.argsort(first, stable=True)
        return subset(ps, order)

    def _relabel_enabled(self) -> bool:
        mode = self.cfg.gene_relabel
        return mode == "on" or (mode == "auto" and self.G >= 100_000)

    def _first_touch_order(self, ps: PathSet) -> torch.Tensor:
        """i64 [G] new-id -> old-id: genes ordered by their first
        appearance in the flat path stream. Co-path genes (one walk ≈ one
        co-expression module) land on contiguous new ids, so the fwd/eval
        s-gathers and the W-row gathers of consecutive paths touch
        L1-resident slices instead of random 4-byte lines across the
        whole table — the measured wall of the 100k+-gene configs
        (profiles/README.md, 1M-config notes). Untouched genes keep
        their relative order at the end. Rank 0's order is broadcast so
        every DP rank maps identically (the c all-reduce lives in the
        relabeled id space); when weak-scaling ranks hold INDEPENDENT
        datasets, rank 0's order is correct-but-approximate locality for
        the other ranks."""
        big = torch.iinfo(torch.int64).max
        first = torch.full((self.G,), big, dtype=torch.int64,
                           device=ps.genes.device)
        pos = torch.arange(ps.genes.numel(), dtype=torch.int64,
                           device=ps.genes.device)
        first.scatter_reduce_(0, ps.genes.long(), pos, reduce="amin")
        # stable argsort: untouched genes (key=big) keep ascending old id
        order = torch.argsort(first, stable=True)
        self.ctx.broadcast_(order)
        return order

    def setup(self, ps: PathSet, pre_sharded: bool = False) -> TrainState:
        """Initialise weights/optimizer state and split the path set.
        Returns the mutable training state used by the runners."""
        cfg = self.cfg
        gen = None
        if cfg.seed is not None:
            gen = torch.Generator()
            gen.manual_seed(int(cfg.seed))
        W, who = self._init_weights(gen)
        self.ctx.broadcast_(W)      # C4: replicated params (all ranks identical)
        self.ctx.broadcast_(who)
        self.gene_order = None      # new-id -> old-id (gather-locality relabel)
        self.gene_o2n = None
        if self._relabel_enabled():
            order = self._first_touch_order(ps)
            o2n = torch.empty_like(order)
            o2n[order] = torch.arange(self.G, dtype=torch.int64,
                                      device=order.device)
            ps = PathSet(o2n[ps.genes.long()].int().contiguous(),
                         ps.offsets, ps.labels, ps.n_genes)
            # weights were drawn in OLD-id order (seed parity with the
            # unrelabeled run): permute rows into the relabeled layout —
            # gene old(j)=order[j] keeps its exact init vector
            W = W[order].contiguous()
            self.gene_order, self.gene_o2n = order, o2n
        tr, vl = self._split(ps, pre_sharded)

        use_general = cfg.trainer_path == "general"
        if cfg.batch_size == 0:
            # full batch: within-shard path ORDER is free (all math is a sum
            # over paths) — sort paths by first gene so co-module paths are
            # processed by adjacent sub-waves and the s/dO gathers hit
            # cache-resident slices instead of the whole table
            tr = self._locality_sort(tr)
            vl = self._locality_sort(vl)
        # gene-sorted instance plan: drives the deterministic backward on
        # both trainer paths (genes never change across epochs). The
        # general path's row backward writes one dW row per segment, so it
        # takes the single-pass layout at every path count.
        plan = ops.build_scatter_plan(tr.genes, tr.offsets, self.G,
                                      slabs=not use_general)
        if self.n_tr_global + self.n_vl_global == 0:
            raise ValueError(
                "no paths to train on: the integrated path set is empty "
                "(every walk was dropped as a cross-group duplicate, or "
                "the PCC-thresholded graphs have no edges — check the "
                "expression signal / --pcc-threshold)")
        P_loc = tr.n_paths
        bs = cfg.batch_size if cfg.batch_size > 0 else max(P_loc, 1)
        st = TrainState(
            W=W, who=who, mW=torch.zeros_like(W), vW=torch.zeros_like(W),
            mO=torch.zeros_like(who), vO=torch.zeros_like(who),
            W_keep=W.clone(), tr=tr, vl=vl, plan=plan,
            inv_b=1.0 / max(self.n_tr_global, 1),
            batches=[(i, min(i + bs, P_loc)) for i in range(0, P_loc, bs)])
        if use_general and cfg.dtype != "fp32":
            st.W16 = (W.bfloat16() if cfg.dtype == "bf16" else W.half())
        if self.ctx.world > 1 and cfg.batch_size > 0:
            # lockstep minibatching: strided shards can differ by one
            # path, so per-rank batch COUNTS can differ — pad with empty
            # batches up to the global max so every rank joins the same
            # number of grad all-reduces (an empty batch contributes a
            # zero gradient)
            nb = torch.tensor([float(len(st.batches))], dtype=torch.float64,
                              device=self.device)
            self.ctx.allreduce_max_(nb)
            while len(st.batches) < int(nb.item()):
                st.batches.append((P_loc, P_loc))
        # persistent fast-path buffers (stable addresses across hipGraph replays)
        if not use_general:
            st.s_buf = torch.empty(self.G, dtype=torch.float32,
                                   device=self.device)
            ops.gemv_rows(W, who, st.s_buf)
            st.c_buf = torch.zeros(self.G, dtype=torch.float32,
                                   device=self.device)
        st.lrt_buf = torch.zeros(1, dtype=torch.float32, device=self.device)
        st.counts_buf = torch.zeros(2, dtype=torch.float32, device=self.device)
        # concatenated train+val evaluation set: both accuracy splits ride
        # ONE forward kernel per epoch
        if not use_general and tr.n_paths + vl.n_paths > 0:
            off_vl = vl.offsets.int() + tr.offsets[-1]
            st.ev_genes = torch.cat([tr.genes, vl.genes]).contiguous()
            st.ev_offsets = torch.cat([tr.offsets, off_vl[1:]]).contiguous()
            st.ev_labels = torch.cat([tr.labels, vl.labels]).contiguous()
        # full-batch steady state fuses the forward into the PREVIOUS
        # epoch's eval (same s, same train paths — the gather runs once per
        # weight version): dO_buf carries the pending dlogits; seed it here
        # from the initial weights (the one standalone forward of a run)
        if not use_general and cfg.batch_size == 0:
            st.dO_buf = torch.zeros(tr.n_paths, dtype=torch.float32,
                                    device=self.device)
            if tr.n_paths > 0:
                _l, _c, d0 = ops.cbow_fwd_scalar(
                    st.s_buf, tr.genes, tr.offsets, tr.labels, st.inv_b, True)
                st.dO_buf.copy_(d0)
        return st

    def _epoch_body_fast(self, st, counts_out=None, lrt_slot=None,
                         reduce_counts: bool = True,
                         partials_out=None) -> None:
        """One full-batch fast-path epoch as a capturable body: optimizer
        step at W_t, then post-update s + accuracy counts. All inputs and
        outputs live in persistent buffers (s_buf, lrt_buf, counts_buf) so
        the body can be recorded once into a hipGraph and replayed.

        counts_out/lrt_slot override the default buffers — the k-epoch
        block graph records k bodies, each bound to its own slot of a
        [k,2] counts buffer and a [k] lr_t buffer.

        reduce_counts=False skips the C3 metric all-reduce: fixed-epoch
        runs consume accuracies only after the loop, so per-epoch counts
        go into a device-side history that is all-reduced ONCE at the end
        (identical values — the sum over ranks commutes with the copy into
        the history). Steady-state collective cost: one grad all-reduce
        per epoch. Early-stop epochs keep reduce_counts=True (the stop
        decision reads the global accuracy every epoch).

        partials_out (block graph only): the eval parks its per-block
        count partials in that table and folds nothing; counts_out is then
        written by the block's ONE fold_partials_rows_ after its last body.

        On GPU c lives in st.c_buf, zero on entry and zero again on exit:
        the scatter accumulates into it, and the post-update GEMV — which
        runs after Adam, c's only reader — clears it in the same launch, so
        the chain has no fill node. Five kernels per epoch in a block
        graph: scatter, adam_rank1, fold_gw_adam, gemv_rows, eval."""
        cfg = self.cfg
        tr, vl = st.tr, st.vl
        on_gpu = self.device.type == "cuda"
        if counts_out is None:
            counts_out = st.counts_buf
        if self.device.type != "cuda" or st.ev_genes is None:
            counts_out.zero_()      # CPU oracle accumulates (+=); the GPU
                                    # fold kernel OVERWRITES counts, so the
                                    # fill launch is pure overhead there
                                    # (still zeroed on an empty-shard rank,
                                    # whose eval never runs)
        if lrt_slot is not None:
            lrt = lrt_slot
        else:
            lrt = st.lrt_buf if self.device.type == "cuda" else None
        # dO for THIS epoch's step was emitted by the previous epoch's
        # fused eval (or the setup() seeding) — no standalone forward
        c = ops.scatter_dO(tr.genes, tr.offsets, st.dO_buf, self.G,
                           plan=st.plan, out=st.c_buf if on_gpu else None)
        self.ctx.allreduce_(c)                  # C1: whole dW_ih message
        # fused tail: one streaming pass over the pre-update W rows does
        # the rank-1 Adam AND emits dW_ho = W_pre^T c; a fold launch
        # applies the who update (3 launches + a full W read saved)
        ops.adam_rank1_fused(st.W, st.mW, st.vW, c, st.who, st.mO, st.vO,
                             st.t_adam, cfg.lr, self.B1, self.B2, self.EPS,
                             lrt_buf=lrt)
        # post-update accuracy (reference order, G2Vec.py:264-267): one
        # fused eval kernel over the concatenated train+val paths, which
        # ALSO emits the next epoch's train dlogits (post-update s is the
        # next epoch's pre-update s — bitwise the same forward)
        ops.gemv_rows(st.W, st.who, st.s_buf,
                      clear=st.c_buf if on_gpu else None)
        if st.ev_genes is not None:
            ops.cbow_eval_counts_(st.s_buf, st.ev_genes, st.ev_offsets,
                                  st.ev_labels, tr.n_paths, counts_out,
                                  dO=st.dO_buf, inv_b=st.inv_b,
                                  partials=partials_out)
        if reduce_counts:
            self.ctx.allreduce_(counts_out)     # C3: 2-float metric reduce

    def run_epoch(self, st) -> tuple:
        """One reference epoch: optimizer step(s) at W_t, then post-update
        accuracy on both splits (G2Vec.py:262-267). Returns (acc_tr, acc_val).

        Fast full-batch path: the whole epoch body runs from persistent
        buffers; s = W_ih @ W_ho is computed once per weight version, and on
        GPU the body is recorded into a hipGraph once (epoch >= 2) and
        replayed thereafter — one graph launch + one 8-byte D2H per epoch."""
        cfg = self.cfg
        fast_full = cfg.trainer_path != "general" and cfg.batch_size == 0
        if fast_full:
            self._step_epoch(st)
            return self._accs(st.counts_buf.cpu().numpy())

        for (lo, hi) in st.batches:
            # empty pad batch (lockstep minibatching): zero local grad,
            # scale irrelevant
            b_inv = (st.inv_b if cfg.batch_size == 0 else
                     (1.0 / ((hi - lo) * self.ctx.world) if hi > lo else 0.0))
            st.t_adam += 1
            if cfg.trainer_path == "general":
                self._step_general(st, lo, hi, b_inv, st.t_adam)
            else:
                self._step_fast(st, lo, hi, b_inv, st.t_adam)
        if cfg.trainer_path == "general":
            acc_tr = self._accuracy(st.W, st.W16, st.who, st.tr, self.n_tr_global)
            acc_val = self._accuracy(st.W, st.W16, st.who, st.vl, self.n_vl_global)
        else:
            ops.gemv_rows(st.W, st.who, st.s_buf)   # post-update s
            counts = torch.empty(2, dtype=torch.float32, device=self.device)
            for k, split in enumerate((st.tr, st.vl)):
                if split.n_paths == 0:
                    counts[k] = 0.0
                    continue
                _l, corr, _d = ops.cbow_fwd_scalar(
                    st.s_buf, split.genes, split.offsets, split.labels, 1.0, False)
                counts[k] = corr.sum()
            self.ctx.allreduce_(counts)         # C3: one fused metric reduce
            acc_tr, acc_val = self._accs(counts.cpu().numpy())
        st.epoch_idx += 1
        return acc_tr, acc_val

    def _accs(self, counts) -> tuple:
        return accuracies(counts, self.n_tr_global, self.n_vl_global)

    def _step_epoch(self, st, **body_kw) -> None:
        """Advance ONE fast full-batch epoch, asynchronously: bump t_adam,
        stage lr_t, run the body, bump epoch_idx. body_kw are the optional
        counts_out / lrt_slot / reduce_counts of _epoch_body_fast. lr_t
        goes into st.lrt_buf with one fill launch unless the caller brings
        a slot that already holds it (a slice of a staged schedule: no
        launch). The per-epoch graph is a recording of the DEFAULT body,
        so it is captured and replayed only when nothing is overridden;
        an overridden body runs eagerly (at world>1 the recorded body's
        metric all-reduce must not slip into a deferred-metric run)."""
        st.t_adam += 1
        if "lrt_slot" not in body_kw and self.device.type == "cuda":
            st.lrt_buf.fill_(ops.tf1_lr_t(self.cfg.lr, self.B1, self.B2,
                                          st.t_adam))
        if not body_kw:
            self._ensure_graph(st)
        if not body_kw and st.graph is not None:
            st.graph.replay()
        else:
            self._epoch_body_fast(st, **body_kw)
        st.epoch_idx += 1

    def _ensure_graph(self, st) -> None:
        """Capture the epoch body into a hipGraph when eligible. At
        world>1 the body contains RCCL collectives; capture is gated on a
        one-time runtime probe (DistContext.graph_capture_ok: capture +
        replay + verify a tiny all-reduce; G2VEC_DIST_GRAPH=0 opts out).
        A rank that falls back to eager stays collective-compatible with
        ranks that replay graphs — both issue the identical collective
        sequence per epoch. A CPU-device trainer never captures, also on
        a host that has a GPU: its body would run once during capture,
        record nothing, and every replay would then be a no-op epoch."""
        if (self.device.type == "cuda" and
                self.cfg.use_hipgraph and st.graph is None and
                not st.graph_failed and st.epoch_idx >= 1 and
                self.ctx.graph_capture_ok()):
            st.graph = capture_graph(
                lambda: self._epoch_body_fast(st), self.log,
                "    (hipGraph capture unavailable: %s; running eager)")
            st.graph_failed = st.graph is None

    def _launch_epoch(self, st, slot: int, pinned, snaps, events,
                      keep: bool = True) -> None:
        """Queue one whole epoch asynchronously: the step, D2H copy of the
        accuracy counts into pinned memory, rolling weight snapshot,
        completion event. Stream order guarantees the copy reads THIS
        epoch's counts before the next epoch's body overwrites them."""
        self._step_epoch(st)
        pinned[slot].copy_(st.counts_buf, non_blocking=True)
        if keep:                            # rolling keep-last-good snapshot;
            snaps[slot][0].copy_(st.W)      # skipped when early_stop is off
            snaps[slot][1].copy_(st.who)    # (2 GB/epoch at the 1M x 512 cfg)
        events[slot].record()

    KBLOCK = 8   # epochs recorded per block graph (fixed-epoch runs)

    def pick_kblock(self, n_epochs: int) -> int:
        """Block size whose replays tile n_epochs with no eager tail:
        n itself when small (one replay per run), else the largest
        divisor <= 64, else the default KBLOCK (leaves a short tail).
        A non-dividing block size leaves n % K epochs running as eager
        bodies — measured ~0.02 ms/epoch slower than a replayed body at
        ex scale (0.066 vs 0.063 ms mean at steps=30 with K=8)."""
        n = max(int(n_epochs), 1)
        if n <= 64:
            return n
        for k in range(64, 1, -1):
            if n % k == 0:
                return k
        return self.KBLOCK

    def _ensure_kgraph(self, st, k: Optional[int] = None) -> None:
        """Allocate the k-block buffers and record the k-epoch block graph
        (recording executes nothing and mutates no epoch state). Callable
        ahead of time — bench.py warms it during the untimed warmup so the
        one-time capture never lands in a timed region. Requires at least
        one prior eager epoch (st.epoch_idx >= 1). At world>1 each
        recorded body contains the grad all-reduce; capture is gated on
        the runtime RCCL-capture probe (see _ensure_graph). Bodies are
        recorded with reduce_counts=False — the kblocked runner all-
        reduces the accuracy history once after the loop — and with their
        count partials parked in st.kparts, folded by one launch recorded
        after the K bodies (5K + 1 kernels per replay). When capture is
        unavailable the caller's eager tail loop runs every epoch — still
        with the deferred readback/reduce.

        k sizes the recorded block (pick_kblock chooses one that tiles a
        known run length); k=None keeps the existing recorded size, or
        KBLOCK if none was recorded yet."""
        if self.device.type != "cuda" or not self.cfg.use_hipgraph:
            return
        if not self.ctx.graph_capture_ok():
            return
        K = max(int(k), 1) if k is not None else (st.kblock_k or self.KBLOCK)
        if st.kbufs is None or st.kbufs[0].numel() != K:
            st.kbufs = (
                torch.empty(K, dtype=torch.float32, device=self.device),
                torch.zeros(K, 2, dtype=torch.float32, device=self.device))
            st.kparts = None
            st.kgraph = None
        if st.kgraph is None and not st.kgraph_failed:
            klrt, kcounts = st.kbufs
            # body j parks its eval's count partials in row j of one table
            # (<= 1 MB at K = 64) and ONE launch after the K bodies folds
            # the rows into kcounts: nothing reads a block's counts before
            # its replay has ended. A rank without paths runs no eval; its
            # bodies zero their counts slots themselves.
            if st.ev_genes is not None:
                grid = ops.eval_grid(st.ev_labels.numel(), self.G)
                if st.kparts is None or tuple(st.kparts.shape) != (K, grid, 2):
                    st.kparts = torch.empty(K, grid, 2, dtype=torch.float32,
                                            device=self.device)
            kparts = st.kparts

            def bodies():
                for j in range(K):
                    self._epoch_body_fast(
                        st, counts_out=kcounts[j], lrt_slot=klrt[j:j + 1],
                        reduce_counts=False,
                        partials_out=None if kparts is None else kparts[j])
                if kparts is not None:
                    ops.fold_partials_rows_(kparts, kcounts)
            # capture mutates no epoch state; on failure callers fall back
            # to the per-epoch path / eager tail loop
            st.kgraph = capture_graph(
                bodies, self.log, "    (k-epoch block graph unavailable: "
                                  "%s; running per-epoch)")
            if st.kgraph is not None:
                st.kblock_k = K
            else:
                st.kgraph_failed = True

    def kblock_eligible(self, st, n_epochs: int, early_stop: bool) -> bool:
        """Fixed-epoch runs go through the deferred-readback runner: block
        graphs where capture is available, eager epoch bodies otherwise
        (--no-hipgraph / failed probe / CPU) — either way zero mid-run D2H
        and ONE metric all-reduce for the whole run."""
        return (not early_stop and not st.kgraph_failed and
                st.ev_genes is not None and n_epochs >= 2)

    def _run_epochs_kblocked(self, st, n_epochs: int, on_epoch):
        """Fixed-epoch fast path (early stop OFF): KBLOCK epochs are
        recorded into ONE hipGraph — each recorded body bound to its own
        lr_t slot and [2]-counts slot. Per-epoch counts are appended to a
        DEVICE-side history with D2D copies; the whole history is read
        back in a single D2H at the end AND (world>1) all-reduced in a
        single collective: zero mid-run host<->device crossings and ONE
        metric collective per RUN — the steady-state per-epoch collective
        cost is exactly the grad all-reduce. (A rare per-process driver
        slow-mode was traced to degraded D2H copies — ~1 ms each
        regardless of size; with one final read the worst case costs
        ~1 ms per RUN, not per block.)
        Exact per-epoch semantics: every epoch runs the full optimizer
        pass and both accuracy evals; fixed-epoch runs consume the
        accuracies only after the loop, so deferring the readback and the
        metric sum-over-ranks (which commutes with the history append)
        changes nothing observable. Runs on CPU too (eager bodies, same
        deferred schedule) so the gloo DP tier covers this exact path.
        Returns the run_epochs_pipelined tuple."""
        on_gpu = self.device.type == "cuda"
        if st.epoch_idx == 0:    # one eager epoch: warm allocator/state
            warm = [self.run_epoch(st)]
        else:
            warm = []
        self._ensure_kgraph(st)
        n_rest = n_epochs - len(warm)
        # recorded block size (pick_kblock); epochs past the last whole
        # block, or all of them without a graph, run as the eager tail
        K = st.kblock_k if st.kgraph is not None else None
        n_blocked = (n_rest // K) * K if K else 0
        # whole lr_t schedule staged to device ONCE; each block slices it
        # (_replay_block). The staging itself goes through a cached pinned
        # buffer with a non-blocking H2D: a plain torch.tensor(...,
        # device="cuda") synchronizes, and at ex scale that ~50 us is a
        # measurable share of a 30 x 0.063 ms timed run.
        sched_vals = torch.tensor(
            [ops.tf1_lr_t(self.cfg.lr, self.B1, self.B2, st.t_adam + i)
             for i in range(1, n_rest + 1)], dtype=torch.float32)
        if on_gpu:
            cap = max(n_rest, 1)
            if st.run_bufs is None or st.run_bufs[0].numel() < cap:
                st.run_bufs = (
                    torch.empty(cap, dtype=torch.float32, pin_memory=True),
                    torch.empty(cap, dtype=torch.float32,
                                device=self.device),
                    torch.zeros(cap, 2, dtype=torch.float32,
                                device=self.device))
            pin, sched, hist_dev = st.run_bufs
            pin[:n_rest].copy_(sched_vals)               # host-side copy
            sched = sched[:cap]
            sched.copy_(pin[:cap], non_blocking=True)
            hist_dev = hist_dev[:cap]
        else:
            sched = sched_vals
            hist_dev = torch.zeros(max(n_rest, 1), 2, dtype=torch.float32,
                                   device=self.device)
        for lo in range(0, n_blocked, K or 1):
            self._replay_block(st, sched[lo:lo + K], hist_dev[lo:lo + K])
        for e in range(n_blocked, n_rest):     # tail: eager bodies, same
            # zero-readback scheme; lr_t straight from its schedule slot
            self._step_epoch(st, lrt_slot=sched[e:e + 1], reduce_counts=False)
            hist_dev[e].copy_(st.counts_buf, non_blocking=True)
            if on_gpu and (e - n_blocked + 1) % 64 == 0:   # bound launch-
                torch.cuda.synchronize()   # queue depth, long eager runs

        if n_rest > 0:
            self.ctx.allreduce_(hist_dev)      # C3: ONE reduce for the run
        # the ONE host readback; .numpy() view because per-element
        # float(tensor[i, j]) costs ~2.4 us each — 60 of them were
        # ~145 us of a ~1.9 ms 30-epoch run (numpy indexing: ~11 us)
        accs = warm + [self._accs(c) for c in hist_dev.cpu().numpy()[:n_rest]]
        if on_epoch is not None:
            for e, (acc_tr, acc_val) in enumerate(accs):
                on_epoch(e, acc_tr, acc_val)
        return ([a[1] for a in accs], -1, st.W, st.who,
                accs[-1][0] if accs else 0.0)

    def _replay_block(self, st, sched_slice, hist_out) -> None:
        """Replay the recorded K-epoch block once: K lr_t values from
        sched_slice into the graph's slots, then the K per-epoch counts
        (local, not yet reduced) into hist_out. All stream-ordered D2D
        copies — a host-side refill of klrt could race a replay still
        queued behind it."""
        klrt, kcounts = st.kbufs
        klrt.copy_(sched_slice, non_blocking=True)
        st.t_adam += st.kblock_k
        st.epoch_idx += st.kblock_k
        st.kgraph.replay()
        hist_out.copy_(kcounts, non_blocking=True)

    def _snapshot(self, st):
        """Deep copy of the mutable epoch state (for k-granular replay)."""
        return ([t.clone() if t is not None else None
                 for t in _epoch_tensors(st)], st.t_adam, st.epoch_idx)

    def _restore(self, st, snap) -> None:
        saved, st.t_adam, st.epoch_idx = snap
        for dst, src in zip(_epoch_tensors(st), saved):
            if src is not None:
                dst.copy_(src)

    def _run_block(self, st, k: int, hist_out) -> None:
        """k epoch bodies, per-epoch counts into hist_out[:k] (local, not
        yet reduced). Uses the recorded block graph when k matches."""
        if st.kgraph is not None and k == st.kblock_k:
            sched = torch.tensor(
                [ops.tf1_lr_t(self.cfg.lr, self.B1, self.B2, st.t_adam + i)
                 for i in range(1, k + 1)],
                dtype=torch.float32, device=self.device)
            return self._replay_block(st, sched, hist_out[:k])
        for j in range(k):
            self._step_epoch(st, reduce_counts=False)
            hist_out[j].copy_(st.counts_buf, non_blocking=True)

    def run_epochs_kgranular(self, st, n_epochs: int, k: int, on_epoch=None):
        """Early-stop training with accuracy readbacks every k epochs
        (opt-in, --earlystop-every k; round-1 verdict item 8 / STATUS
        item 1). EXACT reference semantics via deterministic replay: run
        k epochs with counts parked in a device-side history, then ONE
        all-reduce + ONE D2H for the block; if the reference dip rule
        (val-ACC strictly below the previous epoch's, G2Vec.py:276-279)
        fires at epoch e inside the block, restore the block-start
        snapshot and deterministically re-run to e-1 (the epoch body has
        no RNG, so the replayed weights are bitwise the epoch-granular
        ones). Costs <= k-1 epochs of discarded work per stop; saves
        (k-1)/k of the per-epoch collectives + readbacks that dominate
        small-problem multi-GPU epochs. Returns the run_epochs_pipelined
        tuple."""
        assert k >= 1
        trk = StopTracker(True)
        if st.epoch_idx == 0:      # eager warm epoch (allocator/graph prep)
            a_tr0, a_val0 = self.run_epoch(st)
            if on_epoch is not None:
                on_epoch(0, a_tr0, a_val0)
            trk.feed(0, a_tr0, a_val0)
            if n_epochs == 1:
                return trk.hist, -1, st.W, st.who, a_tr0
        self._ensure_kgraph(st)
        hist_dev = torch.zeros(k, 2, dtype=torch.float32, device=self.device)
        acc_tr = 0.0
        e = len(trk.hist)
        while e < n_epochs:
            blk = min(k, n_epochs - e)
            snap = self._snapshot(st)
            self._run_block(st, blk, hist_dev)
            self.ctx.allreduce_(hist_dev[:blk])     # one reduce per block
            cc = hist_dev[:blk].cpu().numpy()       # one D2H per block
            for j in range(blk):
                a_tr, a_val = self._accs(cc[j])
                if on_epoch is not None:
                    on_epoch(e + j, a_tr, a_val)
                if trk.feed(e + j, a_tr, a_val):
                    # dip at e + j: rewind to the state after stop_epoch —
                    # restore the block start (post-(e-1)) and
                    # deterministically re-run up to it; the body has no
                    # RNG, so the replayed weights are bitwise the
                    # epoch-granular ones
                    self._restore(st, snap)
                    if j > 0:
                        self._run_block(st, j, hist_dev)
                    return trk.hist, trk.stop_epoch, st.W, st.who, acc_tr
                acc_tr = a_tr
            e += blk
        return trk.hist, -1, st.W, st.who, acc_tr

    def run_epochs_pipelined(self, st, n_epochs: int, early_stop: bool,
                             on_epoch=None):
        """Speculative epoch pipeline (GPU fast-path full-batch only):
        epoch e+1's launch is queued before epoch e's accuracy readback, so
        the per-epoch D2H sync overlaps the next epoch's compute. Reference
        semantics are exact: the accuracy trajectory is identical, an
        early-stop truncates the history at the dip, the returned weights
        are the pre-dip epoch's (rolling 3-deep snapshots implement the
        keep-last-good rule, G2Vec.py:276-283); at most one speculative
        epoch's compute is discarded. Returns (hist, stop_epoch, final_W,
        final_who, last_acc_tr)."""
        DEPTH = 3
        on_gpu = self.device.type == "cuda"
        if self.kblock_eligible(st, n_epochs, early_stop):
            return self._run_epochs_kblocked(st, n_epochs, on_epoch)
        if st.pipe_bufs is None:
            st.pipe_bufs = (
                [torch.empty(2, dtype=torch.float32, pin_memory=on_gpu)
                 for _ in range(DEPTH)],
                ([(torch.empty_like(st.W), torch.empty_like(st.who))
                  for _ in range(DEPTH)] if early_stop else None),
                [torch.cuda.Event() if on_gpu else _CpuEvent()
                 for _ in range(DEPTH)])
        pinned, snaps, events = st.pipe_bufs
        if early_stop and snaps is None:    # first call was early_stop=False
            snaps = [(torch.empty_like(st.W), torch.empty_like(st.who))
                     for _ in range(DEPTH)]
            st.pipe_bufs = (pinned, snaps, events)
        trk = StopTracker(early_stop)
        self._launch_epoch(st, 0, pinned, snaps, events, keep=early_stop)
        launched = 1
        e = 0
        while True:
            if launched < n_epochs and launched - e < DEPTH - 1:
                self._launch_epoch(st, launched % DEPTH, pinned, snaps,
                                   events, keep=early_stop)
                launched += 1
            events[e % DEPTH].synchronize()
            acc_tr, acc_val = self._accs(pinned[e % DEPTH])
            if on_epoch is not None:
                on_epoch(e, acc_tr, acc_val)
            if trk.feed(e, acc_tr, acc_val):
                # dip at e: report/return epoch e-1 from its rolling slot
                W_good, who_good = snaps[trk.stop_epoch % DEPTH]
                return trk.hist, trk.stop_epoch, W_good, who_good, acc_tr
            e += 1
            if e >= n_epochs:
                return trk.hist, -1, st.W, st.who, acc_tr

    def run_epochs_sync(self, st, n_epochs: int, early_stop: bool,
                        on_epoch=None, tracker: Optional[StopTracker] = None,
                        after_epoch=None):
        """The synchronous runner: one run_epoch and one readback per
        epoch, on any device and trainer path (minibatch and general
        included), keep-last-good in st.W_keep (G2Vec.py:283). Epochs are
        aligned with the host, so this is the runner under train-state
        checkpointing: it starts at st.epoch_idx (non-zero after
        load_train_state), takes a tracker primed with the resumed
        before_val / before_tr / history, and calls after_epoch(epoch,
        tracker) once per kept epoch. Returns the run_epochs_pipelined
        tuple."""
        trk = tracker if tracker is not None else StopTracker(early_stop)
        acc_tr = trk.before_tr
        for epoch in range(st.epoch_idx, n_epochs):
            acc_tr, acc_val = self.run_epoch(st)
            if on_epoch is not None:
                on_epoch(epoch, acc_tr, acc_val)
            if trk.feed(epoch, acc_tr, acc_val):
                break
            st.W_keep.copy_(st.W)
            if after_epoch is not None:
                after_epoch(epoch, trk)
        return trk.hist, trk.stop_epoch, st.W_keep, st.who, acc_tr

    # --------------------------------------------------- train-state ckpt
    def _fingerprint(self) -> dict:
        return {"n_genes": self.G, "hidden": self.h, "seed": self.cfg.seed,
                "lr": self.cfg.lr, "trainer_path": self.cfg.trainer_path,
                "world": self.ctx.world, "rank": self.ctx.rank}

    def save_train_state(self, st, path: str, extra: dict) -> None:
        """Epoch-boundary training checkpoint: weights,
        TF1-Adam moments, the fused-eval dlogit carry, early-stop
        trackers, and a config fingerprint. Resuming from it continues
        the EXACT trajectory (epoch bodies are deterministic)."""
        blob = {name: (t.cpu() if t is not None else None)
                for name, t in zip(EPOCH_TENSORS, _epoch_tensors(st))}
        blob.update(W_keep=st.W_keep.cpu(), t_adam=st.t_adam,
                    epoch_idx=st.epoch_idx, fingerprint=self._fingerprint())
        blob.update(extra)
        torch.save(blob, path)

    def load_train_state(self, st, path: str) -> dict:
        blob = torch.load(path, map_location="cpu", weights_only=False)
        fp, mine = blob["fingerprint"], self._fingerprint()
        # world / rank are recorded for the reader, not compared
        for key in ("n_genes", "hidden", "seed", "lr", "trainer_path"):
            if fp[key] != mine[key]:
                raise ValueError(
                    f"--resume-train checkpoint mismatch: {key} was "
                    f"{fp[key]}, this run has {mine[key]}")
        for name, dst in zip(EPOCH_TENSORS + ("W_keep",),
                             _epoch_tensors(st) + (st.W_keep,)):
            if dst is not None and blob[name] is not None:
                dst.copy_(blob[name].to(self.device))
        st.t_adam = int(blob["t_adam"])
        st.epoch_idx = int(blob["epoch_idx"])
        if st.s_buf is not None:        # derived: recompute from W, who
            ops.gemv_rows(st.W, st.who, st.s_buf)
        return blob

    # ------------------------------------------------------------------ train
    def train(self, ps: PathSet, pre_sharded: bool = False) -> TrainResult:
        """The one driver: resume if asked, pick a runner, report."""
        cfg = self.cfg
        st = self.setup(ps, pre_sharded)

        def rank_path(p: str) -> str:
            # dO_buf / split shards are rank-local: world>1 checkpoints
            # are one file per rank
            return p if self.ctx.world == 1 else f"{p}.rank{self.ctx.rank}"

        trk = StopTracker(cfg.early_stop)
        if cfg.resume_train:
            blob = self.load_train_state(st, rank_path(cfg.resume_train))
            trk = StopTracker(cfg.early_stop,
                              float(blob.get("before_val", -1.0)),
                              float(blob.get("before_tr", -1.0)),
                              list(blob.get("acc_hist", [])))
            self.log(f"    (resumed training state at epoch {st.epoch_idx} "
                     f"from {cfg.resume_train})")
        rep = _Reporter(self.log, trk.before_val, trk.before_tr)

        ckpting = bool(cfg.train_ckpt) or bool(cfg.resume_train)
        if (not ckpting and
                cfg.trainer_path != "general" and cfg.batch_size == 0 and
                (self.device.type == "cuda" or
                 (cfg.early_stop and cfg.earlystop_every > 1))):
            # GPU fast path always; CPU too when --earlystop-every opts
            # into the k-granular runner (the flag must never be a
            # silent no-op — cf. the round-1 --dtype finding).
            if cfg.early_stop and cfg.earlystop_every > 1:
                out = self.run_epochs_kgranular(
                    st, cfg.epochs, cfg.earlystop_every, rep.on_epoch)
            else:
                out = self.run_epochs_pipelined(
                    st, cfg.epochs, cfg.early_stop, rep.on_epoch)
        else:
            # Train-state checkpointing runs the synchronous runner on any
            # device: checkpoints must be epoch-aligned, which the
            # speculative pipeline is not.
            def save_ckpt(epoch, t):
                if (epoch + 1) % max(cfg.train_ckpt_every, 1) == 0:
                    self.save_train_state(
                        st, rank_path(cfg.train_ckpt),
                        {"acc_hist": t.hist, "before_val": t.before_val,
                         "before_tr": t.before_tr})
            out = self.run_epochs_sync(
                st, cfg.epochs, cfg.early_stop, rep.on_epoch, trk,
                save_ckpt if cfg.train_ckpt else None)
        hist, stop_epoch, W_final, _who, _acc_tr = out
        return rep.finish(self._unrelabel(W_final), hist, stop_epoch)

    def _unrelabel(self, W: torch.Tensor) -> torch.Tensor:
        """Rows back to original gene order (no-op when relabeling is off).
        Applied once, where weights leave the trainer."""
        if self.gene_o2n is None:
            return W
        return W[self.gene_o2n].contiguous()

    # ------------------------------------------------------------------ steps
    def _slice(self, ps: PathSet, lo: int, hi: int):
        if lo == 0 and hi == ps.n_paths:
            return ps.genes, ps.offsets, ps.labels
        offs = ps.offsets.long()
        g = ps.genes[offs[lo]:offs[hi]]
        o = (ps.offsets[lo:hi + 1] - ps.offsets[lo]).contiguous()
        return g, o, ps.labels[lo:hi]

    def _step_fast(self, st, lo, hi, inv_b, t):
        """Minibatch fast step (full-batch epochs go through
        _epoch_body_fast instead)."""
        W, who, tr = st.W, st.who, st.tr
        genes, offsets, labels = self._slice(tr, lo, hi)
        if lo != 0:                 # s_buf is fresh only for the first batch
            ops.gemv_rows(W, who, st.s_buf)
        _loss, _corr, dO = ops.cbow_fwd_scalar(st.s_buf, genes, offsets,
                                               labels, inv_b, True)
        use_plan = st.plan if (lo == 0 and hi == tr.n_paths) else None
        c = ops.scatter_dO(genes, offsets, dO, self.G, plan=use_plan)
        self.ctx.allreduce_(c)                      # C1: the whole dW_ih message
        ops.adam_rank1_fused(W, st.mW, st.vW, c, who, st.mO, st.vO, t,
                             self.cfg.lr, self.B1, self.B2, self.EPS)

    def _step_general(self, st, lo, hi, inv_b, t):
        W, W16, who, tr = st.W, st.W16, st.who, st.tr
        mW, vW, mO, vO = st.mW, st.vW, st.mO, st.vO
        genes, offsets, labels = self._slice(tr, lo, hi)
        Wg = W16 if W16 is not None else W
        act = 1 if self.cfg.activation == "relu" else 0
        _loss, _corr, dO, H = ops.cbow_fwd(Wg, who, genes, offsets, labels,
                                           inv_b, True, act=act)
        full = lo == 0 and hi == tr.n_paths
        dW = ops.cbow_bwd_rows(who, genes, offsets, dO, self.G,
                               plan=(st.plan if full else None),
                               H_pre=(H if act else None))
        grad_who = torch.mv((torch.relu(H) if act else H).t(), dO)
        self.ctx.allreduce_(dW)
        self.ctx.allreduce_(grad_who)
        ops.adam_dense(W, mW, vW, dW, t, self.cfg.lr, self.B1, self.B2, self.EPS)
        ops.adam_dense(who, mO, vO, grad_who, t, self.cfg.lr, self.B1,
                       self.B2, self.EPS)
        if W16 is not None:
            W16.copy_(W)

    def _accuracy(self, W, W16, who, ps: PathSet, n_global: int) -> float:
        """One split's accuracy on the general path (the fast path counts
        both splits in its fused eval)."""
        if ps.n_paths == 0:
            correct = torch.zeros((), dtype=torch.float32, device=self.device)
        else:
            Wg = W16 if W16 is not None else W
            _l, corr, _d, _h = ops.cbow_fwd(
                Wg, who, ps.genes, ps.offsets, ps.labels, 1.0, False,
                act=1 if self.cfg.activation == "relu" else 0)
            correct = corr.sum()
        self.ctx.allreduce_(correct)                # C3 scalar metric reduce
        return float(correct.item()) / max(n_global, 1)


def _trunc_normal(shape, std: float, gen: torch.Generator) -> torch.Tensor:
    """Seeded +-2sigma truncated normal via rejection resampling
    (reference init semantics, tf.truncated_normal G2Vec.py:234-235)."""
    out = torch.randn(shape, generator=gen) * std
    bad = out.abs() > 2 * std
    while bool(bad.any()):
        out[bad] = torch.randn((int(bad.sum()),), generator=gen) * std
        bad = out.abs() > 2 * std
    return out
