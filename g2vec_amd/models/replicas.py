"""R model replicates trained in one batched epoch (--replicates R).

G2Vec is stochastic: the truncated-normal initialisation alone moves the
d-score ranking from seed to seed. Replicates differ ONLY in their initial
weights (replica r is the plain run with seed + r), so everything derived
from the paths — the optional relabel, the seeded 80/20 split, the locality
sort, the scatter plan, the concatenated eval set, inv_b — is built once,
by CbowTrainer.setup itself, and shared. With the replica index innermost
in the s / dO / c tables one id load serves all replicas, the R gathered
values are contiguous, and the launch count stays that of one model:

    scatter_dO_rep -> adam_rank1_rep -> gemv_rows_rep_ -> cbow_eval_counts_rep_

Every batched op is, per replica, bitwise the single op on the same device
(ops/__init__.py), so replica r's trajectory, stop epoch and returned W_ih
are bitwise those of the corresponding single synchronous run.

Early stop is per replica with the reference rule (first epoch whose
val-ACC falls below the previous one; last-good weights returned). Replicas
are independent, so a stopped one simply keeps being stepped while its
snapshot, history and stop epoch stay frozen.
"""
from __future__ import annotations

import dataclasses
import time
from typing import Any, List, Optional

import torch

from .. import ops
from ..config import G2VecConfig
from ..parallel.dist import single
from ..paths import PathSet
from .cbow import CbowTrainer, StopTracker, TrainResult, accuracies


@dataclasses.dataclass
class ReplicaState:
    """TrainState's batched counterpart: the path-derived pieces are the
    base state's, the weight-shaped ones carry a leading replica axis."""
    R: int
    tr: PathSet
    vl: PathSet
    plan: Any
    inv_b: float
    ev_genes: Optional[torch.Tensor]
    ev_offsets: Optional[torch.Tensor]
    ev_labels: Optional[torch.Tensor]
    W: torch.Tensor                          # [R, G, h]
    who: torch.Tensor                        # [R, h]
    mW: Optional[torch.Tensor] = None
    vW: Optional[torch.Tensor] = None
    mO: Optional[torch.Tensor] = None
    vO: Optional[torch.Tensor] = None
    W_keep: Optional[torch.Tensor] = None    # only under early stop
    s_R: Optional[torch.Tensor] = None       # [G, R]
    dO_R: Optional[torch.Tensor] = None      # [P_tr, R]
    counts_R: Optional[torch.Tensor] = None  # [R, 2]
    lrt_buf: Optional[torch.Tensor] = None
    t_adam: int = 0
    epoch_idx: int = 0
    graph: Any = None
    graph_failed: bool = False


class ReplicaTrainer:
    B1, B2, EPS = CbowTrainer.B1, CbowTrainer.B2, CbowTrainer.EPS
    # the epoch step and its single-branch hipGraph capture (from the
    # second epoch on; lr_t is read from its device slot) are the single
    # trainer's own methods, run on this trainer's batched body: they touch
    # only device, cfg, ctx, log and _epoch_body_fast
    _step_epoch = CbowTrainer._step_epoch
    _ensure_graph = CbowTrainer._ensure_graph

    def __init__(self, cfg: G2VecConfig, n_genes: int, device: torch.device,
                 log=print):
        cfg.validate()
        cfg.check_replicate_scope()
        self.cfg = cfg
        self.G = n_genes
        self.h = cfg.hidden
        self.device = device
        self.ctx = single(device)       # replicates are single-process
        self.log = log

    # ------------------------------------------------------------------ setup
    def _check_memory(self, ps, R: int) -> None:
        """W, m, v and the last-good snapshot are R*G*h*16 bytes; refuse
        before allocating when that plus the path tables would not fit."""
        if self.device.type != "cuda":
            return
        nnz, P = int(ps.genes.numel()), int(ps.n_paths)
        tables = 12 * nnz + P * (4 * R + 16) + 16 * self.G * R
        need = R * self.G * self.h * 16 + tables
        free, _total = torch.cuda.mem_get_info(self.device)
        if need > 0.8 * free:
            raise ValueError(
                f"--replicates {R}: needs about {need / 2**30:.2f} GiB "
                f"(R*G*h*16 = {R * self.G * self.h * 16 / 2**30:.2f} GiB of "
                f"weights, moments and snapshots + {tables / 2**30:.2f} GiB "
                f"of path tables), more than 80% of the "
                f"{free / 2**30:.2f} GiB free on {self.device}")

    def setup(self, ps, R: int):
        if not 1 <= int(R) <= ops.REP_MAX:
            raise ValueError(f"replicates must be in [1, {ops.REP_MAX}], "
                             f"got {R}")
        R = int(R)
        cfg = self.cfg
        self._check_memory(ps, R)
        seed = (int(cfg.seed) if cfg.seed is not None
                else int(torch.randint(0, 2 ** 31 - 1, (1,)).item()))
        quiet = lambda *a, **k: None   # noqa: E731
        # replica 0 IS the plain run: its setup builds the shared pieces
        self.base = CbowTrainer(dataclasses.replace(cfg, seed=seed), self.G,
                                self.device, log=quiet)
        b = self.base.setup(ps)
        self.n_tr, self.n_vl = self.base.n_tr_global, self.base.n_vl_global
        dev, G, h = self.device, self.G, self.h
        st = ReplicaState(
            R=R, tr=b.tr, vl=b.vl, plan=b.plan, inv_b=b.inv_b,
            ev_genes=b.ev_genes, ev_offsets=b.ev_offsets,
            ev_labels=b.ev_labels,
            W=torch.empty(R, G, h, dtype=torch.float32, device=dev),
            who=torch.empty(R, h, dtype=torch.float32, device=dev))
        st.W[0].copy_(b.W)
        st.who[0].copy_(b.who)
        b.W = b.mW = b.vW = b.W_keep = None      # only the shared pieces
        for r in range(1, R):                    # of the base state stay
            t = CbowTrainer(dataclasses.replace(cfg, seed=seed + r), G, dev,
                            log=quiet)
            gen = torch.Generator()
            gen.manual_seed(seed + r)
            W, who = t._init_weights(gen)
            if self.base.gene_order is not None:     # rows into the relabel
                W = W[self.base.gene_order]
            st.W[r].copy_(W)
            st.who[r].copy_(who)
            del W, who
        st.mW, st.vW = torch.zeros_like(st.W), torch.zeros_like(st.W)
        st.mO, st.vO = torch.zeros_like(st.who), torch.zeros_like(st.who)
        st.W_keep = st.W.clone() if cfg.early_stop else None
        st.s_R = torch.empty(G, R, dtype=torch.float32, device=dev)
        st.dO_R = torch.zeros(st.tr.n_paths, R, dtype=torch.float32,
                              device=dev)
        st.counts_R = torch.zeros(R, 2, dtype=torch.float32, device=dev)
        st.lrt_buf = torch.zeros(1, dtype=torch.float32, device=dev)
        # the pending dlogits of the first step: one eval over the train
        # paths at the initial weights
        ops.gemv_rows_rep_(st.W, st.who, st.s_R)
        if st.tr.n_paths > 0:
            ops.cbow_eval_counts_rep_(st.s_R, st.tr.genes, st.tr.offsets,
                                      st.tr.labels, st.tr.n_paths,
                                      st.counts_R, dO_R=st.dO_R,
                                      inv_b=st.inv_b)
        return st

    # ------------------------------------------------------------------ epoch
    def _epoch_body_fast(self, st) -> None:
        """CbowTrainer._epoch_body_fast, batched: optimizer step at W_t from
        the pending dO_R, then post-update s_R, the accuracy counts and the
        next epoch's dO_R. Persistent buffers only, so it can be captured."""
        lrt = st.lrt_buf if self.device.type == "cuda" else None
        c_R = ops.scatter_dO_rep(st.plan, st.dO_R, self.G)
        ops.adam_rank1_rep(st.W, st.mW, st.vW, c_R, st.who, st.mO, st.vO,
                           st.t_adam, self.cfg.lr, self.B1, self.B2, self.EPS,
                           lrt_buf=lrt)
        ops.gemv_rows_rep_(st.W, st.who, st.s_R)
        if st.ev_genes is not None:
            ops.cbow_eval_counts_rep_(st.s_R, st.ev_genes, st.ev_offsets,
                                      st.ev_labels, st.tr.n_paths,
                                      st.counts_R, dO_R=st.dO_R,
                                      inv_b=st.inv_b)

    def run_epoch(self, st):
        """One epoch of all replicas and ONE [R, 2] readback. Returns
        (acc_tr, acc_val), two lists of R floats."""
        self._step_epoch(st)
        accs = [accuracies(c, self.n_tr, self.n_vl)
                for c in st.counts_R.cpu().numpy()]
        return [a[0] for a in accs], [a[1] for a in accs]

    # ------------------------------------------------------------------ train
    def train(self, ps, R: int) -> List[TrainResult]:
        cfg = self.cfg
        st = self.setup(ps, R)
        R = st.R
        trk = [StopTracker(cfg.early_stop) for _ in range(R)]
        stopped = [False] * R
        times: List[List[float]] = [[] for _ in range(R)]
        wall: List = [None] * R
        t0_all = time.perf_counter()
        self.log("     Start training %d replicates of the modified CBOW "
                 "with early stopping" % R)
        for epoch in range(cfg.epochs):
            ep_t0 = time.perf_counter()
            acc_tr, acc_val = self.run_epoch(st)
            now = time.perf_counter()
            for r in range(R):
                if stopped[r]:
                    continue
                times[r].append(now - ep_t0)
                if wall[r] is None and acc_val[r] >= CbowTrainer.ACC_TARGET:
                    wall[r] = now - t0_all
                stopped[r] = trk[r].feed(epoch, acc_tr[r], acc_val[r])
            if cfg.early_stop:          # keep-last-good, frozen once stopped
                if not any(stopped):
                    st.W_keep.copy_(st.W)
                else:
                    for r in range(R):
                        if not stopped[r]:
                            st.W_keep[r].copy_(st.W[r])
                if all(stopped):
                    break
        out = []
        final = st.W_keep if cfg.early_stop else st.W
        for r, t in enumerate(trk):
            self.log("    - Replica %02d: Epoch(stop): %03d\tACC[val]=%.4f"
                     "\tACC[tr]=%.4f" % (r, t.stop_epoch, t.before_val,
                                         t.before_tr))
            out.append(TrainResult(
                W_ih=self.base._unrelabel(final[r]), stop_epoch=t.stop_epoch,
                acc_val=t.before_val, acc_tr=t.before_tr,
                epochs_run=len(t.hist), acc_val_history=t.hist,
                epoch_times_s=times[r], wall_to_acc_s=wall[r]))
        self.log("    Optimization Finish (%.3f sec)"
                 % (time.perf_counter() - t0_all))
        return out
