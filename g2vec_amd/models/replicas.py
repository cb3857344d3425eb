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
from typing import List

import torch

from .. import ops
from ..config import G2VecConfig
from .cbow import CbowTrainer, TrainResult


class ReplicaTrainer:
    def __init__(self, cfg: G2VecConfig, n_genes: int, device: torch.device,
                 log=print):
        cfg.validate()
        cfg.check_replicate_scope()
        self.cfg = cfg
        self.G = n_genes
        self.h = cfg.hidden
        self.device = device
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
        st = type("ReplicaState", (), {})()
        st.R = R
        st.tr, st.vl, st.plan, st.inv_b = b.tr, b.vl, b.plan, b.inv_b
        st.ev_genes, st.ev_offsets = b.ev_genes, b.ev_offsets
        st.ev_labels = b.ev_labels if b.ev_genes is not None else None
        st.W = torch.empty(R, G, h, dtype=torch.float32, device=dev)
        st.who = torch.empty(R, h, dtype=torch.float32, device=dev)
        st.W[0].copy_(b.W)
        st.who[0].copy_(b.who)
        for name in ("W", "mW", "vW", "W_keep"):     # only the shared pieces
            delattr(b, name)                         # of the base state stay
        for r in range(1, R):
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
        st.t_adam = 0
        st.epoch_idx = 0
        st.graph = None
        st.graph_failed = False
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
    def _epoch_body(self, st) -> None:
        """CbowTrainer._epoch_body_fast, batched: optimizer step at W_t from
        the pending dO_R, then post-update s_R, the accuracy counts and the
        next epoch's dO_R. Persistent buffers only, so it can be captured."""
        B = CbowTrainer
        lrt = st.lrt_buf if self.device.type == "cuda" else None
        c_R = ops.scatter_dO_rep(st.plan, st.dO_R, self.G)
        ops.adam_rank1_rep(st.W, st.mW, st.vW, c_R, st.who, st.mO, st.vO,
                           st.t_adam, self.cfg.lr, B.B1, B.B2, B.EPS,
                           lrt_buf=lrt)
        ops.gemv_rows_rep_(st.W, st.who, st.s_R)
        if st.ev_genes is not None:
            ops.cbow_eval_counts_rep_(st.s_R, st.ev_genes, st.ev_offsets,
                                      st.ev_labels, st.tr.n_paths,
                                      st.counts_R, dO_R=st.dO_R,
                                      inv_b=st.inv_b)

    def _ensure_graph(self, st) -> None:
        """Single-branch hipGraph of the body from the second epoch on, as
        CbowTrainer._ensure_graph (lr_t is read from its device slot)."""
        if (self.device.type == "cuda" and self.cfg.use_hipgraph and
                st.graph is None and not st.graph_failed and
                st.epoch_idx >= 1):
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._epoch_body(st)
                st.graph = g
            except Exception as e:  # noqa: BLE001
                st.graph_failed = True
                self.log(f"    (hipGraph capture unavailable: {e!r}; "
                         f"running eager)")

    def run_epoch(self, st):
        """One epoch of all replicas and ONE [R, 2] readback. Returns
        (acc_tr, acc_val), two lists of R floats."""
        B = CbowTrainer
        st.t_adam += 1
        if self.device.type == "cuda":
            st.lrt_buf.fill_(ops.tf1_lr_t(self.cfg.lr, B.B1, B.B2, st.t_adam))
            self._ensure_graph(st)
        if st.graph is not None:
            st.graph.replay()
        else:
            self._epoch_body(st)
        cc = st.counts_R.cpu().numpy()
        st.epoch_idx += 1
        acc_tr = [float(cc[r, 0]) / max(self.n_tr, 1) for r in range(st.R)]
        acc_val = [float(cc[r, 1]) / max(self.n_vl, 1) for r in range(st.R)]
        return acc_tr, acc_val

    # ------------------------------------------------------------------ train
    def train(self, ps, R: int) -> List[TrainResult]:
        cfg = self.cfg
        st = self.setup(ps, R)
        R = st.R
        before_val, before_tr = [-1.0] * R, [-1.0] * R
        stop_epoch, epochs_run = [-1] * R, [0] * R
        stopped = [False] * R
        hist: List[List[float]] = [[] for _ in range(R)]
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
                epochs_run[r] = epoch + 1
                hist[r].append(acc_val[r])
                times[r].append(now - ep_t0)
                if wall[r] is None and acc_val[r] >= CbowTrainer.ACC_TARGET:
                    wall[r] = now - t0_all
                if cfg.early_stop and acc_val[r] < before_val[r]:
                    stopped[r] = True
                    stop_epoch[r] = epoch - 1
                else:
                    before_val[r], before_tr[r] = acc_val[r], acc_tr[r]
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
        for r in range(R):
            self.log("    - Replica %02d: Epoch(stop): %03d\tACC[val]=%.4f"
                     "\tACC[tr]=%.4f" % (r, stop_epoch[r], before_val[r],
                                         before_tr[r]))
            out.append(TrainResult(
                W_ih=self.base._unrelabel(final[r]), stop_epoch=stop_epoch[r],
                acc_val=before_val[r], acc_tr=before_tr[r],
                epochs_run=epochs_run[r], acc_val_history=hist[r],
                epoch_times_s=times[r], wall_to_acc_s=wall[r]))
        self.log("    Optimization Finish (%.3f sec)"
                 % (time.perf_counter() - t0_all))
        return out
