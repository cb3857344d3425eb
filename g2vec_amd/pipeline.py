"""End-to-end 7-step pipeline driver (reference main(), G2Vec.py:11-119).

Console transcript mirrors the reference's phase-numbered prints (they ARE
the published baseline); structured JSONL metrics go beside
them when cfg.log_jsonl is set.

`run` is the table of contents, one function per numbered step below it.
A tool that needs part of a run calls `load_study` (steps 1-2),
`generate_paths` (steps 2b-3) or `Steps56` (steps 5-6 of one weight matrix).
"""
from __future__ import annotations

import contextlib
import dataclasses
import functools
import time
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import io as gio
from . import ops, scoring, stability
from . import preprocess as pp
from .cluster import find_lgroups
from .cluster_quality import silhouette
from .config import G2VecConfig, resolve_device
from .graph import build_group_graph, dedupe_edges
from .models.cbow import CbowTrainer, TrainResult
from .models.replicas import ReplicaTrainer
from .neighbors import nearest_genes
from .parallel.dist import DistContext, single
from .paths import PathSet, integrate_pathsets
from .utils.obs import JsonlLogger, PhaseTimers
from .walks import WalkSet, generate_walks


def _run_seed(cfg: G2VecConfig) -> int:
    """cfg.seed; None -> nondeterministic like the reference."""
    return cfg.seed if cfg.seed is not None else int(time.time_ns() & 0x7FFFFFFF)


def _gather_walks(ctx: DistContext, ws: WalkSet) -> WalkSet:
    """C5: all-gather per-rank walk shards into the global walk set."""
    if ctx.world == 1:
        return ws
    nodes = torch.cat(ctx.allgather_varlen(ws.nodes))
    lengths = torch.cat(ctx.allgather_varlen(ws.lengths.unsqueeze(1))).squeeze(1)
    hashes = torch.cat(ctx.allgather_varlen(ws.hashes.unsqueeze(1))).squeeze(1)
    return WalkSet(nodes, lengths, hashes)


def generate_paths(cfg: G2VecConfig, expr_t: torch.Tensor, labels_t: torch.Tensor,
                   edge_idx_t: torch.Tensor, n_genes: int, ctx: DistContext,
                   log=print, timers: Optional[PhaseTimers] = None):
    """Steps 2b-3: per-group graph construction + random walks + integration.
    Returns (pathset, gene_freq, n_genes_in_paths, stats dict)."""
    timers = timers or PhaseTimers()
    seed = _run_seed(cfg)
    shard = ctx.shard_range(n_genes)
    edge_idx_t = dedupe_edges(edge_idx_t, n_genes)   # once for both groups
    overlap = expr_t.is_cuda
    # the CPU loop times every link of a chain; two overlapped chains are
    # timed from outside, as one phase
    phase = (lambda name: contextlib.nullcontext()) if overlap else timers.phase

    def chain(group: int):
        """One group's graph and this rank's walks on it."""
        with phase(f"graph_g{group}"):
            g = build_group_graph(expr_t, labels_t, group, edge_idx_t,
                                  n_genes, threshold=cfg.pcc_threshold,
                                  mode=cfg.pcc_mode, edges_deduped=True,
                                  corr=cfg.corr)
        with phase(f"walks_g{group}"):
            ws = generate_walks(g, cfg.len_path, cfg.num_repetition, seed,
                                group, shard)
            return g, ws if overlap else _gather_walks(ctx, ws)

    if overlap:
        # the two prognosis groups' graph-build + walk chains are
        # independent: run them on separate HIP streams so each group's
        # PCC/threshold/CSR torch chains and walk kernel overlap the
        # other's (the C5 all-gather stays on the default stream, after
        # both streams join). Bitwise identical output — only scheduling
        # changes.
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        chains = []
        with timers.phase("graphs_walks_overlapped"):
            for group in (0, 1):
                streams[group].wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(streams[group]):
                    chains.append(chain(group))
            for st_ in streams:
                torch.cuda.current_stream().wait_stream(st_)
        walksets = []
        for group in (0, 1):
            with timers.phase(f"walks_g{group}"):
                walksets.append(_gather_walks(ctx, chains[group][1]))
    else:
        chains = [chain(0), chain(1)]
        walksets = [ws for _g, ws in chains]
    stats: Dict[str, float] = {f"nnz_g{group}": int(g.col_idx.numel())
                               for group, (g, _ws) in enumerate(chains)}
    with timers.phase("integrate"):
        ps, freq, n_in_paths = integrate_pathsets(walksets[0], walksets[1],
                                                  n_genes)
    stats["n_walks"] = int(walksets[0].nodes.shape[0] + walksets[1].nodes.shape[0])
    return ps, freq, n_in_paths, stats


@dataclasses.dataclass
class Study:
    """What steps 1-2 leave: the expression data of the genes it shares with
    the network, on the host and (the *_t tensors) on the run's device."""
    expr: np.ndarray            # f32 [n_samples, n_genes]
    labels: np.ndarray          # int64 [n_samples]: 0 good, 1 poor
    genes: Sequence[str]        # [n_genes]
    edge_idx: np.ndarray        # int32 [n_edges, 2], rows of `genes`
    device: torch.device

    def __post_init__(self):
        self.n_samples, self.n_genes = self.expr.shape
        self.n_edges = len(self.edge_idx)
        self.expr_t = torch.from_numpy(self.expr).to(self.device)
        self.labels_t = torch.from_numpy(self.labels).to(self.device)
        self.edge_idx_t = torch.from_numpy(self.edge_idx).to(self.device)

    @functools.cached_property
    def expr_f32(self) -> torch.Tensor:
        """expr_t as the step-6 kernels read it. Formed on first use: a run
        without device scores or ranks never has it."""
        return self.expr_t.float().contiguous()


def load_study(cfg: G2VecConfig, log=print, timers: Optional[PhaseTimers] = None,
               jsonl: Optional[JsonlLogger] = None) -> Study:
    """Steps 1-2: read the file triple and restrict it to the common genes."""
    timers, jsonl = timers or PhaseTimers(), jsonl or JsonlLogger()
    log(">>> 1. Load data")
    with timers.phase("load"):
        data = gio.load_expression(cfg.expression_file)
        clinical = gio.load_clinical(cfg.clinical_file)
        network = gio.load_network(cfg.network_file)

    log(">>> 2. Preprocess data")
    with timers.phase("preprocess"):
        data["label"] = pp.match_labels(clinical, data["sample"])
        common = pp.find_common_genes(network["gene"], data["gene"])
        network = pp.restrict_network(network, common)
        data = pp.restrict_data(data, common)
        edge_idx = pp.edges_to_indices(network["edge"], common)
    labels = np.asarray(data["label"])
    n_poor = int(np.sum(labels == 1))
    if min(n_poor, len(labels) - n_poor) < 2:
        # per-group PCC and the pooled t-statistic need >= 2 samples per
        # prognosis group; the reference nan-propagates here — fail loud
        raise ValueError(
            f"each prognosis group needs >= 2 samples: clinical file has "
            f"{len(labels) - n_poor} good / {n_poor} poor")
    study = Study(data["expr"], labels, data["gene"], edge_idx,
                  torch.device(resolve_device(cfg.device)))
    log("    n_samples: %d" % study.n_samples)
    log("    n_genes  : %d\t(common genes in both EXPRESSION and NETWORK)"
        % study.n_genes)
    log("    n_edges  : %d\t(edges with the common genes)" % study.n_edges)
    jsonl.emit("counts", n_samples=study.n_samples, n_genes=study.n_genes,
               n_edges=study.n_edges)
    return study


def random_paths(study, cfg, ctx, log, timers, jsonl):
    """Step 3: (pathset, gene_freq, n_genes_in_paths), cached or generated."""
    log("    *** most time consuming step ***")
    if cfg.corr != "pearson":
        log("    corr    : %s" % cfg.corr)
        jsonl.emit("corr", corr=cfg.corr)
    if cfg.load_paths:
        blob = torch.load(cfg.load_paths, map_location=study.device)
        ps = PathSet(blob["genes"], blob["offsets"], blob["labels"],
                     study.n_genes)
        freq, n_in_paths = blob["freq"], int(blob["n_in_paths"])
        stats = {}
    else:
        ps, freq, n_in_paths, stats = generate_paths(
            cfg, study.expr_t, study.labels_t, study.edge_idx_t,
            study.n_genes, ctx, log, timers)
        if cfg.save_paths and ctx.is_primary:
            torch.save({"genes": ps.genes, "offsets": ps.offsets,
                        "labels": ps.labels, "freq": freq,
                        "n_in_paths": n_in_paths}, cfg.save_paths)
    log("    n_paths : %d" % ps.n_paths)
    log("    n_genes : %d\t(genes in good or poor random paths)" % n_in_paths)
    jsonl.emit("paths", n_paths=ps.n_paths, n_genes_in_paths=n_in_paths, **stats)
    return ps, freq, n_in_paths


def train_models(study, cfg, ps, ctx, log, timers, jsonl):
    """Step 4: ([TrainResult per replica], the clock reading the `replicates`
    event counts from). One result without --replicates; replica 0 is the
    run without the flag."""
    n_genes, t0 = study.n_genes, time.perf_counter()
    if cfg.load_model:
        # resume from a --save-model checkpoint: skip training entirely
        # (steps 5-7 only need W_ih); shape metadata must match this run
        blob = torch.load(cfg.load_model, map_location="cpu")
        if int(blob["n_genes"]) != n_genes or int(blob["hidden"]) != cfg.hidden:
            raise ValueError(
                f"--load-model checkpoint was trained on n_genes="
                f"{blob['n_genes']}/hidden={blob['hidden']}, this run has "
                f"n_genes={n_genes}/hidden={cfg.hidden}")
        trained = [TrainResult(W_ih=blob["W_ih"].float(),
                               stop_epoch=int(blob.get("stop_epoch", -1)),
                               acc_val=float(blob.get("acc_val", float("nan"))),
                               acc_tr=float(blob.get("acc_tr", float("nan"))),
                               epochs_run=0, acc_val_history=[],
                               epoch_times_s=[], wall_to_acc_s=None)]
        log("    (loaded weights from %s; training skipped)" % cfg.load_model)
    elif cfg.replicates > 1:
        if ctx.world != 1:
            raise ValueError("replicates > 1 runs on one process; it "
                             f"conflicts with world size {ctx.world}")
        log("    replicates: %d" % cfg.replicates)
        with timers.phase("train"):
            trained = ReplicaTrainer(cfg, n_genes, study.device, log=log).train(
                ps, cfg.replicates)
    else:
        trainer = CbowTrainer(cfg, n_genes, study.device, ctx, log=log)
        with timers.phase("train"):
            trained = [trainer.train(ps)]
    res = trained[0]
    jsonl.emit("train", acc_val=res.acc_val, acc_tr=res.acc_tr,
               stop_epoch=res.stop_epoch, epochs_run=res.epochs_run,
               wall_to_acc088_s=res.wall_to_acc_s)
    if cfg.save_model and ctx.is_primary:
        torch.save({"W_ih": res.W_ih.float().cpu(),
                    "acc_val": res.acc_val, "acc_tr": res.acc_tr,
                    "stop_epoch": res.stop_epoch,
                    "hidden": cfg.hidden, "n_genes": n_genes,
                    "gene_index": list(map(str, study.genes))},
                   cfg.save_model)
    return trained, t0


class Steps56:
    """Steps 5-6 of one weight matrix, the package's only caller of
    find_lgroups, ops.row_norms and score_genes. Two calls, not one: a run
    prints between them (the silhouette line, the step-6 heading)."""

    def __init__(self, study: Study, cfg: G2VecConfig, W_ih: torch.Tensor,
                 W: Optional[np.ndarray] = None):
        """W: W_ih as a host f32 array, where the caller already has it."""
        self.study, self.cfg = study, cfg
        self.W = W if W is not None else W_ih.float().cpu().numpy()
        # the opt-in device backends read W_ih where it already lives (f32,
        # on the run's device): no host round trip. None without them.
        self.W_dev = None
        if cfg.kmeans_backend == "hip" or cfg.scoring_backend == "device":
            self.W_dev = W_ih.float().to(study.device).contiguous()

    def lgroups(self, freq: torch.Tensor, info: Dict) -> np.ndarray:
        """Step 5. info: the hip backend's inertia and iterations go here."""
        cfg = self.cfg
        return find_lgroups(
            self.W_dev if cfg.kmeans_backend == "hip" else self.W,
            freq.cpu().numpy(), cfg.compat_lgroup_bug,
            backend=cfg.kmeans_backend, device=self.study.device, info=info)

    def scores(self, lg: np.ndarray, expr_score, full: bool) -> Dict:
        """Step 6: the dict of scoring.score_genes. expr_score: (t_all,
        auc_all) of expression_scores. full: with the raw scores of the
        genes no L-group ranks, and auc: what the scores table needs."""
        st, (t_all, auc_all) = self.study, expr_score
        d_all = None
        if self.cfg.scoring_backend == "device":
            d_all = ops.row_norms(self.W_dev).cpu().numpy()
        out = scoring.score_genes(self.W, lg, st.expr, st.labels, st.genes,
                                  self.cfg.num_biomarker, d_all=d_all,
                                  t_all=t_all, rank_only=not full)
        if full and auc_all is not None:
            out["auc"] = auc_all
        return out


def expression_scores(study, cfg, log, jsonl):
    """(t_all, auc_all): step 6's expression score over all genes, decided
    here alone. t_all is None for the host t, which score_genes computes per
    L-group; auc_all is None unless score_stat is ranksum."""
    on_device = cfg.scoring_backend == "device"
    if cfg.score_stat == "ranksum":
        # |z| of the rank-sum test over all genes once, in place of the
        # t-scores; min-max, the sort and top-N do not change
        log("    score   : %s" % cfg.score_stat)
        if on_device:
            z_t, auc_t = ops.ranksum_scores(study.expr_f32, study.labels_t)
            both = z_t.cpu().numpy(), auc_t.cpu().numpy()
        else:
            both = scoring.ranksum_scores(study.expr, study.labels)
        jsonl.emit("score_stat", stat=cfg.score_stat,
                   backend=cfg.scoring_backend)
        return both
    if on_device:
        return ops.t_scores(study.expr_f32, study.labels_t).cpu().numpy(), None
    return None, None


def lgroup_silhouette(s56, lg, log, timers):
    """--silhouette under step 5: the dict of cluster_quality.silhouette, or
    None where fewer than two L-groups have genes."""
    with timers.phase("silhouette"):
        if int((np.bincount(np.asarray(lg, dtype=np.int64),
                            minlength=3) > 0).sum()) < 2:
            log("    silhouette: fewer than two non-empty L-groups, "
                "not defined")
            return None
        sil = silhouette(s56.W_dev if s56.W_dev is not None
                         else torch.from_numpy(s56.W).to(s56.study.device),
                         lg, k=3)
        log("    silhouette: mean %.4f (good %.4f, poor %.4f, other %.4f)"
            % ((sil["mean"],) + tuple(sil["mean_by_cluster"])))
        return sil


def add_silhouette_columns(scores, sil, timers, jsonl):
    """--silhouette under step 6: its two columns of the scores table (NA
    where sil is None) and its event."""
    scores["silhouette"] = None if sil is None else sil["s"]
    scores["nearest_lgroup"] = None if sil is None else sil["nearest"]
    if sil is not None:
        sel = np.asarray(scores["is_biomarker"]).astype(bool)
        jsonl.emit("silhouette", mean=sil["mean"],
                   mean_by_lgroup=[float(v) for v in sil["mean_by_cluster"]],
                   mean_biomarkers=(float(sil["s"][sel].mean())
                                    if sel.any() else float("nan")),
                   n_negative=int((sil["s"] < 0).sum()),
                   seconds=timers.times["silhouette"])


def replicate_stability(study, cfg, freq, trained, first, expr_score, t0,
                        timers, jsonl):
    """--replicates: steps 5-6 once more per further replica, through the
    same calls and backends, then the stability summary over all of them.
    first: replica 0's (L-groups, scores). The expression scores do not
    depend on the weights, so one vector serves every replica."""
    with timers.phase("replicates_steps56"):
        t_once = expr_score[0] if expr_score[0] is not None else \
            scoring.t_scores(study.expr, study.labels)
        each = [first]
        for rr in trained[1:]:
            s56 = Steps56(study, cfg, rr.W_ih)
            lg_r = s56.lgroups(freq, {})
            each.append((lg_r, s56.scores(lg_r, (t_once, None), full=False)))
        stab = stability.summarize(
            np.stack([lg for lg, _sc in each]),
            np.stack([sc["is_biomarker"] for _lg, sc in each]),
            np.stack([sc["gene_score"] for _lg, sc in each]),
            cfg.num_biomarker)
    jsonl.emit("replicates", R=cfg.replicates,
               stop_epochs=[r.stop_epoch for r in trained],
               acc_val=[r.acc_val for r in trained],
               acc_tr=[r.acc_tr for r in trained],
               jaccard=stab["jaccard"], seconds=time.perf_counter() - t0)
    return stab


def permutation_table(study, cfg, timers, jsonl):
    """--permutations: label-permutation p-values of the expression score."""
    seed = cfg.perm_seed if cfg.perm_seed is not None else _run_seed(cfg)
    with timers.phase("permutations"):
        x = study.expr
        if cfg.score_stat == "ranksum":
            # the pooled t^2 of the ranks is monotone in |W1 - E W1|, so
            # the same null gives the exact permutation rank-sum p-value
            x = ops.rank_columns(study.expr_f32).cpu().numpy()
        perm = scoring.permutation_pvalues(x, study.labels, cfg.permutations,
                                           seed, device=study.device)
    jsonl.emit("perm", B=cfg.permutations, seed=seed,
               seconds=timers.times["permutations"],
               n_q05=int(np.sum(perm["q_bh"] <= 0.05)))
    return perm


def neighbor_table(study, cfg, s56, biomarkers, timers, jsonl):
    """--neighbors: (query rows, neighbour rows, similarities) of the K
    nearest genes of every query gene."""
    if cfg.neighbors_of == "all":
        q = np.arange(study.n_genes, dtype=np.int64)
    else:
        row_of = {str(g): i for i, g in enumerate(study.genes)}
        q = np.array([row_of[str(b)] for b in biomarkers], dtype=np.int64)
    with timers.phase("neighbors"):
        idx, sim = nearest_genes(
            s56.W_dev if s56.W_dev is not None else s56.W, q, cfg.neighbors,
            metric="cosine", device=study.device)
    jsonl.emit("neighbors", Q=int(q.size), k=cfg.neighbors,
               seconds=timers.times["neighbors"])
    return q, idx, sim


def write_results(study, cfg, W, lg, scores, perm, nbr, stab, log):
    """Step 7: the standard triple, then one file per opt-in table."""
    name, genes, biomarkers = cfg.result_name, study.genes, scores["biomarkers"]
    log("    %s" % gio.write_biomarkers(name, biomarkers))
    log("    %s" % gio.write_lgroups(name, lg, genes))
    log("    %s" % gio.write_vectors(name, W, genes))
    if cfg.write_scores:
        log("    %s" % gio.write_scores(name, genes, lg, scores, perm))
    if nbr is not None:
        log("    %s" % gio.write_neighbors(name, genes, *nbr, lg, biomarkers))
    if stab is not None:
        log("    %s" % gio.write_stability(name, genes, stab))
        log("    %s" % gio.write_consensus(name, genes, stab))


def run(cfg: G2VecConfig, ctx: Optional[DistContext] = None) -> Dict:
    cfg.validate()
    ctx = ctx or single(torch.device(resolve_device(cfg.device)))
    log = print if ctx.is_primary else (lambda *a, **k: None)
    # closed on every way out: a run that raises leaves a complete file
    with contextlib.closing(
            JsonlLogger(cfg.log_jsonl if ctx.is_primary else "")) as jsonl:
        timers = PhaseTimers(jsonl)
        log(">>> 0. Arguments")
        log("    " + str(cfg))
        study = load_study(cfg, log, timers, jsonl)     # >>> 1. and >>> 2.
        log(">>> 3. Generate random paths from each group")
        ps, freq, n_in_paths = random_paths(study, cfg, ctx, log, timers, jsonl)
        log(">>> 4. Compute distributed representations using modified CBOW")
        trained, t0 = train_models(study, cfg, ps, ctx, log, timers, jsonl)
        res = trained[0]
        result: Dict = {
            "n_samples": study.n_samples, "n_genes": study.n_genes,
            "n_edges": study.n_edges, "n_paths": ps.n_paths,
            "n_genes_in_paths": n_in_paths,
            "acc_val": res.acc_val, "acc_tr": res.acc_tr,
            "stop_epoch": res.stop_epoch,
            "W_ih": res.W_ih.float().cpu().numpy(),
            "timers": timers.summary(), "genes": study.genes,
        }
        if not ctx.is_primary:
            return result

        s56 = Steps56(study, cfg, res.W_ih, result["W_ih"])
        log(">>> 5. Find L-groups")
        km_info: Dict = {}
        with timers.phase("lgroups"):
            lg = s56.lgroups(freq, km_info)
        if km_info:
            jsonl.emit("kmeans", backend=cfg.kmeans_backend, **km_info)
        sil = (lgroup_silhouette(s56, lg, log, timers) if cfg.silhouette
               else None)
        log(">>> 6. Select biomarkers with gene scores")
        with timers.phase("scoring"):
            expr_score = expression_scores(study, cfg, log, jsonl)
            scores = s56.scores(lg, expr_score, full=cfg.write_scores)
            if cfg.silhouette:
                add_silhouette_columns(scores, sil, timers, jsonl)
        stab = perm = nbr = None
        if cfg.replicates > 1:
            stab = replicate_stability(study, cfg, freq, trained, (lg, scores),
                                       expr_score, t0, timers, jsonl)
        if cfg.permutations > 0:
            perm = permutation_table(study, cfg, timers, jsonl)
        if cfg.neighbors > 0:
            nbr = neighbor_table(study, cfg, s56, scores["biomarkers"],
                                 timers, jsonl)
        log(">>> 7. Save results")
        with timers.phase("write"):
            write_results(study, cfg, s56.W, lg, scores, perm, nbr, stab, log)

        if stab is not None:
            result["stability"] = stab
        result.update({"lgroups": lg, "biomarkers": scores["biomarkers"],
                       "timers": timers.summary()})
        jsonl.emit("done", **{k: v for k, v in result.items()
                              if isinstance(v, (int, float, str))})
        return result
