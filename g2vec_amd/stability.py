"""Stability of the biomarker selection over R replicates (--replicates R):
which genes survive a change of the initialisation seed. Pure NumPy on the
per-replica results of steps 5-6; nothing here touches a device."""
from __future__ import annotations

from typing import Dict

import numpy as np


def mean_pairwise_jaccard(selected: np.ndarray) -> float:
    """Mean |A & B| / |A | B| over all pairs of rows of selected bool [R, G]
    (two empty sets count as 1); 1.0 when there is no pair."""
    sel = np.asarray(selected, dtype=bool)
    R = sel.shape[0]
    vals = []
    for a in range(R):
        for b in range(a + 1, R):
            union = int(np.sum(sel[a] | sel[b]))
            inter = int(np.sum(sel[a] & sel[b]))
            vals.append(inter / union if union else 1.0)
    return float(np.mean(vals)) if vals else 1.0


def summarize(lgroups: np.ndarray, selected: np.ndarray,
              gene_scores: np.ndarray, num_biomarker: int) -> Dict:
    """Per-gene summary of R replicates.

    lgroups      int [R, G]   L-group of every gene per replica
    selected     bool [R, G]  gene is in the replica's biomarker list
    gene_scores  f64 [R, G]   within-L-group gene score, NaN where the
                              replica defines none (gene outside L-groups
                              0 and 1)

    Returns arrays over genes: lgroup (replica 0's), lgroup_mode (most
    frequent L-group, ties to the lowest id), lgroup_agreement (share of
    replicas equal to the mode), selected (count), frequency (count / R),
    mean_gene_score (mean over the replicas where it is defined, NaN if
    never); consensus: the indices of the num_biomarker genes with the
    highest count, ties by higher mean_gene_score (NaN last), then by lower
    gene index, best first; jaccard: mean pairwise Jaccard index of the R
    biomarker sets."""
    lg = np.asarray(lgroups, dtype=np.int64)
    sel = np.asarray(selected, dtype=bool)
    gs = np.asarray(gene_scores, dtype=np.float64)
    if lg.ndim != 2 or sel.shape != lg.shape or gs.shape != lg.shape:
        raise ValueError("lgroups, selected and gene_scores must be [R, G]")
    if lg.size and lg.min() < 0:
        raise ValueError("L-group ids must be >= 0")
    R, G = lg.shape
    n_ids = int(lg.max()) + 1 if lg.size else 1
    votes = np.stack([(lg == k).sum(axis=0) for k in range(n_ids)])  # [ids, G]
    mode = votes.argmax(axis=0)              # argmax: first = lowest id
    agreement = votes.max(axis=0) / float(R)
    count = sel.sum(axis=0).astype(np.int64)
    defined = ~np.isnan(gs)
    n_def = defined.sum(axis=0)
    total = np.where(defined, gs, 0.0).sum(axis=0)
    mean_gs = np.full(G, np.nan)
    np.divide(total, n_def, out=mean_gs, where=n_def > 0)
    # lexsort: last key first; NaN scores sort after every defined one
    score_key = np.where(np.isnan(mean_gs), np.inf, -mean_gs)
    order = np.lexsort((np.arange(G), score_key, -count))
    return {"lgroup": lg[0].copy(), "lgroup_mode": mode,
            "lgroup_agreement": agreement, "selected": count,
            "frequency": count / float(R), "mean_gene_score": mean_gs,
            "consensus": order[:max(int(num_biomarker), 0)],
            "jaccard": mean_pairwise_jaccard(sel), "R": R}
