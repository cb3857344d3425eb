"""Biomarker scoring (reference step 6, G2Vec.py:85-157). Host-side NumPy;
with scoring_backend="device" the two [G] score vectors come from the
row_norms / t_scores kernels (ops) and only the ranking runs here."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np


def transform_minmax(scores: np.ndarray, lo: float = 0.0, hi: float = 1.0
                     ) -> np.ndarray:
    """Min-max rescale (G2Vec.py:133-136). Guard: constant input -> zeros
    (the reference divides by zero there)."""
    old_min, old_max = float(scores.min()), float(scores.max())
    if old_max <= old_min:
        return np.zeros_like(scores)
    return (hi - lo) / (old_max - old_min) * (scores - old_min) + lo


def t_statistic(x: np.ndarray, y: np.ndarray) -> float:
    """Pooled-variance two-sample t (ddof=1 stds; 0 on zero denominators),
    G2Vec.py:138-149."""
    nx, ny = len(x), len(y)
    if nx < 2 or ny < 2:
        return 0.0
    sx, sy = x.std(ddof=1), y.std(ddof=1)
    d1 = np.sqrt(((nx - 1.0) * sx * sx + (ny - 1.0) * sy * sy) / (nx + ny - 2.0))
    d2 = np.sqrt(1.0 / nx + 1.0 / ny)
    if d1 > 0.0 and d2 > 0.0:
        return float((x.mean() - y.mean()) / d1 / d2)
    return 0.0


def t_scores(expr: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """|t| per gene column, good (label 0) vs poor (label 1) samples
    (G2Vec.py:151-157). Vectorized over genes; `t_statistic` is the scalar
    oracle it is tested against."""
    good = expr[labels == 0].astype(np.float64)
    poor = expr[labels == 1].astype(np.float64)
    nx, ny = good.shape[0], poor.shape[0]
    if nx < 2 or ny < 2:
        return np.zeros(expr.shape[1], dtype=np.float32)
    sx = good.std(axis=0, ddof=1)
    sy = poor.std(axis=0, ddof=1)
    d1 = np.sqrt(((nx - 1.0) * sx * sx + (ny - 1.0) * sy * sy) / (nx + ny - 2.0))
    d2 = np.sqrt(1.0 / nx + 1.0 / ny)
    diff = good.mean(axis=0) - poor.mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d1 > 0.0, diff / np.where(d1 > 0, d1, 1.0) / d2, 0.0)
    return np.abs(t).astype(np.float32)


def average_ranks(x: np.ndarray) -> np.ndarray:
    """f64 [S, G] average ranks (1-based; ties share the mean of their
    positions) of every element within its column of x [S, G]."""
    x = np.asarray(x)
    S = x.shape[0]
    order = np.argsort(x, axis=0, kind="stable")
    xs = np.take_along_axis(x, order, axis=0)
    # a run of equal values shares the mean of its first and last position
    start = np.ones(xs.shape, dtype=bool)
    start[1:] = xs[1:] != xs[:-1]
    stop = np.ones(xs.shape, dtype=bool)
    stop[:-1] = start[1:]
    pos = np.arange(1, S + 1, dtype=np.float64)[:, None]
    first = np.maximum.accumulate(np.where(start, pos, 1.0), axis=0)
    last = np.minimum.accumulate(
        np.where(stop, pos, float(S))[::-1], axis=0)[::-1]
    ranks = np.empty(xs.shape, dtype=np.float64)
    np.put_along_axis(ranks, order, 0.5 * (first + last), axis=0)
    return ranks


def ranksum_scores(expr: np.ndarray, labels: np.ndarray):
    """(|z|, auc) f32 [G]: Wilcoxon rank-sum test of the poor (label 1)
    against the good (label 0) samples per gene column; other labels are
    left out. Normal approximation with the tie-corrected variance and no
    continuity correction:
        z = (W1 - n1 (S+1)/2) / sqrt(n1 n0 / (S (S-1)) * SSR)
    W1 = the poor group's rank sum, SSR = sum (rank - (S+1)/2)^2, and
    auc = (W1 - n1 (n1+1)/2) / (n1 n0) = U / (n1 n0). z = 0 and auc = 0.5
    for a constant gene or a group of fewer than 2 samples (the rule of
    t_scores). Host f64; ops.ranksum_scores is the device counterpart."""
    labels = np.asarray(labels)
    keep = (labels == 0) | (labels == 1)
    x = np.asarray(expr)[keep]
    m = labels[keep] == 1
    S, G = x.shape
    n1 = int(m.sum())
    n0 = S - n1
    z = np.zeros(G, dtype=np.float64)
    auc = np.full(G, 0.5, dtype=np.float64)
    if n1 < 2 or n0 < 2:
        return z.astype(np.float32), auc.astype(np.float32)
    r = average_ranks(x)
    W1 = r[m].sum(axis=0)
    SSR = ((r - 0.5 * (S + 1.0)) ** 2).sum(axis=0)
    live = SSR > 0.0
    var = n1 * n0 / (S * (S - 1.0)) * SSR[live]
    z[live] = np.abs(W1[live] - 0.5 * n1 * (S + 1.0)) / np.sqrt(var)
    auc[live] = (W1[live] - 0.5 * n1 * (n1 + 1.0)) / (float(n1) * n0)
    return z.astype(np.float32), auc.astype(np.float32)


def select_biomarkers(embeddings: np.ndarray, lgroup_idx: np.ndarray,
                      expr: np.ndarray, labels: np.ndarray,
                      genes: Sequence[str], num_biomarker: int,
                      d_all: Optional[np.ndarray] = None,
                      t_all: Optional[np.ndarray] = None) -> List[str]:
    """Top-N per L-group by gene score = 0.5*(minmax d-score + minmax t-score),
    union sorted (G2Vec.py:85-109).
    d_all / t_all: optional precomputed f32 [G] d-scores (embedding row
    norms) and t-scores over ALL genes; each L-group indexes them in place
    of computing its own. Both scores are per-gene, so min-max, ranking and
    top-N are the same arithmetic either way."""
    return score_genes(embeddings, lgroup_idx, expr, labels, genes,
                       num_biomarker, d_all=d_all, t_all=t_all,
                       rank_only=True)["biomarkers"]


def score_genes(embeddings: np.ndarray, lgroup_idx: np.ndarray,
                expr: np.ndarray, labels: np.ndarray,
                genes: Sequence[str], num_biomarker: int,
                d_all: Optional[np.ndarray] = None,
                t_all: Optional[np.ndarray] = None,
                rank_only: bool = False) -> Dict:
    """The selection of `select_biomarkers` together with the numbers it was
    made from: {"biomarkers": sorted names, "d_score" / "t_score": raw [G]
    values, "gene_score": f64 [G] within-L-group 0.5*(minmax d + minmax t),
    NaN outside L-groups 0 and 1, "is_biomarker": bool [G]}.
    rank_only: skip the raw scores of the genes no L-group ranks."""
    genes = np.asarray(genes)
    n = len(genes)
    d_raw = np.zeros(n, dtype=np.float64)
    t_raw = np.zeros(n, dtype=np.float64)
    gene_score = np.full(n, np.nan, dtype=np.float64)
    chosen = np.zeros(n, dtype=bool)
    result: List[str] = []
    for grp in (0, 1):      # 0 good, 1 poor
        sel = lgroup_idx == grp
        if not sel.any():
            continue
        mat = embeddings[sel]
        sub_genes = genes[sel]
        sub_expr = expr[:, sel]
        d_sub = (np.linalg.norm(mat, axis=1) if d_all is None
                 else d_all[sel])
        t_sub = (t_scores(sub_expr, labels) if t_all is None
                 else t_all[sel])
        d = transform_minmax(d_sub)
        t = transform_minmax(t_sub)
        score = 0.5 * (d + t)
        # stable sort desc by score (reference: Python sorted, stable)
        order = np.argsort(-score, kind="stable")[:num_biomarker]
        result += sorted(sub_genes[order].tolist())
        idx = np.flatnonzero(sel)
        d_raw[idx], t_raw[idx], gene_score[idx] = d_sub, t_sub, score
        chosen[idx[order]] = True
    rest = ~np.isin(lgroup_idx, (0, 1))
    if rest.any() and not rank_only:    # the genes no L-group ranks
        d_raw[rest] = (np.linalg.norm(embeddings[rest], axis=1)
                       if d_all is None else d_all[rest])
        t_raw[rest] = (t_scores(expr[:, rest], labels) if t_all is None
                       else t_all[rest])
    return {"biomarkers": sorted(result), "d_score": d_raw, "t_score": t_raw,
            "gene_score": gene_score, "is_biomarker": chosen}


# ------------------------------------------------ label-permutation p-values
def perm_masks(labels: np.ndarray, B: int, seed: int) -> np.ndarray:
    """u8 [B, S] random relabellings that keep the group sizes: row b gives
    label 1 to the n1 = #(labels == 1) samples with the smallest keys, key
    (b, s) being one draw of the splitmix64 stream keyed on (seed, b, s) and
    warmed by one draw like the walk and init streams; ties go by sample
    order (stable sort). Host code for CPU and GPU runs alike."""
    from .ops.cpu_ref import _SM64_M2, splitmix64_vec
    labels = np.asarray(labels)
    S = labels.shape[0]
    n1 = int(np.sum(labels == 1))
    if B < 1:
        raise ValueError("perm_masks needs B >= 1")
    masks = np.zeros((B, S), dtype=np.uint8)
    s_idx = np.arange(S, dtype=np.uint64)
    step = max(1, (1 << 22) // max(S, 1))
    for lo in range(0, B, step):
        b_idx = np.arange(lo, min(B, lo + step), dtype=np.uint64)
        gid = (b_idx[:, None] << np.uint64(32)) | s_idx[None, :]
        state = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) ^ (
            gid * _SM64_M2 + np.uint64(1))
        state, _ = splitmix64_vec(state)            # warm draw
        _, key = splitmix64_vec(state)
        order = np.argsort(key, axis=1, kind="stable")[:, :n1]
        np.put_along_axis(masks[lo:lo + len(b_idx)], order, 1, axis=1)
    return masks


def bh_adjust(p: np.ndarray) -> np.ndarray:
    """Benjamini-Hochberg q-values over all of p, made monotone in p (the
    running minimum from the largest p down), capped at 1."""
    p = np.asarray(p, dtype=np.float64)
    n = p.shape[0]
    if n == 0:
        return p.copy()
    order = np.argsort(p, kind="stable")
    q = p[order] * n / np.arange(1, n + 1, dtype=np.float64)
    q = np.minimum(np.minimum.accumulate(q[::-1])[::-1], 1.0)
    out = np.empty(n, dtype=np.float64)
    out[order] = q
    return out


def permutation_pvalues(expr: np.ndarray, labels: np.ndarray, B: int,
                        seed: int, device="cpu", chunk: int = 8192) -> Dict:
    """Label-permutation null of the pooled two-sample t, per gene column of
    expr [S, G] (labels 0 good / 1 poor), over the B relabellings of
    `perm_masks(labels, B, seed)`. Returns f64 [G] arrays:
      t_obs   |t| of the observed labelling (sqrt of the kernel's t^2)
      p       (1 + #{b : t2[b, g] exceeds}) / (1 + B)
      q_bh    Benjamini-Hochberg over all genes
      p_maxT  (1 + #{b : max_g t2[b, g] exceeds}) / (1 + B), the single-step
              Westfall-Young adjustment
    "exceeds" is >= stat_obs[g] * (1 - 2^-30). A gene whose pooled variance
    is <= 0 (constant inside both groups) has t_obs = 0 and p = 1. The
    masks are walked `chunk` rows at a time; the counts are integers, so the
    result does not depend on chunk."""
    import torch

    from . import ops
    from .ops.cpu_ref import PERM_TIE
    if B < 1:
        raise ValueError("permutation_pvalues needs B >= 1")
    if chunk < 1:
        raise ValueError("chunk must be >= 1")
    labels = np.asarray(labels)
    x = np.asarray(expr, dtype=np.float64)
    # t is shift-invariant; centred columns keep q - s*s/n from cancelling
    x32 = np.ascontiguousarray((x - x.mean(axis=0)).astype(np.float32))
    dev = torch.device(device)
    expr_t = torch.from_numpy(x32).to(dev)
    obs = torch.from_numpy(
        np.ascontiguousarray((labels == 1).astype(np.uint8))[None, :]).to(dev)
    stat_obs = ops.perm_t_stats(expr_t, obs)[0].contiguous()
    moments = ops.col_moments(expr_t) if expr_t.is_cuda else None
    G = x32.shape[1]
    counts = np.zeros(G, dtype=np.int64)
    maxstat = np.empty(B, dtype=np.float64)
    masks = perm_masks(labels, B, seed)
    for lo in range(0, B, chunk):
        m = torch.from_numpy(masks[lo:lo + chunk]).to(dev)
        c, mx = ops.perm_t_counts(expr_t, m, stat_obs, moments=moments)
        counts += c.cpu().numpy()
        maxstat[lo:lo + chunk] = mx.cpu().numpy()
    so = stat_obs.cpu().numpy()
    p = (1.0 + counts) / (1.0 + B)
    ms = np.sort(maxstat)
    n_ge = B - np.searchsorted(ms, so * PERM_TIE, side="left")
    return {"t_obs": np.sqrt(so), "p": p, "q_bh": bh_adjust(p),
            "p_maxT": (1.0 + n_ge) / (1.0 + B), "stat_obs": so,
            "counts": counts, "maxstat": maxstat}
