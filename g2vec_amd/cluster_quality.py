"""How good is a clustering of the embedding: per-gene silhouettes.

silhouette(W, labels) is the statistic of Rousseeuw (1987), the
`silhouette_samples` of scikit-learn, with exact Euclidean distances over all
G^2 pairs. The pairs are never held: ops.cluster_dist_sums streams them (a
fused MFMA GEMM + per-cluster distance sums on the GPU, a blocked torch
mirror on the CPU) and returns one f64 distance sum per (gene, cluster), from
which everything here follows in f64 on the host.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import ops

# The launch split silhouette() asks of the GPU op is a function of G alone:
# a block walks at least SIL_WALK candidate tiles of 64, and at most SIL_GY
# blocks share a query tile (one resident set of the tile kernel at two
# query tiles). The f64 addition order follows the split, so a rule that
# looked at the number of queries would let a gene's silhouette depend on
# which other genes were asked with it.
SIL_WALK = 16
SIL_GY = 384
SIL_PART_BYTES = 1 << 28        # partial buffer [chunk, gy, k] f64 per call


def sil_grid_y(G: int) -> int:
    return max(1, min(SIL_GY, ((G + 63) // 64) // SIL_WALK))


def silhouette_from_sums(D: np.ndarray, own: np.ndarray,
                         n_c: np.ndarray) -> Dict[str, np.ndarray]:
    """(s, a, b, nearest) from D f64 [Q, k] (distance sums of each query to
    every cluster, itself excluded), own [Q] (the query's cluster) and n_c
    [k] (cluster sizes over all genes):
        a = D[i, A] / (n_A - 1)
        b = min over c != A with n_c > 0 of D[i, c] / n_c   (lowest c on ties)
        s = (b - a) / max(a, b);  s = 0 if n_A == 1 or max(a, b) == 0."""
    D = np.asarray(D, dtype=np.float64)
    own = np.asarray(own, dtype=np.int64)
    n_c = np.asarray(n_c, dtype=np.int64)
    Q, k = D.shape
    rows = np.arange(Q)
    n_own = n_c[own]
    a = np.where(n_own > 1, D[rows, own] / np.maximum(n_own - 1, 1), 0.0)
    other = np.where(n_c[None, :] > 0, D / np.maximum(n_c, 1)[None, :], np.inf)
    other[rows, own] = np.inf
    nearest = other.argmin(axis=1)              # the first minimum
    b = other[rows, nearest]
    m = np.maximum(a, b)
    live = (n_own > 1) & (m > 0)
    s = np.where(live, (b - a) / np.where(live, m, 1.0), 0.0)
    return dict(s=s, a=a, b=b, nearest=nearest.astype(np.int32))


def silhouette(W, labels, k: int = 3, rows=None, device="cpu",
               q_chunk: int = 65536) -> Dict:
    """Silhouettes of the rows of W [G, h] (NumPy array or torch tensor; a
    tensor is used in place on its device) under labels [G] in [0, k).

    The f64 column mean of W is subtracted before the f32 cast: distances
    do not change under a shift, and centred rows cut the cancellation in
    nq + nx - 2 dot. rows selects the query genes (default: all); a query
    always excludes itself. Queries are walked q_chunk at a time and the
    result does not depend on q_chunk.

    Returns dict(s, a, b f64 [Q]; nearest i32 [Q], the closest other
    cluster; mean_by_cluster f64 [k] over the queried rows, NaN for a
    cluster none of them lies in; mean). Raises ValueError when fewer than
    two clusters are non-empty."""
    if not 1 <= int(k) <= ops.CDS_K_MAX:
        raise ValueError(f"k must be in [1, {ops.CDS_K_MAX}], got {k}")
    k = int(k)
    if q_chunk < 1:
        raise ValueError("q_chunk must be >= 1")
    if isinstance(W, torch.Tensor):
        Wt = W.detach()
        dev = Wt.device
    else:
        Wt = torch.from_numpy(np.asarray(W))
        dev = torch.device(device)
    if Wt.dim() != 2:
        raise ValueError("W must be a [G, h] matrix")
    G = Wt.shape[0]
    lab = np.asarray(labels.cpu() if isinstance(labels, torch.Tensor)
                     else labels)
    if lab.shape != (G,) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError("labels must be an integer [G] array")
    lab = lab.astype(np.int64)
    bad = np.nonzero((lab < 0) | (lab >= k))[0]
    if bad.size:
        raise ValueError(f"labels must lie in [0, {k}): labels[{bad[0]}] = "
                         f"{lab[bad[0]]}")
    n_c = np.bincount(lab, minlength=k)
    if int((n_c > 0).sum()) < 2:
        raise ValueError("the silhouette needs at least two non-empty "
                         f"clusters, sizes are {n_c.tolist()}")
    if rows is None:
        q = np.arange(G, dtype=np.int64)
    else:
        q = np.asarray(rows.cpu() if isinstance(rows, torch.Tensor) else rows)
        if q.ndim != 1 or (q.size and not np.issubdtype(q.dtype, np.integer)):
            raise ValueError("rows must be a 1-D integer array of row indices")
        q = q.astype(np.int64)
        if q.size and (q.min() < 0 or q.max() >= G):
            raise ValueError(f"rows must lie in [0, {G})")
    Wd = Wt.to(device=dev, dtype=torch.float64)
    if not bool(torch.isfinite(Wd).all()):
        raise ValueError("W must be finite")
    X = (Wd - Wd.mean(dim=0)).float().contiguous()
    del Wd
    lab_t = torch.from_numpy(lab.astype(np.int32)).to(dev)
    gy = sil_grid_y(G)
    step = min(q_chunk, max(64, SIL_PART_BYTES // (gy * k * 8) // 64 * 64))
    D = np.empty((q.size, k), dtype=np.float64)
    for lo in range(0, q.size, step):
        qi = torch.from_numpy(q[lo:lo + step]).to(dev)
        D[lo:lo + step] = ops.cluster_dist_sums(
            X[qi].contiguous(), X, lab_t, k, q_index=qi.int(),
            grid_y=gy).cpu().numpy()
    out: Dict = silhouette_from_sums(D, lab[q], n_c)
    own = lab[q]
    by = np.full(k, np.nan, dtype=np.float64)
    for c in range(k):
        if (own == c).any():
            by[c] = out["s"][own == c].mean()
    out["mean_by_cluster"] = by
    out["mean"] = float(out["s"].mean()) if q.size else float("nan")
    return out
