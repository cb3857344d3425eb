"""Nearest genes in the embedding: the `most_similar` of a gene2vec output.

nearest_genes(W, queries, k) answers "which genes lie closest to these?"
for rows of the trained W_ih without ever forming W W^T: the scores are
streamed through ops.knn_topk (fused MFMA GEMM + top-k on the GPU, a blocked
torch mirror on the CPU) and only the k best per query are kept.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import ops

METRICS = ("cosine", "dot")


def unit_rows(W: torch.Tensor) -> torch.Tensor:
    """Rows of W f32 [G, h] scaled to unit length: f64 norm, W / norm in f32.
    A zero row stays zero (its cosine with everything is 0)."""
    norm = W.double().pow(2).sum(dim=1).sqrt().float()
    norm = torch.where(norm > 0, norm, torch.ones_like(norm))
    return W / norm[:, None]


def nearest_genes(W, queries, k: int, metric: str = "cosine",
                  device="cpu", q_chunk: int = 65536
                  ) -> Tuple[np.ndarray, np.ndarray]:
    """(idx int32 [Q, k], sim float32 [Q, k]): for every query (a row index of
    W [G, h], NumPy array or torch tensor) its k most similar other rows,
    best first; equal similarities by ascending row index. metric "cosine"
    normalises the rows once, "dot" uses W as is. A query never returns
    itself; with k > G - 1 the tail is idx -1, sim -inf. Queries are walked
    q_chunk at a time to bound the kernel's partial buffer; the result does
    not depend on q_chunk."""
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    if not 1 <= int(k) <= 64:
        raise ValueError(f"k must be in [1, 64], got {k}")
    if q_chunk < 1:
        raise ValueError("q_chunk must be >= 1")
    dev = torch.device(device)
    Wt = W if isinstance(W, torch.Tensor) else torch.from_numpy(np.asarray(W))
    if Wt.dim() != 2:
        raise ValueError("W must be a [G, h] matrix")
    Wt = Wt.detach().to(device=dev, dtype=torch.float32).contiguous()
    if not bool(torch.isfinite(Wt).all()):
        raise ValueError("W must be finite")
    G = Wt.shape[0]
    q = np.asarray(queries.cpu() if isinstance(queries, torch.Tensor)
                   else queries)
    if q.ndim != 1 or (q.size and not np.issubdtype(q.dtype, np.integer)):
        raise ValueError("queries must be a 1-D integer array of row indices")
    q = q.astype(np.int64)
    if q.size and (q.min() < 0 or q.max() >= G):
        raise ValueError(f"queries must lie in [0, {G})")
    X = unit_rows(Wt) if metric == "cosine" else Wt
    k = int(k)
    idx = np.empty((q.size, k), dtype=np.int32)
    sim = np.empty((q.size, k), dtype=np.float32)
    for lo in range(0, q.size, q_chunk):
        qi = torch.from_numpy(q[lo:lo + q_chunk]).to(dev)
        i, v = ops.knn_topk(X[qi].contiguous(), X, k, q_index=qi.int())
        idx[lo:lo + q_chunk] = i.cpu().numpy()
        sim[lo:lo + q_chunk] = v.cpu().numpy()
    return idx, sim
