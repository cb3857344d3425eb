"""Per-group graph construction: PCC edge weights + CSR build.

Reference builds a dense G x G adjacency per prognosis group with
weight = |PCC| over that group's samples, kept iff > 0.5, directed
src->dest (G2Vec.py:370-391). Dense G^2 does not scale (4 TB at 1M genes),
so this module builds a CSR graph instead:

  - z-score each gene over the group's samples (std==0 -> zero row,
    reproducing the pcc=0 rule of G2Vec.py:356-367)
  - PCC per edge: either a per-edge dot kernel (default; scales to 100M
    edges) or the MFMA f32 correlation GEMM (dense-output path for graphs
    whose G^2 fits HBM — 288 GB on MI355X)
  - threshold + CSR assembly with torch ops (device-resident)
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import ops


class CsrGraph(NamedTuple):
    row_ptr: torch.Tensor   # i32 [G+1]
    col_idx: torch.Tensor   # i32 [nnz]
    weights: torch.Tensor   # f32 [nnz]
    n_nodes: int


CORR_KINDS = ("pearson", "spearman")


def zscore_group(expr: torch.Tensor, labels: torch.Tensor, group: int,
                 corr: str = "pearson") -> torch.Tensor:
    """f32 [G, S_group] z-scored transposed expression for one group.
    std is population std (ddof=0) to match np.ndarray.std() in G2Vec.py:356.
    corr="spearman": the group's rows are replaced by their within-group
    average ranks first (ops.rank_columns), so every correlation downstream
    is Spearman's rho, ties included."""
    if corr not in CORR_KINDS:
        raise ValueError(f"corr must be pearson|spearman, got {corr}")
    X = expr[labels == group].float()          # [Sg, G]
    if corr == "spearman" and X.shape[0] > 0:
        X = ops.rank_columns(X.contiguous())
    mean = X.mean(dim=0)
    std = X.std(dim=0, unbiased=False)
    z = (X - mean) / torch.where(std > 0, std, torch.ones_like(std))
    z = torch.where(std[None, :] > 0, z, torch.zeros_like(z))
    return z.t().contiguous()                  # [G, Sg]


def edge_pcc_weights(zt: torch.Tensor, edge_idx: torch.Tensor,
                     mode: str = "auto") -> torch.Tensor:
    """|PCC| per directed edge. mode: 'edge' | 'gemm' | 'auto'."""
    G = zt.shape[0]
    n_group = zt.shape[1]
    if mode == "auto":
        # small G: the MFMA f32 corr GEMM computes all G^2 correlations in
        # ~0.1 ms and the dense C fits trivially in 288 GB HBM; large G:
        # the per-edge dot kernel is the only thing that scales (1M genes
        # -> a 4 TB dense C)
        dense_bytes = 4 * G * G
        mode = "gemm" if (zt.is_cuda and dense_bytes <= 2 << 30 and
                          n_group <= 288) else "edge"
    if mode == "gemm":
        C = ops.corr_gemm(zt, n_group)
        return C[edge_idx[:, 0].long(), edge_idx[:, 1].long()].abs()
    return ops.pcc_edges(zt, edge_idx, n_group)


def dedupe_edges(edge_idx: torch.Tensor, n_genes: int) -> torch.Tensor:
    """Unique directed edges as i32 [E,2] (the dense adjMat overwrites
    repeated file edges, G2Vec.py:390). Dataset-static: compute once and
    pass to build_group_graph for both prognosis groups."""
    key = edge_idx[:, 0].long() * n_genes + edge_idx[:, 1].long()
    key = torch.unique(key)
    src = (key // n_genes).int()
    dst = (key % n_genes).int()
    return torch.stack([src, dst], dim=1)


def build_group_graph(expr: torch.Tensor, labels: torch.Tensor, group: int,
                      edge_idx: torch.Tensor, n_genes: int,
                      threshold: float = 0.5, mode: str = "auto",
                      edges_deduped: bool = False,
                      corr: str = "pearson") -> CsrGraph:
    """CSR graph for one prognosis group (the sparse equivalent of
    construct_adjMat, G2Vec.py:370-391). edges_deduped=True skips the
    per-call unique pass (callers hoist dedupe_edges once per dataset).
    corr: "pearson" | "spearman" (see zscore_group)."""
    if corr not in CORR_KINDS:
        raise ValueError(f"corr must be pearson|spearman, got {corr}")
    device = expr.device
    if edge_idx.numel() == 0:
        return CsrGraph(torch.zeros(n_genes + 1, dtype=torch.int32, device=device),
                        torch.zeros(0, dtype=torch.int32, device=device),
                        torch.zeros(0, dtype=torch.float32, device=device), n_genes)
    pairs = (edge_idx.int() if edges_deduped
             else dedupe_edges(edge_idx, n_genes))
    src, dst = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()

    zt = zscore_group(expr, labels, group, corr)
    w = edge_pcc_weights(zt, pairs, mode)
    keep = w > threshold
    src, dst, w = src[keep], dst[keep], w[keep]

    order = torch.argsort(src.long() * n_genes + dst.long())
    src, dst, w = src[order], dst[order], w[order]
    counts = torch.bincount(src.long(), minlength=n_genes)
    row_ptr = torch.zeros(n_genes + 1, dtype=torch.int64, device=device)
    torch.cumsum(counts, 0, out=row_ptr[1:])
    return CsrGraph(row_ptr.int().contiguous(), dst.contiguous(),
                    w.float().contiguous(), n_genes)
