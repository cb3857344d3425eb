"""Device-op dispatch layer.

CUDA/HIP tensors -> the in-tree native extension `g2vec_amd._C`
(hand-written gfx950 HIP kernels; FAILS LOUDLY if the extension is not
built — there is deliberately no silent eager fallback on a GPU box).
CPU tensors -> the torch/numpy oracles in `cpu_ref`.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch

from . import cpu_ref

_NATIVE = None
_NATIVE_ERR: Optional[BaseException] = None
try:  # pragma: no cover - exercised only when the extension is built
    from g2vec_amd import _C as _NATIVE  # type: ignore
except Exception as e:  # noqa: BLE001
    _NATIVE_ERR = e


def native_available() -> bool:
    return _NATIVE is not None


def native():
    if _NATIVE is None:
        raise RuntimeError(
            "g2vec_amd._C HIP extension is not importable on this host — the GPU "
            "compute path refuses to fall back to eager PyTorch. Build it in-tree "
            "with `python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Import error was: {_NATIVE_ERR!r}")
    return _NATIVE


# ------------------------------------------------------------------ walks
def random_walks(row_ptr, col_idx, weights, sources, num_repetition: int,
                 len_path: int, seed: int):
    if row_ptr.is_cuda:
        return native().random_walks(row_ptr, col_idx, weights, sources,
                                     num_repetition, len_path, seed)
    return cpu_ref.random_walks(row_ptr, col_idx, weights, sources,
                                num_repetition, len_path, seed)


# ------------------------------------------------------------------ CBOW fast (scalar) path
def cbow_fwd_scalar(s, genes, offsets, labels, inv_b: float, want_grad: bool):
    if s.is_cuda:
        loss, correct, dO = native().cbow_fwd_scalar(
            s, genes, offsets, labels, float(inv_b), bool(want_grad))
        return loss, correct, (dO if want_grad else None)
    return cpu_ref.cbow_fwd_scalar(s, genes, offsets, labels, inv_b, want_grad)


def cbow_eval_counts_(s, genes, offsets, labels, p_split: int,
                      counts: torch.Tensor, dO: Optional[torch.Tensor] = None,
                      inv_b: float = 1.0, scan=None,
                      partials: Optional[torch.Tensor] = None) -> None:
    """Accumulate the concatenated train+val correct counts into counts[2]
    (caller zeroes it). One fused kernel on GPU; oracle math on CPU.

    partials (GPU, subwave eval only) = a caller-owned f32 [eval_grid(P, G),
    2] table: the eval writes its per-block partials there, launches no
    fold and leaves counts alone; fold_partials_rows_ folds a stack of such
    tables later (the K-epoch block graph: one fold per block).

    dO given: also emit the train split's (p < p_split) dlogit into dO with
    scale inv_b — the fused next-epoch forward (this eval's s is the next
    epoch's pre-update s), numerically identical to a separate
    cbow_fwd_scalar over the train paths (fp32 summation order differs
    between the kernel variants).

    scan = (pathid i32[nnz], piece f32[>=P*cap], cap): persistent buffers
    enabling the instance-parallel segmented-scan variant — the hot
    steady-state eval (see eval_scan_kernel)."""
    if partials is not None and (not s.is_cuda or scan is not None):
        raise ValueError("partials goes with the GPU subwave eval only")
    if s.is_cuda:
        if scan is not None:
            pathid, piece, cap = scan
            native().cbow_eval_scan_(s, genes, pathid, offsets, labels,
                                     int(p_split), int(cap), piece, counts,
                                     dO=dO, inv_b=float(inv_b))
            return
        native().cbow_eval_counts_(s, genes, offsets, labels, int(p_split),
                                   counts, dO=dO, inv_b=float(inv_b),
                                   partials=partials)
        return
    _l, corr, d = cpu_ref.cbow_fwd_scalar(s, genes, offsets, labels, inv_b,
                                          dO is not None)
    counts[0] += corr[:p_split].sum()
    counts[1] += corr[p_split:].sum()
    if dO is not None:
        dO.copy_(d[:p_split])


def eval_grid(P: int, G: int) -> int:
    """Rows of the per-block partial table the GPU eval of P paths over a
    G-gene s table writes (G2VEC_EVAL_GRID / G2VEC_EVAL_LDS* applied, as
    read at this call)."""
    return int(native().eval_grid(int(P), int(G)))


def fold_partials_rows_(partials: torch.Tensor, counts: torch.Tensor) -> None:
    """counts [K, 2] (OVERWRITTEN) = the fold of K evals' partial tables
    [K, grid, 2], each exactly as the eval's own fold would give it. GPU."""
    native().fold_partials_rows_(partials, counts)


class ScatterPlan(NamedTuple):
    """Precomputed gene-sorted instance layout for the deterministic
    c = X^T dO reduction (built once per path set; genes never change
    across epochs).

    When the dO table outgrows one XCD's 4 MB L2 (large path counts), the
    instances are sorted by (path-slab, gene) instead — slab_seg_ptr marks
    each ~3 MB slab's segment range and scatter_dO launches the reduce one
    slab at a time, so every XCD gathers from an L2-resident dO slice.
    Accumulation order (ascending slab) is fixed: still deterministic."""
    inst_path: torch.Tensor   # i32 [nnz]  path id of each instance, gene-sorted
    seg_start: torch.Tensor   # i32 [n_seg+1]
    seg_gene: torch.Tensor    # i32 [n_seg]
    slab_seg_ptr: Optional[list] = None   # [n_slabs+1] segment-range bounds


SLAB_BYTES = 3 << 20     # dO slice per launch; < the 4 MB per-XCD L2


def build_scatter_plan(genes: torch.Tensor, offsets: torch.Tensor,
                       n_genes: int, _force_slabs: bool = False,
                       slabs: bool = True) -> ScatterPlan:
    # _force_slabs: CPU tests exercise the slab geometry (the CPU compute
    # path itself never consumes a slabbed plan)
    # slabs=False: always one gene-sorted pass — what cbow_bwd_rows needs
    # (it WRITES one dW row per segment, so a gene may own only one)
    counts = (offsets[1:] - offsets[:-1]).long()
    P = len(counts)
    path_of = torch.repeat_interleave(
        torch.arange(P, device=genes.device), counts)
    slab_paths = SLAB_BYTES // 4
    n_slabs = ((P + slab_paths - 1) // slab_paths
               if slabs and (genes.is_cuda or _force_slabs) else 1)
    if n_slabs <= 1:
        sorted_key, perm = torch.sort(genes.long(), stable=True)
    else:
        key = (path_of // slab_paths) * n_genes + genes.long()
        sorted_key, perm = torch.sort(key, stable=True)
    inst_path = path_of[perm].int().contiguous()
    seg_key, seg_counts = torch.unique_consecutive(sorted_key,
                                                   return_counts=True)
    seg_start = torch.zeros(len(seg_key) + 1, dtype=torch.int64,
                            device=genes.device)
    torch.cumsum(seg_counts, 0, out=seg_start[1:])
    if n_slabs <= 1:
        return ScatterPlan(inst_path, seg_start.int().contiguous(),
                           seg_key.int().contiguous())
    seg_slab = seg_key // n_genes
    seg_gene = (seg_key - seg_slab * n_genes).int().contiguous()
    ptr = torch.searchsorted(
        seg_slab, torch.arange(n_slabs + 1, device=genes.device)).cpu()
    return ScatterPlan(inst_path, seg_start.int().contiguous(), seg_gene,
                       [int(x) for x in ptr])


def _plan_slabs(plan: ScatterPlan):
    """(seg_start, seg_gene) per slab, ascending (one L2-resident dO slice at
    a time); an unslabbed plan is one slab, empty slabs are skipped."""
    ptr = plan.slab_seg_ptr
    if ptr is None:                 # whole tensors: no per-call slice views
        if plan.seg_gene.numel():
            yield plan.seg_start, plan.seg_gene
        return
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b > a:
            yield plan.seg_start[a:b + 1], plan.seg_gene[a:b]


def scatter_dO(genes, offsets, dO, n_genes: int,
               plan: Optional[ScatterPlan] = None,
               out: Optional[torch.Tensor] = None):
    """c = X^T dO. out (GPU only) = a caller-owned f32 [n_genes] buffer that
    is ALREADY all zero: the reduction accumulates into it and returns it,
    with no allocation and no fill launch."""
    if dO.is_cuda:
        if plan is None:
            plan = build_scatter_plan(genes, offsets, n_genes)
        if out is None:
            c = torch.zeros(n_genes, dtype=torch.float32, device=dO.device)
        else:
            if out.numel() != n_genes:
                raise ValueError("out must have n_genes elements")
            c = out
        for seg_start, seg_gene in _plan_slabs(plan):
            native().scatter_dO_det_(plan.inst_path, seg_start, seg_gene,
                                     dO, c)
        return c
    if out is not None:
        raise ValueError("out goes with the GPU path only")
    return cpu_ref.scatter_dO(genes, offsets, dO, n_genes)


def trunc_normal_(out: torch.Tensor, std: float, seed: int) -> None:
    """Seeded +-2sigma truncated-normal fill (K9, reference init
    semantics tf.truncated_normal G2Vec.py:234-235). Device kernel on
    GPU — no host-side multi-GB rejection loop at the 1M x 512 config."""
    if out.is_cuda:
        native().trunc_normal_(out, float(std), int(seed))
        return
    cpu_ref.trunc_normal_(out, std, seed)


def tf1_lr_t(lr: float, b1: float, b2: float, t: int) -> float:
    """TF1 AdamOptimizer effective step size (G2Vec.py:245-246 semantics)."""
    return lr * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)


def _lrt_buf(lrt_buf, W, t: int, lr: float, b1: float, b2: float):
    """The caller's lr_t device slot, or a fresh one holding this step's."""
    if lrt_buf is not None:
        return lrt_buf
    return torch.tensor([tf1_lr_t(lr, b1, b2, t)], dtype=torch.float32,
                        device=W.device)


def adam_rank1(W, m, v, c, who, t: int, lr: float, b1: float, b2: float,
               eps: float, lrt_buf: Optional[torch.Tensor] = None) -> None:
    """lrt_buf: optional persistent f32[1] device buffer holding lr_t —
    required under hipGraph capture (the per-step value must be read from
    device memory, not baked into the recorded launch)."""
    if W.is_cuda:
        lrt_buf = _lrt_buf(lrt_buf, W, t, lr, b1, b2)
        native().adam_rank1(W, m, v, c, who, lrt_buf, float(b1), float(b2),
                            float(eps))
        return
    cpu_ref.adam_rank1(W, m, v, c, who, t, lr, b1, b2, eps)


def adam_rank1_fused(W, m, v, c, who, mO, vO, t: int, lr: float,
                     b1: float, b2: float, eps: float,
                     lrt_buf: Optional[torch.Tensor] = None) -> None:
    """Fused epoch tail: rank-1 Adam on W_ih AND the dW_ho = W_pre^T c
    reduction AND the W_ho Adam update — one streaming pass over the
    pre-update W rows plus a single fold launch (replaces gemv_cols +
    adam_rank1 + adam_dense: three launches and an extra full W read).
    Deterministic (fixed per-thread/block fold order)."""
    if W.is_cuda:
        lrt_buf = _lrt_buf(lrt_buf, W, t, lr, b1, b2)
        native().adam_rank1(W, m, v, c, who, lrt_buf, float(b1), float(b2),
                            float(eps), mO=mO, vO=vO)
        return
    grad_who = torch.mv(W.t(), c)          # pre-update W
    cpu_ref.adam_rank1(W, m, v, c, who, t, lr, b1, b2, eps)
    cpu_ref.adam_dense(who, mO, vO, grad_who, t, lr, b1, b2, eps)


def adam_dense(W, m, v, grad, t: int, lr: float, b1: float, b2: float,
               eps: float, lrt_buf: Optional[torch.Tensor] = None) -> None:
    if W.is_cuda:
        lrt_buf = _lrt_buf(lrt_buf, W, t, lr, b1, b2)
        native().adam_dense(W, m, v, grad, lrt_buf, float(b1), float(b2),
                            float(eps))
        return
    cpu_ref.adam_dense(W, m, v, grad, t, lr, b1, b2, eps)


# ------------------------------------------------------------------ CBOW general (kernel-chain) path
def cbow_fwd(W, who, genes, offsets, labels, inv_b: float, want_grad: bool,
             act: int = 0):
    """act: 0 linear (reference semantics); 1 ReLU on the hidden vector
    (opt-in non-linear successor; returned H is the pre-activation)."""
    if W.is_cuda:
        loss, correct, dO, H = native().cbow_fwd(
            W, who, genes, offsets, labels, float(inv_b), bool(want_grad),
            act=int(act))
        if not want_grad:
            return loss, correct, None, None
        return loss, correct, dO, H
    return cpu_ref.cbow_fwd(W, who, genes, offsets, labels, inv_b, want_grad,
                            act=act)


def cbow_bwd_rows(who, genes, offsets, dO, n_genes: int,
                  plan: Optional[ScatterPlan] = None,
                  H_pre: Optional[torch.Tensor] = None):
    """General-path dW_ih backward. On GPU this is the deterministic
    per-gene-segment kernel (no atomics) driven by the same ScatterPlan as
    the fast path's c-reduction. H_pre given = ReLU backward mask source
    (the forward's pre-activation H)."""
    if dO.is_cuda:
        if plan is None:
            plan = build_scatter_plan(genes, offsets, n_genes, slabs=False)
        if plan.slab_seg_ptr is not None:
            # a slab-blocked plan has one segment per (slab, gene): the
            # kernel would overwrite a gene's row once per slab
            raise RuntimeError(
                "cbow_bwd_rows needs a single-pass plan "
                "(build_scatter_plan(..., slabs=False)), got a slab-blocked one")
        return native().cbow_bwd_rows(who, plan.inst_path, plan.seg_start,
                                      plan.seg_gene, dO, int(n_genes),
                                      Hpre=H_pre)
    return cpu_ref.cbow_bwd_rows(who, genes, offsets, dO, n_genes,
                                 H_pre=H_pre)


def gemv_rows(W, x, out, clear: Optional[torch.Tensor] = None) -> None:
    """out = W @ x (tall-skinny GEMV). Own wave-per-row kernel on GPU:
    rocBLAS gemvn ran at ~2% of HBM bandwidth on the [1M, 512] shape.
    clear = an f32 [G] tensor zeroed (+0.0) by the same launch."""
    if W.is_cuda:
        native().gemv_rows_(W, x, out, clear=clear)
        return
    torch.mv(W, x, out=out)
    if clear is not None:
        clear.zero_()


def gemv_cols(W, c, out) -> None:
    """out = W^T @ c (column reduction over G rows); atomic-free
    partials + fold on GPU."""
    if W.is_cuda:
        native().gemv_cols_(W, c, out)
        return
    torch.mv(W.t(), c, out=out)


# ------------------------------------------------------------------ replica-batched fast path
# R independently initialised models over ONE path set (models/replicas.py).
# Layouts, all f32 and contiguous: s_R / c_R [G, R] and dO_R [P_tr, R]
# replica-minor, counts_R [R, 2], W/m/v [R, G, h] and who/mO/vO [R, h]
# replica-major (W[r] is an ordinary [G, h] view). Contract: for every
# replica r each output is bitwise what the single op above gives on the same
# device when fed replica r's slice. The CPU mirrors loop the single ops.
REP_MAX = 32


def _rep_R(t: torch.Tensor, name: str) -> int:
    if t.dim() != 2 or t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 [rows, R] tensor")
    R = int(t.shape[1])
    if not 1 <= R <= REP_MAX:
        raise ValueError(f"{name}: R must be in [1, {REP_MAX}], got {R}")
    return R


def cbow_eval_counts_rep_(s_R, genes, offsets, labels, p_split: int,
                          counts_R: torch.Tensor,
                          dO_R: Optional[torch.Tensor] = None,
                          inv_b: float = 1.0) -> None:
    """Batched cbow_eval_counts_: counts_R[r] = the two correct counts of
    replica r (OVERWRITTEN, no zeroing needed) and, with dO_R, column r of
    dO_R[:p_split] = its train-split dlogits. Rows of dO_R at or beyond
    p_split are not written."""
    R = _rep_R(s_R, "s_R")
    if s_R.is_cuda:
        native().cbow_eval_counts_rep_(s_R, genes, offsets, labels,
                                       int(p_split), counts_R, dO_R=dO_R,
                                       inv_b=float(inv_b))
        return
    for r in range(R):
        cnt = torch.zeros(2, dtype=torch.float32)
        d = (torch.empty(p_split, dtype=torch.float32)
             if dO_R is not None else None)
        cbow_eval_counts_(s_R[:, r].contiguous(), genes, offsets, labels,
                          p_split, cnt, dO=d, inv_b=inv_b)
        counts_R[r] = cnt
        if dO_R is not None:
            dO_R[:p_split, r] = d


def scatter_dO_rep(plan: ScatterPlan, dO_R, n_genes: int) -> torch.Tensor:
    """Batched scatter_dO over the single trainer's ScatterPlan: c_R [G, R]
    with c_R[:, r] = X^T dO_R[:, r], slab by slab like scatter_dO (the slab
    size is the single op's, not re-tuned for the R-times-larger table)."""
    R = _rep_R(dO_R, "dO_R")
    c_R = torch.zeros(n_genes, R, dtype=torch.float32, device=dO_R.device)
    if dO_R.is_cuda:
        for seg_start, seg_gene in _plan_slabs(plan):
            native().scatter_dO_rep_(plan.inst_path, seg_start, seg_gene,
                                     dO_R, c_R)
        return c_R
    # the plan lists each gene's instances in ascending path order, slab by
    # slab: the order cpu_ref.scatter_dO adds them in
    seg_len = (plan.seg_start[1:] - plan.seg_start[:-1]).long()
    gene_of = torch.repeat_interleave(plan.seg_gene.long(), seg_len)
    for r in range(R):
        col = torch.zeros(n_genes, dtype=torch.float32)
        col.index_add_(0, gene_of, dO_R[:, r][plan.inst_path.long()])
        c_R[:, r] = col
    return c_R


def adam_rank1_rep(W, m, v, c_R, who, mO, vO, t: int, lr: float, b1: float,
                   b2: float, eps: float,
                   lrt_buf: Optional[torch.Tensor] = None) -> None:
    """Batched adam_rank1_fused. One lr_t for all replicas (they share the
    Adam step t); lrt_buf as in adam_rank1."""
    R = _rep_R(c_R, "c_R")
    if W.dim() != 3 or W.shape[0] != R:
        raise ValueError("W must be [R, G, h] with R = c_R.shape[1]")
    if W.is_cuda:
        lrt_buf = _lrt_buf(lrt_buf, W, t, lr, b1, b2)
        native().adam_rank1_rep(W, m, v, c_R, who, mO, vO, lrt_buf,
                                float(b1), float(b2), float(eps))
        return
    for r in range(R):
        adam_rank1_fused(W[r], m[r], v[r], c_R[:, r].contiguous(), who[r],
                         mO[r], vO[r], t, lr, b1, b2, eps)


def gemv_rows_rep_(W, who, s_R) -> None:
    """s_R[:, r] = W[r] @ who[r]."""
    R = _rep_R(s_R, "s_R")
    if W.dim() != 3 or W.shape[0] != R:
        raise ValueError("W must be [R, G, h] with R = s_R.shape[1]")
    if W.is_cuda:
        native().gemv_rows_rep_(W, who, s_R)
        return
    for r in range(R):
        s_R[:, r] = torch.mv(W[r], who[r])


# ------------------------------------------------------------------ graph / PCC
def pcc_edges(zt, edge_idx, n_group: int):
    if zt.is_cuda:
        return native().pcc_edges(zt, edge_idx, int(n_group))
    return cpu_ref.pcc_edges(zt, edge_idx, n_group)


def corr_gemm(zt, n_group: int):
    if zt.is_cuda:
        return native().corr_gemm(zt, int(n_group))
    return cpu_ref.corr_gemm(zt, n_group)


# ------------------------------------------------------------------ steps 5-6: k-means / scoring
def kmeans_step(X, C, prev, labels, C_new, sums, counts, n_changed,
                inertia) -> None:
    """One fused Lloyd iteration over X f32[G, h] with centroids C f32[k, h]
    (k <= 8), everything through out-arguments: labels i32[G] (argmin of the
    direct squared distances, lowest index on ties), sums f32[k, h],
    counts i32[k], n_changed i32[1] (rows whose label differs from prev),
    inertia f64[1] and C_new = sums / float(counts) (an empty cluster keeps
    its row). prev may be labels and C_new may be C. On GPU h must be one
    of 64/128/256/512/1024."""
    if X.is_cuda:
        native().kmeans_step(X, C, prev, labels, C_new, sums, counts,
                             n_changed, inertia)
        return
    cpu_ref.kmeans_step(X, C, prev, labels, C_new, sums, counts, n_changed,
                        inertia)


def kmeans_mind2_(X, c, d2) -> None:
    """d2[g] = min(d2[g], |x_g - c|^2) for one new centre c f32[h]."""
    if X.is_cuda:
        native().kmeans_mind2_(X, c, d2)
        return
    cpu_ref.kmeans_mind2_(X, c, d2)


def row_norms(W) -> torch.Tensor:
    """d-score: f32[G] row L2 norms of W f32[G, h], f64-accumulated."""
    if W.is_cuda:
        out = torch.empty(W.shape[0], dtype=torch.float32, device=W.device)
        native().row_norms_(W, out)
        return out
    return cpu_ref.row_norms(W)


def t_scores(expr, labels) -> torch.Tensor:
    """t-score: f32[G] |pooled t| per gene column of expr f32[S, G]
    (samples x genes), labels i32/i64[S] with 0 good / 1 poor."""
    if expr.is_cuda:
        out = torch.empty(expr.shape[1], dtype=torch.float32,
                          device=expr.device)
        native().t_scores_(expr, labels, out)
        return out
    return cpu_ref.t_scores(expr, labels)


# ------------------------------------------------------------------ rank statistics
# Tile constants of rank_body (g2vec_kernels.hip), for the tests' edge
# shapes: genes per block tile, samples per staged j-tile, x_i per wave,
# waves per block, and the grid cap beyond which gene tiles are strided.
RANK_TG = 64
RANK_SJ = 128
RANK_IB = 8
RANK_WAVES = 4
RANK_MAX_BLOCKS = 16384
RANK_S_MAX = 1 << 23            # half-integer ranks <= S are exact in f32 below
RANKSUM_S_MAX = (1 << 21) + 1   # 4*SSR <= S^3 / 3 must fit int64


def _rank_check(expr, name: str = "X") -> None:
    if expr.dtype != torch.float32 or expr.dim() != 2:
        raise ValueError(f"{name} must be a float32 [S, G] tensor")
    if not expr.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if not 1 <= expr.shape[0] < RANK_S_MAX:
        raise ValueError(f"{name} needs 1 <= S < 2^23 rows, got "
                         f"{expr.shape[0]}")
    # NaN has no rank
    if bool(torch.isnan(expr).any()):
        raise ValueError(f"{name} must not hold NaN")


def rank_columns(X) -> torch.Tensor:
    """ranks f32 [S, G]: the average rank (1-based, ties share the mean of
    their positions) of every element of X f32 [S, G] within its column:
    less + 0.5 * (equal + 1) with less = #{j : x[j,g] < x[i,g]} and equal =
    #{j : x[j,g] == x[i,g]}, self included. IEEE compares: -0.0 ties +0.0,
    +-inf are ordinary values; NaN is refused. Half-integers, exact in f32;
    a function of the inputs only."""
    _rank_check(X)
    if X.is_cuda:
        out = torch.empty_like(X)
        native().rank_columns_(X, out)
        return out
    return cpu_ref.rank_columns(X)


def ranksum_scores(expr, labels):
    """(z, auc) f32 [G]: the Wilcoxon rank-sum test of label 1 (poor)
    against label 0 (good) per gene column of expr f32 [S, G], labels
    i32/i64 [S]; rows with any other label are dropped first, as t_scores
    ignores them. z = |W1 - n1 (S+1)/2| / sqrt(n1 n0 / (S (S-1)) * SSR) with
    W1 the poor group's rank sum and SSR the squared deviations of the
    average ranks from (S+1)/2 (tie-corrected, no continuity correction);
    auc = (W1 - n1 (n1+1)/2) / (n1 n0). z = 0 and auc = 0.5 for a constant
    gene or a group of fewer than 2 samples. Integer sums, f64 epilogue:
    bitwise reproducible."""
    if labels.dim() != 1 or labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("labels must be an int32/int64 [S] tensor")
    if labels.device != expr.device:
        raise ValueError("expr and labels must be on the same device")
    if expr.dim() != 2 or labels.shape[0] != expr.shape[0]:
        raise ValueError("labels must have one element per row of expr")
    keep = (labels == 0) | (labels == 1)
    if not bool(keep.all()):
        expr, labels = expr[keep].contiguous(), labels[keep]
    G = expr.shape[1]
    if expr.shape[0] == 0:
        return (torch.zeros(G, dtype=torch.float32, device=expr.device),
                torch.full((G,), 0.5, dtype=torch.float32,
                           device=expr.device))
    _rank_check(expr, "expr")
    if expr.shape[0] >= RANKSUM_S_MAX:
        raise ValueError("ranksum_scores needs S <= 2^21 samples")
    if expr.is_cuda:
        z = torch.empty(G, dtype=torch.float32, device=expr.device)
        auc = torch.empty(G, dtype=torch.float32, device=expr.device)
        native().ranksum_scores_(expr, labels.int().contiguous(), z, auc)
        return z, auc
    return cpu_ref.ranksum_scores(expr, labels)


# ------------------------------------------------------------------ step 6: permutation null of t
def _perm_check(expr, masks) -> int:
    """The guards both perm_t entry points share, before any launch; returns
    n1, the number of poor-group samples every mask row carries."""
    if expr.dtype != torch.float32 or expr.dim() != 2:
        raise ValueError("expr must be a float32 [S, G] tensor")
    if masks.dtype != torch.uint8 or masks.dim() != 2:
        raise ValueError("masks must be a uint8 [B, S] tensor")
    if not expr.is_contiguous() or not masks.is_contiguous():
        raise ValueError("expr and masks must be contiguous")
    if masks.device != expr.device:
        raise ValueError("expr and masks must be on the same device")
    S = expr.shape[0]
    if masks.shape[1] != S:
        raise ValueError(f"masks has {masks.shape[1]} columns, expr has "
                         f"{S} samples")
    if S < 4:
        raise ValueError("the pooled t needs S >= 4 samples")
    if masks.shape[0] == 0:
        raise ValueError("masks has no rows")
    if int(masks.max()) > 1:
        raise ValueError("masks must hold only 0 and 1")
    rows = masks.sum(dim=1, dtype=torch.int64)
    n1, n1_hi = int(rows.min()), int(rows.max())
    if n1 != n1_hi:
        raise ValueError(f"every mask row must mark the same number of "
                         f"samples, got {n1} to {n1_hi}")
    if n1 < 2 or S - n1 < 2:
        raise ValueError(f"each group needs >= 2 samples, masks give "
                         f"{S - n1} / {n1}")
    return n1


def col_moments(expr):
    """(T, Q) f64 [G]: f64-accumulated column sums of x and of the f32
    product x*x of expr f32 [S, G]."""
    if expr.is_cuda:
        G = expr.shape[1]
        T = torch.empty(G, dtype=torch.float64, device=expr.device)
        Q = torch.empty(G, dtype=torch.float64, device=expr.device)
        native().col_moments_(expr, T, Q)
        return T, Q
    return cpu_ref.col_moments(expr)


def perm_t_stats(expr, masks) -> torch.Tensor:
    """stat f64 [B, G] = t^2 of the pooled two-sample t of every gene column
    of expr f32 [S, G] (centred per gene by the caller) under every 0/1 row
    of masks u8 [B, S] (1 = poor group). 0 where the pooled variance is
    <= 0. All rows must mark the same n1 >= 2 samples and leave >= 2. Meant
    for small B: the observed labelling and tests."""
    n1 = _perm_check(expr, masks)
    if expr.is_cuda:
        T, Q = col_moments(expr)
        out = torch.empty(masks.shape[0], expr.shape[1], dtype=torch.float64,
                          device=expr.device)
        native().perm_t_stats_(expr, masks, T, Q, n1, out)
        return out
    return cpu_ref.perm_t_stats(expr, masks, n1)


def perm_t_counts(expr, masks, stat_obs, moments=None):
    """(counts i32 [G], maxstat f64 [B]): counts[g] = number of mask rows
    whose stat[b, g] >= stat_obs[g] * (1 - 2^-30), maxstat[b] = max_g
    stat[b, g]; the same arithmetic as perm_t_stats, nothing of size G x B
    written. moments: optional (T, Q) from col_moments(expr), to share them
    between calls over mask chunks (GPU)."""
    n1 = _perm_check(expr, masks)
    G = expr.shape[1]
    if (stat_obs.dtype != torch.float64 or stat_obs.shape != (G,)
            or not stat_obs.is_contiguous()
            or stat_obs.device != expr.device):
        raise ValueError("stat_obs must be a contiguous float64 [G] tensor "
                         "on expr's device")
    if expr.is_cuda:
        T, Q = moments if moments is not None else col_moments(expr)
        counts = torch.empty(G, dtype=torch.int32, device=expr.device)
        maxstat = torch.empty(masks.shape[0], dtype=torch.float64,
                              device=expr.device)
        native().perm_t_counts_(expr, masks, T, Q, n1, stat_obs, counts,
                                maxstat)
        return counts, maxstat
    return cpu_ref.perm_t_counts(expr, masks, n1, stat_obs)


# ------------------------------------------------------------------ nearest genes
def knn_topk(Xq, X, k: int, q_index=None, grid_y: int = 0):
    """(idx i32 [Q, k], val f32 [Q, k]): for every row of Xq f32 [Q, h] the k
    largest dot(Xq[q], X[g]) over the rows g != q_index[q] of X f32 [G, h]
    (q_index i32 [Q]; -1 or None excludes nothing). Total order: value
    descending, equal values (-0.0 == +0.0) by ascending g; with fewer than
    k candidates the tail is idx -1, val -inf. 1 <= k <= 64, inputs finite.
    A function of the inputs only: bitwise equal run to run and for every
    grid_y (GPU launch split over the candidates; 0 = automatic). Widths
    that are no multiple of 4 are zero-padded (exact) on the GPU."""
    for name, t in (("Xq", Xq), ("X", X)):
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{name} must be a float32 [rows, h] tensor")
    if Xq.shape[1] != X.shape[1]:
        raise ValueError(f"Xq has {Xq.shape[1]} columns, X has {X.shape[1]}")
    if X.device != Xq.device:
        raise ValueError("Xq and X must be on the same device")
    if not 1 <= int(k) <= 64:
        raise ValueError(f"k must be in [1, 64], got {k}")
    if X.shape[0] >= 2 ** 31:
        raise ValueError("X must have fewer than 2^31 rows")
    if grid_y < 0:
        raise ValueError("grid_y must be >= 0")
    # NaN has no place in a total order
    if not (bool(torch.isfinite(Xq).all()) and bool(torch.isfinite(X).all())):
        raise ValueError("Xq and X must be finite")
    Q, G = Xq.shape[0], X.shape[0]
    if q_index is not None:
        if q_index.dim() != 1 or q_index.shape[0] != Q or \
                q_index.dtype not in (torch.int32, torch.int64):
            raise ValueError("q_index must be an int32/int64 [Q] tensor")
        if q_index.device != Xq.device:
            raise ValueError("q_index must be on Xq's device")
        q_index = q_index.int().contiguous()
    if not Xq.is_cuda:
        return cpu_ref.knn_topk(Xq, X, int(k), q_index)
    nat = native()
    pad = -X.shape[1] % 4
    if pad or X.shape[1] == 0:
        pad = pad or 4
        Xq = torch.nn.functional.pad(Xq, (0, pad))
        X = torch.nn.functional.pad(X, (0, pad))
    Xq, X = Xq.contiguous(), X.contiguous()
    idx = torch.empty(Q, k, dtype=torch.int32, device=Xq.device)
    val = torch.empty(Q, k, dtype=torch.float32, device=Xq.device)
    gy = nat.knn_grid_y(Q, G, int(grid_y))
    part_idx = part_val = None
    if gy > 1:
        part_idx = torch.empty(Q, gy, k, dtype=torch.int32, device=Xq.device)
        part_val = torch.empty(Q, gy, k, dtype=torch.float32,
                               device=Xq.device)
    nat.knn_topk_(Xq, X, q_index, int(k), int(grid_y), part_idx, part_val,
                  idx, val)
    return idx, val


# ------------------------------------------------------------------ L-group silhouettes
CDS_K_MAX = 8           # clusters per call, the limit of kmeans_step


def cluster_dist_sums(Xq, X, labels, k: int, q_index=None, grid_y: int = 0):
    """D f64 [Q, k]: D[q, c] = the sum over the rows g of X f32 [G, h] with
    labels[g] == c and g != q_index[q] of the Euclidean distance
    d(q, g) = sqrtf(max(nq[q] + nx[g] - 2 dot(Xq[q], X[g]), 0)) to row q of
    Xq f32 [Q, h]; nq / nx are the squared row norms (f64-accumulated,
    rounded once), d is f32, the sums are f64. labels i32/i64 [G] in [0, k),
    1 <= k <= 8; q_index i32/i64 [Q] (-1 or None excludes nothing); inputs
    finite. An empty cluster's column is +0.0. Bitwise equal run to run for
    a given grid_y (GPU launch split over the candidates; 0 = automatic);
    across splits only the f64 addition order changes. Widths that are no
    multiple of 4 are zero-padded (exact) on the GPU."""
    for name, t in (("Xq", Xq), ("X", X)):
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"{name} must be a float32 [rows, h] tensor")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if Xq.shape[1] != X.shape[1]:
        raise ValueError(f"Xq has {Xq.shape[1]} columns, X has {X.shape[1]}")
    if X.device != Xq.device:
        raise ValueError("Xq and X must be on the same device")
    if not 1 <= int(k) <= CDS_K_MAX:
        raise ValueError(f"k must be in [1, {CDS_K_MAX}], got {k}")
    k = int(k)
    Q, G = Xq.shape[0], X.shape[0]
    if G >= 2 ** 31:
        raise ValueError("X must have fewer than 2^31 rows")
    if grid_y < 0:
        raise ValueError("grid_y must be >= 0")
    if labels.dim() != 1 or labels.shape[0] != G or \
            labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("labels must be an int32/int64 [G] tensor")
    if labels.device != X.device:
        raise ValueError("labels must be on X's device")
    bad = ((labels < 0) | (labels >= k)).nonzero()
    if bad.numel():
        g = int(bad[0])
        raise ValueError(f"labels must lie in [0, {k}): labels[{g}] = "
                         f"{int(labels[g])}")
    if not (bool(torch.isfinite(Xq).all()) and bool(torch.isfinite(X).all())):
        raise ValueError("Xq and X must be finite")
    if q_index is not None:
        if q_index.dim() != 1 or q_index.shape[0] != Q or \
                q_index.dtype not in (torch.int32, torch.int64):
            raise ValueError("q_index must be an int32/int64 [Q] tensor")
        if q_index.device != Xq.device:
            raise ValueError("q_index must be on Xq's device")
        q_index = q_index.int().contiguous()
    labels = labels.int().contiguous()
    if not Xq.is_cuda:
        return cpu_ref.cluster_dist_sums(Xq, X, labels, k, q_index)
    nat = native()
    pad = -X.shape[1] % 4
    if pad or X.shape[1] == 0:
        pad = pad or 4
        Xq = torch.nn.functional.pad(Xq, (0, pad))
        X = torch.nn.functional.pad(X, (0, pad))
    dev = Xq.device
    D = torch.empty(Q, k, dtype=torch.float64, device=dev)
    nq = torch.empty(Q, dtype=torch.float32, device=dev)
    nx = torch.empty(G, dtype=torch.float32, device=dev)
    gy = nat.cds_grid_y(Q, G, k, int(grid_y))
    part = None
    if gy > 1:
        part = torch.empty(Q, gy, k, dtype=torch.float64, device=dev)
    nat.cluster_dist_sums_(Xq, X, labels, q_index, k, int(grid_y), nq, nx,
                           part, D)
    return D
