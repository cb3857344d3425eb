"""CPU reference implementations of every device op.

These are the numerics oracles for the HIP kernels (fp32, torch/numpy) and
the fallback execution path on hosts without a GPU. Semantics mirror the
reference pipeline:
  random walk      G2Vec.py:328-346 (non-revisiting weighted walk)
  CBOW fwd/loss    G2Vec.py:238-251 (linear net + sigmoid-CE, sum-reduce
                   because X is 0/1 multi-hot)
  Adam             G2Vec.py:245-246 (TF1 AdamOptimizer update rule)
  PCC              G2Vec.py:354-368
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

# ---------------------------------------------------------------- RNG helpers
_SM64_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_SM64_M1 = np.uint64(0xBF58476D1CE4E5B9)
_SM64_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(state: np.uint64) -> Tuple[np.uint64, np.uint64]:
    """One splitmix64 draw; returns (new_state, random_u64).
    Must stay bit-identical to the device implementation in g2vec_kernels.hip."""
    with np.errstate(over="ignore"):
        state = np.uint64(state + _SM64_GAMMA)
        z = state
        z = np.uint64((z ^ (z >> np.uint64(30))) * _SM64_M1)
        z = np.uint64((z ^ (z >> np.uint64(27))) * _SM64_M2)
        z = np.uint64(z ^ (z >> np.uint64(31)))
    return state, z


def _u01(r: np.uint64) -> float:
    return float(r >> np.uint64(11)) * (1.0 / 9007199254740992.0)


def gene_hash(g: int) -> np.uint64:
    """Order-independent per-gene mix used for path-set hashing (summed over
    the path's genes; commutative so no sort is needed)."""
    _, z = splitmix64(np.uint64(g) * _SM64_M1 + _SM64_GAMMA)
    return z


def path_hash(genes) -> np.int64:
    h = np.uint64(0)
    with np.errstate(over="ignore"):
        for g in genes:
            h = np.uint64(h + gene_hash(int(g)))
    return np.int64(h.astype(np.int64))


# ------------------------------------------------------------------ walks
def random_walks(row_ptr: torch.Tensor, col_idx: torch.Tensor, weights: torch.Tensor,
                 sources: torch.Tensor, num_repetition: int, len_path: int,
                 seed: int, *, walk_ids=None
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Non-revisiting weighted random walks on a CSR graph.

    One walk per (repetition, source), walk_id = rep * n_src + src_pos.
    Returns (nodes i32 [n_walks, len_path] padded -1, lengths i32, hashes i64).
    Matches the reference walk semantics (G2Vec.py:328-346): the current node
    is appended, all visited nodes (incl. current) are masked to weight 0,
    step chosen proportionally to remaining weights, dead-end breaks.

    walk_ids given: only those walk ids (each in [0, n_walks)) are generated
    and returned, row k being walk walk_ids[k] of the full run.
    """
    rp = row_ptr.cpu().numpy()
    ci = col_idx.cpu().numpy()
    w = weights.cpu().numpy().astype(np.float32)
    src = sources.cpu().numpy()
    n_src = len(src)
    n_walks = n_src * num_repetition
    if walk_ids is None:
        walk_ids = range(n_walks)
    else:
        walk_ids = [int(w) for w in walk_ids]
        if any(w < 0 or w >= n_walks for w in walk_ids):
            raise ValueError(f"walk_ids must be in [0, {n_walks})")
    n_out = len(walk_ids)
    nodes = np.full((n_out, len_path), -1, dtype=np.int32)
    lengths = np.zeros(n_out, dtype=np.int32)
    hashes = np.zeros(n_out, dtype=np.int64)

    for row, wid in enumerate(walk_ids):
        rep = wid // n_src
        source = int(src[wid % n_src])
        # RNG keyed on the GLOBAL (source, repetition) so DP-sharded
        # generation is bitwise-identical to single-process
        gid = np.uint64(source) * np.uint64(num_repetition) + np.uint64(rep)
        with np.errstate(over="ignore"):
            state = np.uint64(np.uint64(seed) ^ np.uint64(gid * _SM64_M2 + np.uint64(1)))
        # warm the stream like the device kernel does
        state, _ = splitmix64(state)
        cur = source
        visited = []
        vset = set()
        for _step in range(len_path):
            visited.append(cur)
            vset.add(cur)
            s, e = int(rp[cur]), int(rp[cur + 1])
            if e <= s:
                break
            nb = ci[s:e]
            wt = w[s:e].copy()
            for k in range(len(nb)):
                if int(nb[k]) in vset:
                    wt[k] = 0.0
            tot = float(np.sum(wt, dtype=np.float32))
            state, r = splitmix64(state)
            if tot <= 0.0:
                break
            target = _u01(r) * tot
            c = np.cumsum(wt, dtype=np.float32)
            j = int(np.searchsorted(c, target, side="right"))
            if j >= len(nb) or wt[j] <= 0.0:
                # rounding tail: tot (pairwise np.sum) can exceed the
                # sequential cumsum total in f32, pushing target past
                # c[-1]. Fall back to the LAST POSITIVE-WEIGHT (unvisited)
                # neighbor, exactly like the device kernel's ballot
                # fallback (g2vec_kernels.hip walk_kernel) — never a
                # visited/zero-weight one (the non-revisit invariant that
                # paths.py's "paths are sets" assumption relies on).
                j = int(np.flatnonzero(wt > 0.0)[-1])
            cur = int(nb[j])
        plen = len(visited)
        nodes[row, :plen] = visited
        lengths[row] = plen
        hashes[row] = path_hash(visited)
    return (torch.from_numpy(nodes), torch.from_numpy(lengths), torch.from_numpy(hashes))


# ------------------------------------------------------------------ K9 init
def trunc_normal_(out: torch.Tensor, std: float, seed: int,
                  start: int = 0) -> None:
    """Counter-based +-2sigma truncated normal, mirroring
    trunc_normal_kernel (g2vec_kernels.hip): element i draws Box-Muller
    normals from its own splitmix64 stream and resamples beyond 2sigma.
    Same streams as the device kernel; the float cos/log tails can differ
    by ulps across libm implementations, so parity tests compare with a
    small tolerance (plus bounds/moments), not bitwise.

    start: element k of out draws from stream start + k, i.e. out is the
    slice [start, start + n) of a longer fill with the same seed."""
    import math

    flat = out.view(-1)
    n = flat.numel()
    vals = np.empty(n, dtype=np.float32)
    with np.errstate(over="ignore"):
        for i in range(n):
            state = np.uint64(seed) ^ np.uint64(
                np.uint64(start + i) * _SM64_M2 + np.uint64(1))
            state, _ = splitmix64(state)      # warm draw (kernel parity)
            while True:
                state, r1 = splitmix64(state)
                state, r2 = splitmix64(state)
                u1 = max(_u01(r1), 1e-300)
                x = np.float32(math.sqrt(-2.0 * math.log(u1)) *
                               math.cos(2.0 * math.pi * _u01(r2)))
                if abs(x) <= np.float32(2.0):
                    break
            vals[i] = x
    flat.copy_(torch.from_numpy(vals * np.float32(std)))


# ------------------------------------------------------------------ CBOW (fast scalar path)
def cbow_fwd_scalar(s: torch.Tensor, genes: torch.Tensor, offsets: torch.Tensor,
                    labels: torch.Tensor, inv_b: float, want_grad: bool):
    """Forward of the linear CBOW in collapsed scalar form.

    o_p = sum_{g in path p} s_g  where s = W_ih @ W_ho  (linearity of the
    reference net, G2Vec.py:238-240). Returns (loss[P], correct[P], dO[P]|None).
    """
    counts = (offsets[1:] - offsets[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    o = torch.zeros(len(counts), dtype=torch.float32)
    o.index_add_(0, seg, s[genes.long()])
    y = labels.float()
    loss = torch.clamp(o, min=0) - o * y + torch.log1p(torch.exp(-o.abs()))
    correct = ((o > 0).float() == y).float()
    dO = (torch.sigmoid(o) - y) * inv_b if want_grad else None
    return loss, correct, dO


def scatter_dO(genes: torch.Tensor, offsets: torch.Tensor, dO: torch.Tensor,
               n_genes: int) -> torch.Tensor:
    """c = X^T dO: for each gene, sum of dO over the paths containing it."""
    counts = (offsets[1:] - offsets[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    c = torch.zeros(n_genes, dtype=torch.float32)
    c.index_add_(0, genes.long(), dO[seg])
    return c


def adam_rank1(W: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
               c: torch.Tensor, who: torch.Tensor, t: int,
               lr: float, b1: float, b2: float, eps: float) -> None:
    """Dense TF1-Adam step with the rank-1 gradient grad = c (outer) who.
    Moments stay dense (reference Adam decays untouched rows too)."""
    grad = torch.outer(c, who)
    adam_dense(W, m, v, grad, t, lr, b1, b2, eps)


def adam_dense(W: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
               grad: torch.Tensor, t: int, lr: float, b1: float, b2: float,
               eps: float) -> None:
    """TF1 AdamOptimizer: theta -= lr * sqrt(1-b2^t)/(1-b1^t) * m/(sqrt(v)+eps)."""
    lr_t = lr * (1.0 - b2 ** t) ** 0.5 / (1.0 - b1 ** t)
    m.mul_(b1).add_(grad, alpha=1 - b1)
    v.mul_(b2).addcmul_(grad, grad, value=1 - b2)
    W.addcdiv_(m, v.sqrt() + eps, value=-lr_t)


# ------------------------------------------------------------------ CBOW (general kernel-chain path)
def cbow_fwd(W: torch.Tensor, who: torch.Tensor, genes: torch.Tensor,
             offsets: torch.Tensor, labels: torch.Tensor, inv_b: float,
             want_grad: bool, act: int = 0):
    """Row-gather forward: H_p = sum of W rows of the path's genes (sum, not
    mean — X is 0/1, G2Vec.py:239), o = act(H) @ who. act: 0 linear
    (reference), 1 ReLU (opt-in non-linear successor). Returns
    (loss, correct, dO|None, H|None) — H is the PRE-activation."""
    Wf = W.float()
    counts = (offsets[1:] - offsets[:-1]).long()
    P = len(counts)
    seg = torch.repeat_interleave(torch.arange(P), counts)
    H = torch.zeros(P, Wf.shape[1], dtype=torch.float32)
    H.index_add_(0, seg, Wf[genes.long()])
    o = (torch.relu(H) if act else H) @ who
    y = labels.float()
    loss = torch.clamp(o, min=0) - o * y + torch.log1p(torch.exp(-o.abs()))
    correct = ((o > 0).float() == y).float()
    if not want_grad:
        return loss, correct, None, None
    dO = (torch.sigmoid(o) - y) * inv_b
    return loss, correct, dO, H


def cbow_bwd_rows(who: torch.Tensor, genes: torch.Tensor, offsets: torch.Tensor,
                  dO: torch.Tensor, n_genes: int,
                  H_pre: torch.Tensor = None) -> torch.Tensor:
    """dW_ih = X^T (dO who^T [(.) relu_mask]): scatter-add dH rows into the
    touched gene rows. H_pre given = ReLU backward (mask = H_pre > 0)."""
    counts = (offsets[1:] - offsets[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    dH = dO[:, None] * who[None, :]
    if H_pre is not None:
        dH = dH * (H_pre > 0).float()
    dW = torch.zeros(n_genes, who.shape[0], dtype=torch.float32)
    dW.index_add_(0, genes.long(), dH[seg])
    return dW


# ------------------------------------------------------------------ graph / PCC
def pcc_edges(zt: torch.Tensor, edge_idx: torch.Tensor, n_group: int) -> torch.Tensor:
    """|PCC| per directed edge. zt: f32 [G, S_group] z-scored expression rows
    (zero rows where std==0, reproducing the pcc=0 rule of G2Vec.py:356-367)."""
    src = zt[edge_idx[:, 0].long()]
    dst = zt[edge_idx[:, 1].long()]
    return ((src * dst).sum(dim=1) / n_group).abs()


def corr_gemm(zt: torch.Tensor, n_group: int) -> torch.Tensor:
    """Full correlation matrix C = Zt Zt^T / S (the MFMA GEMM path on GPU)."""
    return (zt @ zt.t()) / n_group


# ------------------------------------------------------------------ steps 5-6: k-means / scoring
def _dist2_to(X: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """|x_g - c|^2 per row as the direct fp32 sum of squared differences
    (never the |x|^2 - 2xc + |c|^2 expansion), like row_dist2 on the GPU."""
    d = X - c
    return (d * d).sum(dim=1)


def kmeans_step(X, C, prev, labels, C_new, sums, counts, n_changed,
                inertia) -> None:
    """Mirror of kmeans_step_kernel + kmeans_fold_kernel, same
    out-arguments. Ties go to the lowest cluster index (strict <), an
    empty cluster keeps its old centroid row, C' = sums / float(counts) in
    fp32, inertia = f64 sum of the winning fp32 distances. prev may be
    labels and C_new may be C."""
    k = C.shape[0]
    best = _dist2_to(X, C[0])
    lab = torch.zeros(X.shape[0], dtype=torch.int64)
    for j in range(1, k):
        dj = _dist2_to(X, C[j])
        better = dj < best
        best = torch.where(better, dj, best)
        lab[better] = j
    n_changed[0] = int((lab != prev.long()).sum())
    inertia[0] = best.double().sum()
    s = torch.zeros(k, X.shape[1], dtype=torch.float32).index_add_(0, lab, X)
    cnt = torch.bincount(lab, minlength=k)
    new = torch.where((cnt > 0)[:, None],
                      s / cnt.clamp(min=1).float()[:, None], C)
    labels.copy_(lab.int())
    sums.copy_(s.view_as(sums))
    counts.copy_(cnt.int())
    C_new.copy_(new)


def kmeans_mind2_(X, c, d2) -> None:
    """d2[g] = min(d2[g], |x_g - c|^2) for one new centre (k-means++)."""
    torch.minimum(d2, _dist2_to(X, c.view(-1)), out=d2)


def row_norms(W: torch.Tensor) -> torch.Tensor:
    """d-score: row L2 norms accumulated in f64, rounded to fp32 once."""
    Wd = W.double()
    return (Wd * Wd).sum(dim=1).sqrt().float()


def t_scores(expr: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """|pooled-variance t| per gene column of expr[S, G], label 0 vs 1, in
    f64 with two passes (means, then squared deviations): the formula of
    scoring.t_scores and the rules of t_scores_kernel (0 when d1 <= 0 or a
    group has fewer than 2 samples)."""
    G = expr.shape[1]
    x = expr[labels == 0].double()
    y = expr[labels == 1].double()
    nx, ny = x.shape[0], y.shape[0]
    if nx < 2 or ny < 2:
        return torch.zeros(G, dtype=torch.float32)
    mx, my = x.sum(dim=0) / nx, y.sum(dim=0) / ny
    sx = (((x - mx) ** 2).sum(dim=0) / (nx - 1.0)).sqrt()
    sy = (((y - my) ** 2).sum(dim=0) / (ny - 1.0)).sqrt()
    d1 = (((nx - 1.0) * sx * sx + (ny - 1.0) * sy * sy)
          / (nx + ny - 2.0)).sqrt()
    d2 = (1.0 / nx + 1.0 / ny) ** 0.5
    pos = d1 > 0.0
    t = torch.where(pos, (mx - my) / torch.where(pos, d1, 1.0) / d2, 0.0)
    return t.abs().float()


# ------------------------------------------------------------------ rank statistics
RANK_COL_CHUNK = 1 << 15


def rank2_columns(x: np.ndarray) -> np.ndarray:
    """int64 [S, G]: the doubled average rank R2 = 2*less + equal + 1 of every
    element within its column of x [S, G] (rank_body's integer). Sort, then
    the first and last sorted position of each run of equal values: less =
    first, equal = last - first + 1. IEEE ==, so -0.0 ties +0.0."""
    x = np.asarray(x)
    S, G = x.shape
    out = np.empty((S, G), dtype=np.int64)
    pos = np.arange(S, dtype=np.int64)[:, None]
    for lo in range(0, G, RANK_COL_CHUNK):
        xc = x[:, lo:lo + RANK_COL_CHUNK]
        order = np.argsort(xc, axis=0, kind="stable")
        xs = np.take_along_axis(xc, order, axis=0)
        new = np.ones(xs.shape, dtype=bool)         # a run starts here
        new[1:] = xs[1:] != xs[:-1]
        first = np.maximum.accumulate(np.where(new, pos, 0), axis=0)
        end = np.ones(xs.shape, dtype=bool)         # a run ends here
        end[:-1] = new[1:]
        last = np.minimum.accumulate(
            np.where(end, pos, S - 1)[::-1], axis=0)[::-1]
        r2 = np.empty(xs.shape, dtype=np.int64)
        np.put_along_axis(r2, order, first + last + 2, axis=0)
        out[:, lo:lo + RANK_COL_CHUNK] = r2
    return out


def rank_columns(expr: torch.Tensor) -> torch.Tensor:
    """ranks f32 [S, G] = less + 0.5 * (equal + 1) per column (NaN-free
    input; rank_columns_kernel)."""
    r2 = rank2_columns(expr.numpy())
    return torch.from_numpy((0.5 * r2).astype(np.float32))


def ranksum_sums(expr: torch.Tensor, labels: torch.Tensor
                 ) -> Tuple[np.ndarray, np.ndarray]:
    """(2*W1, 4*SSR) int64 [G], the integer sums of ranksum_scores_kernel:
    sum_i R2_i * m_i and sum_i (R2_i - (S + 1))^2, labels 0/1 only."""
    r2 = rank2_columns(expr.numpy())
    m = labels.numpy().astype(np.int64)
    S = r2.shape[0]
    w2 = (r2 * m[:, None]).sum(axis=0)
    d = r2 - (S + 1)
    return w2, (d * d).sum(axis=0)


def ranksum_from_sums(w2: np.ndarray, q4: np.ndarray, n1: int, S: int
                      ) -> Tuple[np.ndarray, np.ndarray]:
    """f64 (|z|, auc) from the integer sums: the kernel's epilogue."""
    n1d, n0d, Sd = float(n1), float(S - n1), float(S)
    W1 = 0.5 * w2.astype(np.float64)
    z = np.zeros(w2.shape, dtype=np.float64)
    auc = np.full(w2.shape, 0.5, dtype=np.float64)
    if n1 < 2 or S - n1 < 2:
        return z, auc
    live = q4 > 0
    var = n1d * n0d / (Sd * (Sd - 1.0)) * (0.25 * q4.astype(np.float64))
    z[live] = (np.abs(W1 - 0.5 * n1d * (Sd + 1.0))[live]
               / np.sqrt(var[live]))
    auc[live] = ((W1 - 0.5 * n1d * (n1d + 1.0)) / (n1d * n0d))[live]
    return z, auc


def ranksum_scores(expr: torch.Tensor, labels: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(|z|, auc) f32 [G] of the Wilcoxon rank-sum test per gene column:
    int64 sums, the f64 epilogue, one rounding to f32. z = 0 and auc = 0.5
    for a constant gene or a group of fewer than 2 samples."""
    w2, q4 = ranksum_sums(expr, labels)
    S = expr.shape[0]
    z, auc = ranksum_from_sums(w2, q4, int(labels.sum()), S)
    return (torch.from_numpy(z.astype(np.float32)),
            torch.from_numpy(auc.astype(np.float32)))


# ------------------------------------------------------------------ step 6: permutation null of t
def splitmix64_vec(state: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """splitmix64 over a uint64 array: (new_state, random_u64), element by
    element the same bits as the scalar `splitmix64`."""
    state = np.asarray(state, dtype=np.uint64) + _SM64_GAMMA   # wraps mod 2^64
    z = state.copy()
    z = (z ^ (z >> np.uint64(30))) * _SM64_M1
    z = (z ^ (z >> np.uint64(27))) * _SM64_M2
    z = z ^ (z >> np.uint64(31))
    return state, z


PERM_TIE = 1.0 - 2.0 ** -30     # exceed: stat_perm >= stat_obs * PERM_TIE


def col_moments(expr: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(T, Q) f64 [G]: column sums of x and of the f32 product x*x of
    expr f32 [S, G], accumulated in f64 (col_moments_kernel)."""
    return expr.double().sum(dim=0), (expr * expr).double().sum(dim=0)


def _perm_t_block(expr, x2, masks, T, Q, n1: int) -> torch.Tensor:
    """stat f64 [B, G] of perm_t_body: f32 matmuls for s1 and q1, then the
    f64 formula (0 when pooled <= 0)."""
    S = expr.shape[0]
    mf = masks.float()
    s1 = (mf @ expr).double()
    q1 = (mf @ x2).double()
    n1f, n0f = float(n1), float(S - n1)
    s0, q0 = T - s1, Q - q1
    ss = (q1 - s1 * s1 / n1f) + (q0 - s0 * s0 / n0f)
    pooled = ss / float(S - 2)
    d = s0 / n0f - s1 / n1f
    pos = pooled > 0.0
    return torch.where(
        pos, d * d / torch.where(pos, pooled, 1.0) / (1.0 / n1f + 1.0 / n0f),
        0.0)


def perm_t_stats(expr: torch.Tensor, masks: torch.Tensor,
                 n1: int) -> torch.Tensor:
    T, Q = col_moments(expr)
    return _perm_t_block(expr, expr * expr, masks, T, Q, n1)


def perm_t_counts(expr: torch.Tensor, masks: torch.Tensor, n1: int,
                  stat_obs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(counts i32 [G], maxstat f64 [B]); walks the masks in row blocks so
    nothing of size G x B is held."""
    T, Q = col_moments(expr)
    x2 = expr * expr
    thr = stat_obs * PERM_TIE
    B, G = masks.shape[0], expr.shape[1]
    counts = torch.zeros(G, dtype=torch.int64)
    maxstat = torch.zeros(B, dtype=torch.float64)
    blk = max(1, min(B, (1 << 22) // max(G, 1)))
    for lo in range(0, B, blk):
        st = _perm_t_block(expr, x2, masks[lo:lo + blk], T, Q, n1)
        counts += (st >= thr).sum(dim=0)
        if G > 0:
            maxstat[lo:lo + blk] = st.max(dim=1).values
    return counts.int(), maxstat


# --------------------------------------------------------------- nearest genes
KNN_QB = 64        # query rows per matmul call (zero-padded to it)
KNN_CB = 4096      # candidate rows per matmul call


def knn_topk(Xq: torch.Tensor, X: torch.Tensor, k: int,
             q_index=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(idx i32 [Q, k], val f32 [Q, k]) of knn_tile_kernel: f32 matmul in
    candidate blocks (nothing of size Q x G is held), the self index masked
    to -inf, and a stable sort on -val, so equal values keep the lower
    candidate index (-0.0 and +0.0 tie). Missing tail: idx -1, val -inf.
    Every matmul call is KNN_QB query rows (the last block zero-padded)
    against KNN_CB candidates, whatever Q is: a BLAS may block a product by
    its shape, and a query's scores must not depend on how many others
    were asked with it."""
    Q, G, h = Xq.shape[0], X.shape[0], Xq.shape[1]
    ninf = float("-inf")
    out_val = torch.full((Q, k), ninf, dtype=torch.float32)
    out_idx = torch.full((Q, k), -1, dtype=torch.int64)
    rows = torch.arange(KNN_QB)
    for q0 in range(0, Q, KNN_QB):
        n = min(KNN_QB, Q - q0)
        xq = torch.zeros(KNN_QB, h, dtype=torch.float32)
        xq[:n] = Xq[q0:q0 + n]
        qi = torch.full((KNN_QB,), -1, dtype=torch.int64)
        if q_index is not None:
            qi[:n] = q_index[q0:q0 + n].long()
        val = torch.full((KNN_QB, k), ninf, dtype=torch.float32)
        idx = torch.full((KNN_QB, k), -1, dtype=torch.int64)
        for lo in range(0, G, KNN_CB):
            hi = min(G, lo + KNN_CB)
            sc = xq @ X[lo:hi].t()
            hit = (qi >= lo) & (qi < hi)
            sc[rows[hit], qi[hit] - lo] = ninf
            # kept entries come first and hold lower indices than the block's
            v = torch.cat([val, sc], dim=1)
            i = torch.cat([idx, torch.arange(lo, hi).expand(KNN_QB, hi - lo)],
                          dim=1)
            order = torch.sort(-v, dim=1, stable=True).indices[:, :k]
            val = torch.gather(v, 1, order)
            idx = torch.gather(i, 1, order)
        out_val[q0:q0 + n] = val[:n]
        out_idx[q0:q0 + n] = idx[:n]
    out_idx[out_val == ninf] = -1
    return out_idx.int(), out_val


# ------------------------------------------------------ L-group silhouettes
def row_sqnorms(X: torch.Tensor) -> torch.Tensor:
    """f32 [G]: squared row norms accumulated in f64, rounded to f32 once
    (row_sqnorms_kernel)."""
    Xd = X.double()
    return (Xd * Xd).sum(dim=1).float()


def cluster_dist_sums(Xq: torch.Tensor, X: torch.Tensor, labels: torch.Tensor,
                      k: int, q_index=None) -> torch.Tensor:
    """D f64 [Q, k] of cds_tile_kernel: D[q, c] = the sum over the rows g of
    X with labels[g] == c and g != q_index[q] of the f32 distance
    sqrt(max(nq[q] + nx[g] - 2 dot, 0)), added in f64. The dots are f32
    matmuls in knn_topk's fixed blocks (KNN_QB zero-padded query rows
    against KNN_CB candidates), so a query's sums do not depend on how many
    others were asked with it; nothing of size Q x G is held. An excluded
    pair contributes +0.0; an empty cluster's column is +0.0."""
    Q, G, h = Xq.shape[0], X.shape[0], Xq.shape[1]
    nq_all, nx = row_sqnorms(Xq), row_sqnorms(X)
    onehot = torch.zeros(G, k, dtype=torch.float64)
    onehot[torch.arange(G), labels.long()] = 1.0
    D = torch.zeros(Q, k, dtype=torch.float64)
    rows = torch.arange(KNN_QB)
    for q0 in range(0, Q, KNN_QB):
        n = min(KNN_QB, Q - q0)
        xq = torch.zeros(KNN_QB, h, dtype=torch.float32)
        xq[:n] = Xq[q0:q0 + n]
        nq = torch.zeros(KNN_QB, dtype=torch.float32)
        nq[:n] = nq_all[q0:q0 + n]
        qi = torch.full((KNN_QB,), -1, dtype=torch.int64)
        if q_index is not None:
            qi[:n] = q_index[q0:q0 + n].long()
        acc = torch.zeros(KNN_QB, k, dtype=torch.float64)
        for lo in range(0, G, KNN_CB):
            hi = min(G, lo + KNN_CB)
            sc = xq @ X[lo:hi].t()
            d2 = (nq[:, None] + nx[None, lo:hi]) - 2.0 * sc
            d = d2.clamp_(min=0.0).sqrt_().double()
            hit = (qi >= lo) & (qi < hi)
            d[rows[hit], qi[hit] - lo] = 0.0
            acc += d @ onehot[lo:hi]
        D[q0:q0 + n] = acc[:n]
    return D
