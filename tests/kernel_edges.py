"""Inputs and references shared by test_gpu_kernel_edges.py (GPU) and
test_kernel_edges_cpu.py (its CPU twins). Plain module, imported as a
sibling like literal_port.py.

Principle: inputs are small integers or dyadic values k/8, so every fp32
partial sum of a reduction is exact in ANY order and the kernel must equal
the fp64 reference bitwise. `exact_ref` asserts that precondition itself, so
a test cannot quietly stop being exact when a shape is edited.
"""
from __future__ import annotations

import functools
import statistics

import numpy as np
import torch

from g2vec_amd.ops import cpu_ref

F32_EXACT = float(1 << 24)      # integers below this are exact in fp32


# ------------------------------------------------------------ exactness
def exact_ref(ref64: torch.Tensor, abs_sum64: torch.Tensor,
              quantum: float) -> torch.Tensor:
    """Return ref64 after asserting the bitwise-comparison precondition:
    every term is a multiple of `quantum`, sum|terms| (in quanta) < 2^24 per
    output, hence any fp32 summation order is exact and the result is an
    fp32 value."""
    assert ref64.dtype == torch.float64 and abs_sum64.dtype == torch.float64
    q = ref64 / quantum
    assert torch.equal(q, q.round()), "terms are not multiples of the quantum"
    worst = float(abs_sum64.max()) / quantum if abs_sum64.numel() else 0.0
    assert worst < F32_EXACT, f"sum|terms| = {worst} quanta >= 2^24"
    assert torch.equal(ref64.float().double(), ref64)
    return ref64


def dyadic(gen: torch.Generator, shape, kmax: int, denom: int = 8):
    """f32 tensor of k/denom, k uniform integer in [-kmax, kmax]."""
    k = torch.randint(-kmax, kmax + 1, shape, generator=gen, dtype=torch.int32)
    return k.float() / denom


def bitwise_equal(got: torch.Tensor, ref64: torch.Tensor) -> bool:
    return torch.equal(got.detach().cpu().double(), ref64)


# ---------------------------------------------------------------- walks
def _csr_from_rows(rows):
    """rows[i] = (neighbour array, weight array) -> (row_ptr, col_idx, w)."""
    deg = np.array([len(c) for c, _ in rows], dtype=np.int64)
    rp = np.zeros(len(rows) + 1, dtype=np.int32)
    rp[1:] = np.cumsum(deg)
    ci = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows])
    w = np.concatenate([np.asarray(x, dtype=np.float32) for _, x in rows])
    return torch.from_numpy(rp), torch.from_numpy(ci), torch.from_numpy(w)


def _others(rng, G, node, deg):
    cand = np.delete(np.arange(G), node)
    return np.sort(rng.choice(cand, size=deg, replace=False))


# degrees pinned to the thresholds between the three sampling paths
# (lean <= 64 < register <= 256 < chunked) and to the 64-lane chunk edges
HUB_DEGREES = (399, 257, 258, 320, 321, 384, 385, 390)
MID_PINNED = (65, 127, 128, 129, 191, 192, 193, 255, 256)
LOW_PINNED = (1, 2, 63, 64)


def mixed_graph():
    """G = 400: 8 hubs (degree > 256, node 0 to every other node), nodes
    8..149 with degree 65..256, the rest degree 1..64, one node of degree 0
    and one whose weights are all 0. Integer weights 0..8 (zeros included):
    all weight sums are exact in fp32."""
    G = 400
    rng = np.random.default_rng(11)
    deg = np.zeros(G, dtype=np.int64)
    deg[:8] = HUB_DEGREES
    deg[8:150] = rng.integers(70, 250, size=142)
    deg[8:8 + len(MID_PINNED)] = MID_PINNED
    deg[150:] = rng.integers(1, 60, size=G - 150)
    deg[150:150 + len(LOW_PINNED)] = LOW_PINNED
    deg[398] = 0                                   # dead-end source
    deg[399] = 30                                  # all-zero weights
    rows = []
    for v in range(G):
        nb = _others(rng, G, v, int(deg[v]))
        wt = rng.integers(0, 9, size=len(nb)).astype(np.float32)
        if v == 399:
            wt[:] = 0.0
        rows.append((nb, wt))
    return _csr_from_rows(rows)


def dense_graph():
    """G = 700, degree 20..100 (lean and register paths), integer weights
    1..8: walks are long enough for len_path 200 and 512."""
    G = 700
    rng = np.random.default_rng(12)
    rows = []
    for v in range(G):
        nb = _others(rng, G, v, int(rng.integers(20, 101)))
        rows.append((nb, rng.integers(1, 9, size=len(nb)).astype(np.float32)))
    return _csr_from_rows(rows)


# name -> (graph builder, sources, num_repetition, len_path, seed)
# Seeds are picked on the CPU only: mirror (fp32 target) and oracle (double
# target) must agree on every walk. On the mixed graph seed 77 has one walk
# where the rounding moves the target across a cumulative-weight boundary
# (roughly 1e-5 per hub step), 78..81 have none.
WALK_CASES = {
    "mixed": (mixed_graph, lambda: torch.arange(400, dtype=torch.int32),
              2, 100, 79),
    "len200": (dense_graph,
               lambda: torch.arange(5, 700, 22, dtype=torch.int32)[:32],
               1, 200, 78),
    "len512": (dense_graph,
               lambda: torch.arange(9, 700, 22, dtype=torch.int32)[:32],
               1, 512, 79),
}


@functools.lru_cache(maxsize=None)
def walk_case(name: str):
    """(row_ptr, col_idx, w, sources, num_rep, len_path, seed, oracle) with
    oracle = cpu_ref.random_walks(...) computed once per process."""
    build, src, rep, L, seed = WALK_CASES[name]
    rp, ci, w = build()
    s = src()
    oracle = cpu_ref.random_walks(rp, ci, w, s, rep, L, seed)
    return rp, ci, w, s, rep, L, seed, oracle


def steps_per_sampling_path(rp, nodes):
    """Sampling steps the walks took through (lean, register, chunked) rows,
    counted from a walk output: every visited node of degree > 0 samples."""
    deg = (rp[1:] - rp[:-1]).numpy()
    visited = nodes.numpy()
    d = deg[visited[visited >= 0]]
    return (int(((d > 0) & (d <= 64)).sum()),
            int(((d > 64) & (d <= 256)).sum()), int((d > 256).sum()))


def mirror_walks(row_ptr, col_idx, weights, sources, num_repetition,
                 len_path, seed, f32_target=True, weight_shift=0):
    """Independent re-statement of cpu_ref.random_walks with the ONE known
    kernel difference: the kernel rounds `target` to fp32, the oracle keeps
    it in double. The CPU twin asserts mirror == oracle on every walk of the
    inputs used on the GPU, so a GPU mismatch there is the kernel's.

    weight_shift != 0 reads the weight row off by that many entries (the
    `wgt[j]`-for-`wgt[s + j]` class of indexing bug) - used only to show
    the comparison has teeth."""
    rp = row_ptr.numpy()
    ci = col_idx.numpy()
    w = weights.numpy().astype(np.float32)
    src = sources.numpy()
    n_src = len(src)
    n_walks = n_src * num_repetition
    G = len(rp) - 1
    with np.errstate(over="ignore"):
        ghash = np.array([cpu_ref.gene_hash(g) for g in range(G)],
                         dtype=np.uint64)
    nodes = np.full((n_walks, len_path), -1, dtype=np.int32)
    lengths = np.zeros(n_walks, dtype=np.int32)
    hashes = np.zeros(n_walks, dtype=np.int64)
    seen = np.zeros(G, dtype=bool)
    for wid in range(n_walks):
        rep = wid // n_src
        source = int(src[wid % n_src])
        with np.errstate(over="ignore"):
            gid = (np.uint64(source) * np.uint64(num_repetition)
                   + np.uint64(rep))
            state = np.uint64(seed) ^ np.uint64(
                gid * np.uint64(0x94D049BB133111EB) + np.uint64(1))
        state, _ = cpu_ref.splitmix64(state)
        seen[:] = False
        cur, path = source, []
        for _ in range(len_path):
            path.append(cur)
            seen[cur] = True
            s, e = int(rp[cur]), int(rp[cur + 1])
            if e <= s:
                break
            nb = ci[s:e]
            lo = min(max(s + weight_shift, 0), len(w) - (e - s))
            wt = np.where(seen[nb], np.float32(0), w[lo:lo + (e - s)])
            tot = float(np.sum(wt, dtype=np.float32))
            state, r = cpu_ref.splitmix64(state)
            if tot <= 0.0:
                break
            u = float(r >> np.uint64(11)) * (1.0 / 9007199254740992.0)
            target = u * tot
            if f32_target:
                target = float(np.float32(target))
            c = np.cumsum(wt, dtype=np.float32)
            j = int(np.searchsorted(c, target, side="right"))
            if j >= len(nb) or wt[j] <= 0.0:
                j = int(np.flatnonzero(wt > 0.0)[-1])
            cur = int(nb[j])
        nodes[wid, :len(path)] = path
        lengths[wid] = len(path)
        with np.errstate(over="ignore"):
            hashes[wid] = np.sum(ghash[path], dtype=np.uint64).astype(np.int64)
    return (torch.from_numpy(nodes), torch.from_numpy(lengths),
            torch.from_numpy(hashes))


# ---- first-step sampling distribution
DIST_SOURCES = (1, 2, 3)          # degree 40 / 200 / 300: one per path
DIST_REPS = 30000
DIST_SEED = 5


@functools.lru_cache(maxsize=None)
def distribution_graph():
    """Sources 1, 2, 3 (degree 40, 200, 300; all at non-zero CSR offsets
    behind node 0's row) point at sink nodes of degree 0, so a len_path-2
    walk is exactly one sampling step. Real-valued weights uniform(0.2, 1)
    with exact zeros at the row ends and across the lane-63/64 boundary."""
    rng = np.random.default_rng(13)
    G = 420
    sinks = np.arange(10, G)
    rows = [(sinks[:7], rng.uniform(0.2, 1.0, 7))]
    for deg in (40, 200, 300):
        nb = np.sort(rng.choice(sinks, size=deg, replace=False))
        wt = rng.uniform(0.2, 1.0, deg).astype(np.float32)
        zeros = [0, deg - 1, deg // 2] + ([63, 64] if deg > 65 else [])
        wt[zeros] = 0.0
        rows.append((nb, wt))
    rows += [(np.zeros(0, np.int32), np.zeros(0, np.float32))] * (G - 4)
    return _csr_from_rows(rows)


def chi2_upper_quantile(df: int, p: float = 1e-6) -> float:
    """Upper-p quantile of chi-square(df), Wilson-Hilferty approximation."""
    z = statistics.NormalDist().inv_cdf(1.0 - p)
    a = 2.0 / (9.0 * df)
    return df * (1.0 - a + z * a ** 0.5) ** 3


def first_step_chi2(rp, ci, w, nodes):
    """Per source of DIST_SOURCES: (chi2 over the positive-weight
    neighbours, df, count landed on zero-weight neighbours, count of walks
    that did not step). nodes: [DIST_REPS * 3, 2] walk output."""
    rp, ci, w = rp.numpy(), ci.numpy(), w.numpy().astype(np.float64)
    nodes = nodes.numpy()
    out = []
    for pos, srcn in enumerate(DIST_SOURCES):
        rows = nodes[pos::len(DIST_SOURCES)]
        assert rows.shape[0] == DIST_REPS and np.all(rows[:, 0] == srcn)
        s, e = rp[srcn], rp[srcn + 1]
        first = rows[:, 1]
        cnt = np.bincount(first[first >= 0], minlength=int(rp.shape[0]))
        obs = cnt[ci[s:e]].astype(np.float64)
        pos_w = w[s:e] > 0
        expct = DIST_REPS * w[s:e][pos_w] / w[s:e][pos_w].sum()
        chi2 = float((((obs[pos_w] - expct) ** 2) / expct).sum())
        out.append((chi2, int(pos_w.sum()) - 1, int(obs[~pos_w].sum()),
                    int((first < 0).sum()) + int(cnt.sum() - obs.sum())))
    return out


# ------------------------------------------------------------ path sets
CBOW_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 80)
CBOW_G = 300


@functools.lru_cache(maxsize=None)
def cbow_pathset(P: int = 2003, short: bool = False, seed: int = 21):
    """(genes i32, offsets i32, labels f32). Lengths cycle through the
    16-lane sub-wave edges 1/15/16/17/31/32/33 and ~80 (75..85); short=True
    gives lengths 1..4 for the large-P grid-stride case."""
    rng = np.random.default_rng(seed)
    if short:
        lens = 1 + (np.arange(P) % 4)
    else:
        lens = np.array(CBOW_LENGTHS)[rng.integers(0, 8, size=P)]
        lens = np.where(lens == 80, rng.integers(75, 86, size=P), lens)
        lens[:8] = CBOW_LENGTHS                      # every edge present
    if short:
        genes = rng.integers(0, CBOW_G, size=int(lens.sum()))
    else:                                  # distinct genes within a path
        order = np.argsort(rng.random((P, CBOW_G)), axis=1)
        genes = np.concatenate([order[p, :lens[p]] for p in range(P)])
    offs = np.zeros(P + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    labels = rng.integers(0, 2, size=P).astype(np.float32)
    return (torch.from_numpy(genes.astype(np.int32)),
            torch.from_numpy(offs.astype(np.int32)),
            torch.from_numpy(labels))


def cbow_scalar_ref64(s, genes, offs, labels, inv_b):
    """fp64 reference of the collapsed CBOW forward. s must be dyadic (k/8)
    so o is exact: returns (o, loss, correct, dO), o checked by exact_ref."""
    counts = (offs[1:] - offs[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    sg = s.double()[genes.long()]
    o = torch.zeros(len(counts), dtype=torch.float64).index_add_(0, seg, sg)
    a = torch.zeros(len(counts), dtype=torch.float64).index_add_(
        0, seg, sg.abs())
    o = exact_ref(o, a, 1.0 / 8)
    # the loss is held to 1e-5 absolute: keep the fp32 result's own
    # half-ulp (7.6e-6 below 256) under it
    assert float(o.abs().max()) < 128.0
    y = labels.double()
    loss = torch.clamp(o, min=0) - o * y + torch.log1p(torch.exp(-o.abs()))
    correct = ((o > 0).double() == y).double()
    dO = (torch.sigmoid(o) - y) * inv_b
    return o, loss, correct, dO


def cbow_general_ref64(W, who, genes, offs, labels, inv_b, act=0):
    """fp64 reference of the row-gather forward for dyadic W and who:
    H (k/8) and o (k/64) are exact. Returns (H, loss, correct, dO)."""
    counts = (offs[1:] - offs[:-1]).long()
    P = len(counts)
    seg = torch.repeat_interleave(torch.arange(P), counts)
    rows = W.double()[genes.long()]
    H = torch.zeros(P, W.shape[1], dtype=torch.float64).index_add_(
        0, seg, rows)
    Ha = torch.zeros(P, W.shape[1], dtype=torch.float64).index_add_(
        0, seg, rows.abs())
    H = exact_ref(H, Ha, 1.0 / 8)
    A = torch.relu(H) if act else H
    o = exact_ref(A @ who.double(), Ha @ who.double().abs(), 1.0 / 64)
    # the loss is held to 1e-5 absolute: keep the fp32 result's own
    # half-ulp (7.6e-6 below 256) under it
    assert float(o.abs().max()) < 128.0
    y = labels.double()
    loss = torch.clamp(o, min=0) - o * y + torch.log1p(torch.exp(-o.abs()))
    correct = ((o > 0).double() == y).double()
    return H, loss, correct, (torch.sigmoid(o) - y) * inv_b


def dO_tol(inv_b: float) -> float:
    """The project's dO tolerance (1e-7 at inv_b = 1/500), scaled."""
    return 1e-7 * inv_b * 500.0


SEG_SIZES = (5000, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513)
SEG_P = 5003
SEG_G = 214          # genes 11 and 213 (the highest index) are in no path


@functools.lru_cache(maxsize=None)
def segment_pathset():
    """Path set whose per-gene instance counts hit the 4x64 unroll edges of
    the segment kernels: gene k < 11 appears in SEG_SIZES[k] paths (gene 0
    is the ~5000-instance hub), genes 12..212 are ~25-instance fillers that
    keep every path non-empty, genes 11 and 213 appear nowhere."""
    rng = np.random.default_rng(22)
    pp, gg = [], []
    for g, n in enumerate(SEG_SIZES):
        pp.append(rng.choice(SEG_P, size=n, replace=False))
        gg.append(np.full(n, g))
    pp.append(np.arange(SEG_P))
    gg.append(12 + (np.arange(SEG_P) * 7) % 201)
    pp, gg = np.concatenate(pp), np.concatenate(gg)
    order = np.lexsort((rng.random(len(pp)), pp))    # by path, genes shuffled
    pp, gg = pp[order], gg[order]
    offs = np.zeros(SEG_P + 1, dtype=np.int64)
    offs[1:] = np.cumsum(np.bincount(pp, minlength=SEG_P))
    sizes = np.bincount(gg, minlength=SEG_G)
    assert tuple(sizes[:11]) == SEG_SIZES and sizes[11] == 0
    assert sizes[SEG_G - 1] == 0 and np.all(np.diff(offs) >= 1)
    return (torch.from_numpy(gg.astype(np.int32)),
            torch.from_numpy(offs.astype(np.int32)))


def scatter_ref64(genes, offs, dO, n_genes):
    counts = (offs[1:] - offs[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    d = dO.double()[seg]
    c = torch.zeros(n_genes, dtype=torch.float64).index_add_(
        0, genes.long(), d)
    a = torch.zeros(n_genes, dtype=torch.float64).index_add_(
        0, genes.long(), d.abs())
    return exact_ref(c, a, 1.0)


def bwd_rows_ref64(who, genes, offs, dO, n_genes, H_pre=None):
    counts = (offs[1:] - offs[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    dH = dO.double()[:, None] * who.double()[None, :]
    if H_pre is not None:
        dH = dH * (H_pre > 0).double()
    rows = dH[seg]
    dW = torch.zeros(n_genes, who.numel(), dtype=torch.float64).index_add_(
        0, genes.long(), rows)
    a = torch.zeros(n_genes, who.numel(), dtype=torch.float64).index_add_(
        0, genes.long(), rows.abs())
    return exact_ref(dW, a, 1.0 / 8)


# ----------------------------------------------------------------- GEMV
def mv_ref64(W, x):
    """W @ x in fp64 for dyadic (k/8) W and x; products are k/64."""
    ref = torch.mv(W.double(), x.double())
    a = torch.mv(W.double().abs(), x.double().abs())
    return exact_ref(ref, a, 1.0 / 64)


# ----------------------------------------------------------------- Adam
def f32(x: float) -> float:
    return float(np.float32(x))


def adam_ref64(W, m, v, grad64, lr_t, b1, b2, eps):
    """TF1 Adam in fp64 on the hyper-parameters as the kernels receive
    them (fp32-rounded lr_t / b1 / b2 / eps). Returns new (W, m, v)."""
    lr_t, b1, b2, eps = f32(lr_t), f32(b1), f32(b2), f32(eps)
    m2 = b1 * m.double() + (1.0 - b1) * grad64
    v2 = b2 * v.double() + (1.0 - b2) * grad64 * grad64
    W2 = W.double() - lr_t * m2 / (v2.sqrt() + eps)
    return W2, m2, v2


def adam_inputs(G: int, h: int, seed: int):
    """Inputs sized so the project's absolute Adam tolerances (1e-6 / 1e-7 /
    1e-7 on W / m / v against fp64) follow from fp32 precision alone:
    |m'| <= 0.14 (ulp 1.5e-8, three roundings), v' <= 0.011 (ulp 9e-10),
    |W'| <= 1.1 with an update <= 0.02 (a few ulp of 1.2e-7).
    W and c are dyadic so the fused variant's W^T c is exact; |who| >= 0.25
    and |mO| <= 1e-4 keep the who / mO results free of cancellation, so
    their rtol is meaningful."""
    gen = torch.Generator().manual_seed(seed)
    W = dyadic(gen, (G, h), 8)
    c = dyadic(gen, (G,), 4)
    m = (torch.rand(G, h, generator=gen) - 0.5) * 0.2
    v = 0.001 + torch.rand(G, h, generator=gen) * 0.009
    sign = torch.randint(0, 2, (h,), generator=gen).float() * 2 - 1
    who = sign * (0.25 + 0.75 * torch.rand(h, generator=gen))
    mO = (torch.rand(h, generator=gen) - 0.5) * 2e-4
    vO = 0.001 + torch.rand(h, generator=gen) * 0.009
    return W, m, v, c, who, mO, vO


# ------------------------------------------------------------------ PCC
def int_rows(G: int, S: int, seed: int, zero_row=None):
    rng = np.random.default_rng(seed)
    z = rng.integers(-8, 9, size=(G, S)).astype(np.float32)
    if zero_row is not None:
        z[zero_row] = 0.0
    return torch.from_numpy(z)


def corr_ref64(zt, n_group):
    z = zt.double()
    return exact_ref((z @ z.t()) / n_group, (z.abs() @ z.abs().t()) / n_group,
                     1.0 / n_group)


def pcc_ref64(zt, edges, n_group):
    a = zt.double()[edges[:, 0].long()]
    b = zt.double()[edges[:, 1].long()]
    return exact_ref(((a * b).sum(1) / n_group).abs(),
                     (a * b).abs().sum(1) / n_group, 1.0 / n_group)


# ----------------------------------------------------------------- bf16
BF16_FINITE_BITS = (
    0x00000000, 0x80000000,             # +-0
    0x3F800000, 0xBF800000,             # +-1
    0x3F808000, 0xBF808000,             # exact tie, even mantissa: down
    0x3F818000, 0xBF818000,             # exact tie, odd mantissa: up
    0x3F807FFF, 0x3F808001,             # one ulp either side of a tie
    0x3F7F8000,                         # tie that carries into the exponent
    0x7F7FFFFF, 0xFF7FFFFF,             # max finite -> +-inf
    0x7F7F7FFF, 0x7F7F8000,             # largest that stays finite / tie up
    0x7F800000, 0xFF800000,             # +-inf
    0x00000001, 0x80000001,             # smallest subnormals
    0x00008000, 0x00018000,             # subnormal ties (down / up)
    0x007FFFFF, 0x807FFFFF,             # largest subnormals -> min normal
    0x00800000,                         # min normal
)
BF16_NAN_BITS = (
    0x7FC00000, 0xFFC00000,             # default quiet NaN, both signs
    0x7FFFFFFF, 0xFFFFFFFF,             # full payload
    0x7F800001, 0xFF800001,             # payload only below the bf16 cut
    0x7FFF8000, 0x7F80FFFF,
)


def bits_to_f32(bits) -> torch.Tensor:
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32))
