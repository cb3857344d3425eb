"""Inputs and references shared by test_gpu_scale.py (GPU) and
test_scale_cases_cpu.py (its CPU twins). Plain module, imported as a sibling
like kernel_edges.py.

The scale tier runs the kernels where the launch geometry itself changes:
past the 2^20-block cap of `grid_for` (a second, ragged grid-stride sweep),
past flat element index 2^31 and past the natural slab threshold of the
scatter plans. Inputs of that size cannot be checked element by element
against an fp64 reference on the host, so every builder here is a small
periodic pattern (periods 7, 13, 127, 130, 1021: none divides 256, 2^20 or a
grid stride) and every reference is a closed form of the pattern: computed in
fp64 / int64 over ONE period with the existing references of kernel_edges.py,
then expanded by indexing. A wrong element index lands on another residue of
the period, hence on another expected value.

Each builder takes the size and the device, so the CPU twins run the same
code at a few thousand rows and prove closed form == existing fp64 reference
over the whole reduced output. That proof is what entitles the GPU tests to
use the closed form at full size."""
from __future__ import annotations

import functools

import numpy as np
import torch

import kernel_edges as ke
from g2vec_amd.ops import cpu_ref

# grid_for(work, per_block) caps the grid at 2^20 blocks of 256 threads
GRID_CAP = 1 << 20
CAP_W = 4 * GRID_CAP          # wave-per-item launches: 4 waves per block
CAP_E = 256 * GRID_CAP        # thread-per-element launches
CHUNK = 1 << 26               # most elements one device comparison touches
PERIOD = 1021                 # prime
N_GROUP = 64                  # power of two: the 1 / n_group scaling is exact


def windows(n: int, boundary: int, width: int = 64):
    """The (lo, hi) row ranges read back to the host: head, boundary
    (starting 32 rows before `boundary`) and tail."""
    assert width <= boundary - 32 and boundary + 1 <= n
    return {"head": (0, width),
            "boundary": (boundary - 32, min(n, boundary - 32 + width)),
            "tail": (n - width, n)}


def chunks(n_rows: int, row_elems: int = 1, most: int = CHUNK):
    """Row ranges of at most `most` (<= CHUNK) elements covering
    [0, n_rows)."""
    assert most <= CHUNK
    step = max(1, most // row_elems)
    return [(a, min(n_rows, a + step)) for a in range(0, n_rows, step)]


# ================================================================ walks
WALK_NODES = 8
WALK_REPS = CAP_W // WALK_NODES + 1          # 524 289: n_walks = CAP_W + 8
WALK_LEN = 3
WALK_SEED = 91
WALK_SUB_SOURCE = 5


def ring_graph():
    """8 nodes, node i has the single out-edge i -> i + 1 (mod 8), weight 1:
    every walk is determined by its source."""
    rp = torch.arange(WALK_NODES + 1, dtype=torch.int32)
    ci = ((torch.arange(WALK_NODES) + 1) % WALK_NODES).int()
    return rp, ci, torch.ones(WALK_NODES)


@functools.lru_cache(maxsize=None)
def ring_hashes() -> torch.Tensor:
    """i64 [8]: cpu_ref.path_hash of the 8 possible triples, by source."""
    return torch.tensor(
        [int(cpu_ref.path_hash([(s + k) % WALK_NODES
                                for k in range(WALK_LEN)]))
         for s in range(WALK_NODES)], dtype=torch.int64)


def ring_expected(lo: int, hi: int, device):
    """Closed form of rows [lo, hi) of the ring run with sources
    arange(8): row w is [s, s + 1, s + 2] (mod 8) with s = w % 8."""
    s = torch.arange(lo, hi, device=device) % WALK_NODES
    nodes = torch.stack([(s + k) % WALK_NODES for k in range(WALK_LEN)],
                        dim=1).int()
    lengths = torch.full((hi - lo,), WALK_LEN, dtype=torch.int32,
                         device=device)
    return nodes, lengths, ring_hashes().to(device)[s]


def _graph(rows):
    return ke._csr_from_rows([(np.asarray(c), np.asarray(w, dtype=np.float32))
                              for c, w in rows])


def sampled_graph(name: str):
    """`deg3`: every node has out-degree 3, integer weights 1..4, so every
    walk reaches len_path 3. `stops`: nodes 1 and 6 have out-degree 2 with
    one edge back to themselves (a walk that steps onto them from their other
    neighbour has nowhere left to go: length 2, one -1 pad), node 3 has
    out-degree 0 (length 1, two pads)."""
    rows = [([(v + 1) % 8, (v + 3) % 8, (v + 6) % 8],
             [1 + (v % 4), 1 + ((v + 1) % 4), 1 + ((3 * v + 2) % 4)])
            for v in range(WALK_NODES)]
    if name == "stops":
        rows[1] = ([1, 2], [2, 3])            # self-loop + node 2
        rows[6] = ([4, 6], [1, 4])            # node 4 + self-loop
        rows[3] = ([], [])
        rows[2] = ([1, 3, 5], [4, 1, 2])      # feeds the stops
        rows[4] = ([3, 6, 7], [1, 3, 2])
    else:
        assert name == "deg3"
    rows = [(sorted(zip(c, w))) for c, w in rows]
    rows = [([c for c, _ in r], [w for _, w in r]) for r in rows]
    return _graph(rows)


def walk_tables(rp, ci, w, device):
    """Small device tables of the validity check: positive-weight adjacency
    (bool [8, 8]), out-neighbour bit mask per node (i64 [8]) and the per-node
    hash terms with a zero at index 8 for the -1 pad (i64 [9])."""
    n = rp.numel() - 1
    adj = torch.zeros(n, n, dtype=torch.bool)
    bits = [0] * n
    for v in range(n):
        for e in range(int(rp[v]), int(rp[v + 1])):
            if float(w[e]) > 0:
                adj[v, int(ci[e])] = True
                bits[v] |= 1 << int(ci[e])
    nbr = torch.tensor(bits, dtype=torch.int64)
    with np.errstate(over="ignore"):
        gh = [int(np.uint64(cpu_ref.gene_hash(g)).astype(np.int64))
              for g in range(n)] + [0]
    return adj.to(device), nbr.to(device), torch.tensor(
        gh, dtype=torch.int64, device=device)


def walks_valid(nodes, lengths, hashes, sources, tables) -> dict:
    """Tensor-op check (any device) that every row is a non-revisiting walk
    of the graph: row w starts at sources[w % n_src], every step follows a
    positive-weight edge to an unvisited node, a walk shorter than len_path
    stopped only with no unvisited out-neighbour left, the tail is -1 and the
    hash is the sum of its nodes' terms. Returns name -> bool."""
    adj, nbr, gh = tables
    n, L = nodes.shape
    assert L == WALK_LEN
    nd = nodes.long()
    ln = lengths.long()
    # the table lookups below need in-range indices: settle that first
    if not (bool(((nd >= -1) & (nd < adj.shape[0])).all())
            and bool((nd[:, 0] >= 0).all())):
        return {"range": False}
    wid = torch.arange(n, device=nodes.device)
    src = sources.long().to(nodes.device)[wid % sources.numel()]
    ok = {"start": bool((nd[:, 0] == src).all()),
          "length": bool(((ln >= 1) & (ln <= L)).all())}
    seen = torch.ones_like(ln) << nd[:, 0]
    edge = torch.ones(n, dtype=torch.bool, device=nodes.device)
    fresh = edge.clone()
    pad = edge.clone()
    for k in range(1, L):
        live = k < ln
        a, b = nd[:, k - 1].clamp(min=0), nd[:, k].clamp(min=0)
        edge &= ~live | ((nd[:, k] >= 0) & adj[a, b])
        bit = torch.ones_like(ln) << b
        fresh &= ~live | ((seen & bit) == 0)
        seen = torch.where(live, seen | bit, seen)
        pad &= live | (nd[:, k] == -1)
    last = nd.gather(1, (ln - 1).clamp(0, L - 1)[:, None])[:, 0].clamp(min=0)
    ok["edge"] = bool(edge.all())
    ok["no_revisit"] = bool(fresh.all())
    ok["pad"] = bool(pad.all())
    ok["stop"] = bool(((ln == L) | ((nbr[last] & ~seen) == 0)).all())
    ok["hash"] = bool((gh[nd].sum(dim=1) == hashes).all())   # -1 -> gh[8]
    return ok


# ================================================================== PCC
PCC_G, PCC_S, PCC_ZERO_ROW = 130, 65, 17
PCC_FORCED = ((PCC_G - 1, PCC_G - 1), (PCC_G - 1, 0), (0, PCC_G - 1),
              (PCC_ZERO_ROW, PCC_ZERO_ROW), (64, 64))


@functools.lru_cache(maxsize=None)
def pcc_rows():
    return ke.int_rows(PCC_G, PCC_S, seed=65, zero_row=PCC_ZERO_ROW)


def pcc_edge_list(E: int, device) -> torch.Tensor:
    """i32 [E, 2]: src = e % 127, dst = (7 e + 3) % 130; the last five rows
    hold the highest index on either side, self-pairs and the zero row."""
    e = torch.arange(E, device=device)
    edges = torch.stack([e % 127, (e * 7 + 3) % PCC_G], dim=1).int()
    edges[E - len(PCC_FORCED):] = torch.tensor(PCC_FORCED, dtype=torch.int32,
                                               device=device)
    return edges.contiguous()


@functools.lru_cache(maxsize=None)
def pcc_table() -> torch.Tensor:
    """f64 [130, 130]: |z_a . z_b| / n_group for every pair, through
    ke.corr_ref64 (so exact in fp32 in any summation order)."""
    return ke.corr_ref64(pcc_rows(), N_GROUP).abs()


def pcc_expected(edges: torch.Tensor) -> torch.Tensor:
    """f32 on edges' device: the table gathered by edge."""
    t = pcc_table().float().to(edges.device)
    return t[edges[:, 0].long(), edges[:, 1].long()]


# ======================================================== general CBOW
CBOW_H = 512
CBOW_P = CAP_W + 3            # CBOW_P * 512 = 2^31 + 1536 elements of H
CBOW_CLASSES = 2 * PERIOD     # p % 2042 fixes parity, genes and label
CBOW_INV_B = 1 / 500
DO_PERIOD = 7
BWD_CLASSES = CBOW_CLASSES * DO_PERIOD       # 14 294: (path class, dO)


def cbow_second_gene(p: torch.Tensor) -> torch.Tensor:
    """Second gene of odd path p: (3p + 1) % 1021, moved one up in the one
    residue class (p = 1531 mod 2042) where that equals the first gene."""
    first = p % PERIOD
    second = (3 * p + 1) % PERIOD
    return torch.where(second == first, (second + 1) % PERIOD, second)


def cbow_paths(lo: int, hi: int, device):
    """(genes i32, offsets i32, labels f32) of paths lo <= p < hi: even p is
    [p % 1021], odd p is [p % 1021, second gene]; label p % 2."""
    p = torch.arange(lo, hi, device=device)
    odd = (p % 2) == 1
    offs = torch.zeros(hi - lo + 1, dtype=torch.int64, device=device)
    torch.cumsum(1 + odd.long(), 0, out=offs[1:])
    genes = torch.empty(int(offs[-1]), dtype=torch.int32, device=device)
    genes[offs[:-1]] = (p % PERIOD).int()
    genes[offs[:-1][odd] + 1] = cbow_second_gene(p[odd]).int()
    return genes, offs.int().contiguous(), (p % 2).float()


@functools.lru_cache(maxsize=None)
def cbow_tables(h: int = CBOW_H):
    """W: integers -2..2 [1021, h] (exact in bf16 and fp16 too); who: k/8,
    |k| <= 4."""
    gen = torch.Generator().manual_seed(1021 + h)
    W = torch.randint(-2, 3, (PERIOD, h), generator=gen).float()
    return W, ke.dyadic(gen, (h,), 4)


@functools.lru_cache(maxsize=None)
def cbow_class_ref(h: int = CBOW_H):
    """ke.cbow_general_ref64 (ReLU) over the 2042 path classes: fp64
    (H [2042, h], loss, correct, dO); path p has class p % 2042."""
    W, who = cbow_tables(h)
    genes, offs, labels = cbow_paths(0, CBOW_CLASSES, "cpu")
    return ke.cbow_general_ref64(W, who, genes, offs, labels, CBOW_INV_B,
                                 act=1)


def cbow_bwd_dO(lo: int, hi: int, device) -> torch.Tensor:
    """Crafted integer upstream gradient dO[p] = p % 7 - 3."""
    return ((torch.arange(lo, hi, device=device) % DO_PERIOD) - 3).float()


def cbow_bwd_ref(P: int, h: int = CBOW_H) -> torch.Tensor:
    """f64 [1021, h]: dW[g, j] = who[j] * sum over paths p < P holding g of
    dO_p * 1[H[p, j] > 0], from the 14 294 (path class, dO) classes: class c
    occurs P // 14294 (+ 1 for c < P % 14294) times. int64 sums, np.add.at
    over the instances of one period, then ke.exact_ref (quantum 1/8)."""
    W, who = cbow_tables(h)
    H = cbow_class_ref(h)[0]
    genes, offs, _ = cbow_paths(0, BWD_CLASSES, "cpu")
    c = np.arange(BWD_CLASSES)
    n_c = P // BWD_CLASSES + (c < P % BWD_CLASSES)
    coef = n_c * ((c % DO_PERIOD) - 3)                      # int64 [classes]
    mask = (H > 0).numpy().astype(np.int64)                 # [2042, h]
    inst_c = np.repeat(c, np.diff(offs.numpy()))
    g = genes.numpy().astype(np.int64)
    S = np.zeros((PERIOD, h), dtype=np.int64)
    A = np.zeros((PERIOD, h), dtype=np.int64)
    term = coef[inst_c, None] * mask[inst_c % CBOW_CLASSES]
    np.add.at(S, g, term)
    # the kernel adds a class's n_c copies one by one; |coef| = n_c * |dO|
    # is the sum of their magnitudes
    np.add.at(A, g, np.abs(term))
    w64 = who.double()
    return ke.exact_ref(torch.from_numpy(S).double() * w64[None, :],
                        torch.from_numpy(A).double() * w64.abs()[None, :],
                        1.0 / 8)


# =========================================================== elementwise
ELEM_N = CAP_E + 257


def tile_into(out: torch.Tensor, pattern: torch.Tensor) -> torch.Tensor:
    """out[i] = pattern[i % len(pattern)] without a temporary of out's size."""
    per = pattern.numel()
    k = out.numel() // per
    pat = pattern.to(out.device)
    out[:k * per].view(k, per).copy_(pat[None, :])
    out[k * per:] = pat[:out.numel() - k * per]
    return out


def tiled(n: int, pattern: torch.Tensor, device) -> torch.Tensor:
    return tile_into(torch.empty(n, dtype=pattern.dtype, device=device),
                     pattern)


def tile_max_err(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """max |got[i] - ref64[i % period]| in fp64 on got's device, at most
    CHUNK elements at a time."""
    per = ref64.numel()
    ref = ref64.to(got.device)
    k = got.numel() // per
    worst = 0.0
    for a, b in chunks(k, per, CHUNK // 4):      # fp64 temporaries: 2^24
        d = got[a * per:b * per].view(b - a, per).double() - ref[None, :]
        worst = max(worst, float(d.abs().max()))
    tail = got[k * per:]
    if tail.numel():
        worst = max(worst, float((tail.double() - ref[:tail.numel()])
                                 .abs().max()))
    return worst


def as_bits(t: torch.Tensor) -> torch.Tensor:
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def tile_equal(got: torch.Tensor, pattern: torch.Tensor) -> bool:
    """got[i] is bitwise pattern[i % period] for every i (same dtype,
    compared as raw bits: -0.0 != +0.0), at most CHUNK elements at a time."""
    per = pattern.numel()
    assert pattern.dtype == got.dtype
    pat = as_bits(pattern.contiguous()).to(got.device)
    got = as_bits(got)
    k = got.numel() // per
    for a, b in chunks(k, per):
        if not bool((got[a * per:b * per].view(b - a, per)
                     == pat[None, :]).all()):
            return False
    tail = got[k * per:]
    return torch.equal(tail, pat[:tail.numel()])


ADAM_HP = dict(t=5, lr=0.005, b1=0.9, b2=0.999, eps=1e-8)


@functools.lru_cache(maxsize=None)
def adam_patterns():
    """One period of (W, m, v, grad) in the value ranges of
    test_adam_dense_ragged_vs_fp64."""
    gen = torch.Generator().manual_seed(PERIOD)
    W = torch.rand(PERIOD, generator=gen) * 2 - 1
    m = (torch.rand(PERIOD, generator=gen) - 0.5) * 0.2
    v = 0.001 + torch.rand(PERIOD, generator=gen) * 0.009
    grad = torch.rand(PERIOD, generator=gen) - 0.5
    return W, m, v, grad


def adam_lr_t() -> float:
    from g2vec_amd import ops
    return ops.tf1_lr_t(ADAM_HP["lr"], ADAM_HP["b1"], ADAM_HP["b2"],
                        ADAM_HP["t"])


@functools.lru_cache(maxsize=None)
def adam_period_ref():
    """ke.adam_ref64 over one period: fp64 (W', m', v') [1021]."""
    W, m, v, grad = adam_patterns()
    return ke.adam_ref64(W, m, v, grad.double(), adam_lr_t(), ADAM_HP["b1"],
                         ADAM_HP["b2"], ADAM_HP["eps"])


@functools.lru_cache(maxsize=None)
def bf16_pattern() -> torch.Tensor:
    """f32 [1021]: ke.BF16_FINITE_BITS, then random finite bit patterns."""
    rng = np.random.default_rng(16)
    bits = rng.integers(0, 1 << 32, size=4 * PERIOD, dtype=np.uint64)
    bits = bits[((bits >> 23) & 0xFF) != 0xFF].astype(np.uint32)
    n_rand = PERIOD - len(ke.BF16_FINITE_BITS)
    assert len(bits) >= n_rand
    pat = torch.cat([ke.bits_to_f32(ke.BF16_FINITE_BITS),
                     torch.from_numpy(bits[:n_rand].view(np.float32).copy())])
    assert pat.numel() == PERIOD and not bool(torch.isnan(pat).any())
    return pat


TN_STD = 0.8796257            # std of a +-2 sigma truncated standard normal
TN_SIGMA = 1.0 / np.sqrt(128.0)
TN_SEED = 1234
TN_WINDOW = (CAP_E - 2048, ELEM_N)


# ============================================================ slab plans
SLAB_PATHS = (3 << 20) // 4                  # ops.SLAB_BYTES // 4 = 786 432
SLAB_P = 2 * SLAB_PATHS + 5                  # three slabs, the last 5 paths
SLAB_DO = 13


def slab_paths(P: int, device):
    """(genes i32, offsets i32): path p has 1 + p % 3 genes
    (5p + 1 + k * (1 + p % 337)) % 1021, k = 0, 1, 2: distinct within a
    path because 3 * 337 < 1021."""
    p = torch.arange(P, device=device)
    lens = 1 + p % 3
    offs = torch.zeros(P + 1, dtype=torch.int64, device=device)
    torch.cumsum(lens, 0, out=offs[1:])
    path_of = torch.repeat_interleave(p, lens)
    k = torch.arange(int(offs[-1]), device=device) - offs[:-1][path_of]
    genes = (5 * path_of + 1 + k * (1 + path_of % 337)) % PERIOD
    return genes.int().contiguous(), offs.int().contiguous()


def slab_dO(P: int, R: int, device) -> torch.Tensor:
    """f32 [P, R] integers in -6..6: column r is ((r + 1) p + r) % 13 - 6."""
    p = torch.arange(P, device=device)[:, None]
    r = torch.arange(R, device=device)[None, :]
    return ((((r + 1) * p + r) % SLAB_DO) - 6).float().contiguous()
