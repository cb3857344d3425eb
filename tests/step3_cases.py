"""Fixtures, fp64 / literal references and checks shared by
test_step3_glue_cpu.py (CPU mirror) and test_gpu_step3_glue.py (device) for
the code that strings the step-3 kernels together: graph.build_group_graph,
paths.integrate_pathsets / subset, pipeline.generate_paths and the device
helpers of CbowTrainer (_first_touch_order, _locality_sort, _split).

The references are plain NumPy fp64 or Python sets (literal_port); none of
them calls g2vec_amd.ops.cpu_ref or a function under test. Every check takes
a torch.device.

The threshold band of part A
----------------------------
An f32 implementation cannot decide an edge whose fp64 |PCC| lies closer to
the threshold than its own rounding error, so such an edge may fall either
way; every other edge must agree with the fp64 reference exactly. The band
is the first-order f32 error of PCC = sum_s z_a[s] z_b[s] / S with
z = (x - mean) / std, u = 2^-24 the unit roundoff, in units of 2u = 2^-23:

  S      the S-term dot product of two unit-variance rows, summed in any
         order, is off by at most (S-1) u sum|z_a z_b| <= S u * S (Cauchy-
         Schwarz), i.e. S u after the division by S; each std is the root
         of an S-term f32 accumulation, relative error <= S u / 2, and the
         two of them scale a |PCC| <= 1: another S u.        S u + S u = S
  8      the roundings that do not grow with S: x - mean, the division by
         std (two per row: 4 u on the products), the product itself, the
         division by S, sqrt, and the f32 weight: under 8 u; doubled so
         that the second-order terms are covered.            16 u = 8
  4 r    r = max |mean| / std over the group's non-constant genes. The f32
         mean of values near 16 is off by a few u |mean|, which shifts the
         whole z row by e = (that) / std. To first order the shift cancels
         (sum_s z_b[s] = 0), so this term is an allowance, counted without
         the cancellation: |e_a| mean|z_b| + |e_b| mean|z_a| <= |e_a| +
         |e_b| with a mean error of 4 u |mean| per row.      8 u r = 4 r

  band = (S + 8 + 4 r) * 2^-23

The CPU "edge" mirror is held to this band against fp64 on every fixture
(test_step3_glue_cpu.py); if it leaves the band the derivation is wrong and
has to be redone, not widened.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import literal_port as lp
from g2vec_amd import ops, pipeline
from g2vec_amd.config import G2VecConfig
from g2vec_amd.graph import build_group_graph, dedupe_edges
from g2vec_amd.models.cbow import CbowTrainer
from g2vec_amd.parallel.dist import single
from g2vec_amd.paths import PathSet, integrate_pathsets, subset
from g2vec_amd.pipeline import generate_paths
from g2vec_amd.walks import WalkSet, generate_walks

THR = 0.5
MODES = ("edge", "gemm", "auto")
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


def npy(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


# =====================================================================
# A. per-group graph
# =====================================================================
# (G, S_group0, S_group1): every S of {2,3,5,63,65,288,289} (the auto switch
# sits at 288, the GEMM's K padding at multiples of 4) and every G of
# {1,2,65,130} (one MFMA tile +1, two tiles +2), unequal groups throughout
GRAPH_SHAPES = ((1, 2, 3), (2, 5, 3), (65, 63, 65), (130, 288, 289),
                (130, 2, 65))


def pcc64_matrix(X: np.ndarray, norm_s_minus_1: bool = False):
    """fp64 dense PCC [G,G] of the columns of X [S,G] (population std, 0
    when either std is 0) and the per-gene (mean, std)."""
    X = X.astype(np.float64)
    S = X.shape[0]
    mean, std = X.mean(axis=0), X.std(axis=0)
    ok = std > 0.0
    z = np.where(ok, (X - mean) / np.where(ok, std, 1.0), 0.0)
    C = z.T @ z / ((S - 1) if norm_s_minus_1 else S)
    return C, mean, std


def band_of(S: int, mean: np.ndarray, std: np.ndarray) -> float:
    ok = std > 0.0
    r = float(np.max(np.abs(mean[ok]) / std[ok])) if ok.any() else 0.0
    return (S + 8 + 4.0 * r) * 2.0 ** -23


def ref_adjacency(expr, labels, group, edges, G, thr=THR, ge=False,
                  norm_s_minus_1=False):
    """Dense fp64 adjacency: cell (s,d) = |PCC64| iff it passes the
    threshold, for every listed edge (directed; repeats collapse; a
    self-edge is an edge like any other, as in the literal port)."""
    C, _m, _s = pcc64_matrix(expr[labels == group], norm_s_minus_1)
    A = np.zeros((G, G), dtype=np.float64)
    for s, d in edges:
        w = abs(C[s, d])
        if (w >= thr) if ge else (w > thr):
            A[s, d] = w
    return A


def _unit_rows(rng, S, n):
    """[S,n] columns with mean exactly ~0 and population std 1."""
    z = rng.standard_normal((S, n))
    z -= z.mean(axis=0)
    sd = z.std(axis=0)
    return z / np.where(sd > 0, sd, 1.0)


@functools.lru_cache(maxsize=None)
def graph_fixture(G: int, S0: int, S1: int):
    """dict(expr f32 [S,G], labels i64 [S], edges i32 [E,2], planted,
    special). Log-expression-like values: per-gene mean in [0,16], std in
    [0.7,1.4] inside each group."""
    rng = np.random.default_rng(1000 * G + 10 * S0 + S1)
    S = S0 + S1
    labels = np.zeros(S, dtype=np.int64)
    labels[rng.permutation(S)[:S1]] = 1           # interleaved groups
    rows = [np.flatnonzero(labels == g) for g in (0, 1)]
    expr = np.zeros((S, G), dtype=np.float64)
    mu = rng.uniform(0.0, 16.0, size=G)
    for g in (0, 1):
        sd = rng.uniform(0.7, 1.4, size=G)
        expr[rows[g]] = mu + sd * _unit_rows(rng, len(rows[g]), G)
    # a few correlated modules so that real edges survive the threshold
    for base in range(0, G - 3, 8):
        for g in (0, 1):
            drv = expr[rows[g], base] - mu[base]
            for j in (1, 2):
                expr[rows[g], base + j] = (mu[base + j] + 0.8 * drv + 0.5 *
                                           _unit_rows(rng, len(rows[g]), 1)[:, 0])
    special, planted = {}, []
    edges = []
    if G >= 65:
        c_grp, c_all, p0, p1, n0, n1 = 40, 41, 42, 43, 44, 45
        expr[rows[0], c_grp] = 7.3                # constant in group 0 only
        expr[:, c_all] = 11.3                     # constant everywhere
        expr[:, p1] = 2.0 * expr[:, p0] - 3.0     # perfectly correlated
        expr[:, n1] = 20.0 - expr[:, n0]          # anti-correlated
        special = dict(c_grp=c_grp, c_all=c_all, perfect=(p0, p1),
                       anti=(n0, n1))
        edges += [(c_grp, 0), (0, c_grp), (c_all, 1), (1, c_all),
                  (c_grp, c_all), (p0, p1), (p1, p0), (n0, n1),
                  (3, 3), (c_all, c_all),          # self-edges
                  (5, 6), (5, 6), (5, 6)]          # a repeated file edge
        # planted near-threshold pairs: y = a x + b noise, bisected on b
        pair_cols = [(48 + 2 * k, 49 + 2 * k) for k in range(4)]
        for g in (0, 1):
            Sg = len(rows[g])
            if Sg < 3:
                continue                          # |PCC| is 0 or 1 at S=2
            C, m, s = pcc64_matrix(expr[rows[g]].astype(np.float32))
            band = band_of(Sg, m, s)
            # 3 band (just outside the undecided zone) and 5e-4, each side
            dists = (3 * band, -3 * band, 5e-4, -5e-4)
            for k, (cx, cy) in enumerate(pair_cols):
                a = 1.0 if k % 2 == 0 else -1.0   # both signs of PCC
                x = expr[rows[g], cx]
                n = rng.standard_normal(Sg)
                xc = x - x.mean()
                n -= n.mean()
                n -= xc * (n @ xc) / (xc @ xc)     # PCC monotone in b
                target = THR + dists[(k + 2 * g) % 4]
                lo, hi = 0.0, 1e3

                def pcc_at(b):
                    y = a * x + b * n
                    return abs(np.corrcoef(x, y)[0, 1])
                for _ in range(200):
                    mid = 0.5 * (lo + hi)
                    if pcc_at(mid) > target:
                        lo = mid
                    else:
                        hi = mid
                y = a * x + lo * n
                expr[rows[g], cy] = y - y.mean() + mu[cy]
                planted.append((g, cx, cy))
        edges += [(cx, cy) for cx, cy in pair_cols]
        edges += [(cy, cx) for cx, cy in pair_cols[:2]]
        n_rand = 6 * G
        rnd = rng.integers(0, G, size=(n_rand, 2))
        edges += [(int(a), int(b)) for a, b in rnd]
        for base in range(0, G - 3, 8):
            edges += [(base, base + 1), (base + 1, base), (base, base + 2),
                      (base + 2, base + 1)]
    elif G == 2:
        edges = [(0, 1), (1, 0), (0, 0), (0, 1), (1, 1)]
    else:
        edges = [(0, 0), (0, 0)]
    return dict(G=G, expr=expr.astype(np.float32), labels=labels,
                edges=np.asarray(edges, dtype=np.int32).reshape(-1, 2),
                planted=tuple(planted), special=special)


@functools.lru_cache(maxsize=None)
def graph_reference(G: int, S0: int, S1: int, group: int):
    """dict(A fp64 adjacency, absC, band, undecided mask) from fp64 alone."""
    fx = graph_fixture(G, S0, S1)
    X = fx["expr"][fx["labels"] == group]
    C, m, s = pcc64_matrix(X)
    band = band_of(X.shape[0], m, s)
    listed = np.zeros((G, G), dtype=bool)
    listed[fx["edges"][:, 0], fx["edges"][:, 1]] = True
    absC = np.abs(C)
    A = np.where(listed & (absC > THR), absC, 0.0)
    undecided = listed & (np.abs(absC - THR) <= band)
    return dict(A=A, absC=absC, band=band, listed=listed,
                undecided=undecided, S=X.shape[0], std=s)


def check_reference_conditions(G, S0, S1):
    """What the fixture must offer, asserted from the reference alone."""
    fx = graph_fixture(G, S0, S1)
    for group in (0, 1):
        ref = graph_reference(G, S0, S1, group)
        n_listed = int(ref["listed"].sum())
        assert ref["undecided"].sum() <= 0.01 * n_listed, \
            (G, S0, S1, group, int(ref["undecided"].sum()), n_listed)
        assert 2 * ref["band"] < 1e-3, ref["band"]
        sides = set()
        for (g, cx, cy) in fx["planted"]:
            if g != group:
                continue
            d = ref["absC"][cx, cy] - THR
            assert 2 * ref["band"] <= abs(d) <= 1e-3, (G, group, cx, cy, d,
                                                      ref["band"])
            sides.add(d > 0)
        if G >= 65 and ref["S"] >= 3:
            assert sides == {True, False}
        if fx["special"]:
            sp = fx["special"]
            assert ref["std"][sp["c_all"]] == 0.0
            assert (ref["std"][sp["c_grp"]] == 0.0) == (group == 0)
            assert ref["absC"][sp["perfect"]] > 1 - 1e-9
            assert ref["absC"][sp["anti"]] > 1 - 1e-9
            assert ref["A"][3, 3] > 1 - 1e-9            # self-edge kept
            assert ref["A"][sp["c_all"], sp["c_all"]] == 0.0
        if ref["S"] == 2:
            # two samples: every listed non-constant pair has |PCC| = 1
            ok = ref["std"] > 0
            pair = ref["listed"] & ok[:, None] & ok[None, :]
            assert np.all(np.abs(ref["absC"][pair] - 1.0) < 1e-9)


def csr_to_dense(g, G: int) -> np.ndarray:
    """f32 CSR -> dense f64 (0 = absent), after the CSR-form checks."""
    rp, ci, w = npy(g.row_ptr), npy(g.col_idx), npy(g.weights)
    assert g.row_ptr.dtype == torch.int32 and g.col_idx.dtype == torch.int32
    assert g.weights.dtype == torch.float32
    assert rp.shape == (G + 1,) and rp[0] == 0 and rp[-1] == len(ci) == len(w)
    assert np.all(np.diff(rp) >= 0)
    D = np.zeros((G, G), dtype=np.float64)
    for i in range(G):
        cols = ci[rp[i]:rp[i + 1]]
        assert np.all(np.diff(cols) > 0), f"row {i}: {cols}"   # ascending, no repeats
        assert np.all((cols >= 0) & (cols < G))
        D[i, cols] = w[rp[i]:rp[i + 1]]
    return D


def compare_banded(D: np.ndarray, ref: dict, thr: float = THR, what=""):
    """Implementation's dense adjacency D against the fp64 reference:
    exact structure outside the band, weights within the band."""
    present = D != 0.0
    assert np.all(D[present] > thr), what
    assert not np.any(present & ~ref["listed"]), f"{what}: unlisted edge"
    decided = ref["listed"] & ~ref["undecided"]
    want = ref["A"] > 0.0
    bad = decided & (present != want)
    assert not bad.any(), (f"{what}: {int(bad.sum())} decided edges differ, "
                           f"first {np.argwhere(bad)[:4].tolist()}")
    err = np.abs(D - ref["absC"])[present]
    if err.size:
        assert err.max() <= ref["band"], (what, float(err.max()), ref["band"])


def build(fx, group, mode, device, thr=THR, edges=None):
    e = fx["edges"] if edges is None else edges
    return build_group_graph(torch.from_numpy(fx["expr"]).to(device),
                             torch.from_numpy(fx["labels"]).to(device), group,
                             torch.from_numpy(e).to(device), fx["G"],
                             threshold=thr, mode=mode)


def check_graph_case(G, S0, S1, device):
    fx = graph_fixture(G, S0, S1)
    for group in (0, 1):
        ref = graph_reference(G, S0, S1, group)
        dense = {}
        for mode in MODES:
            g = build(fx, group, mode, device)
            assert g.n_nodes == G and g.row_ptr.device.type == device.type
            dense[mode] = csr_to_dense(g, G)
            compare_banded(dense[mode], ref,
                           what=f"G={G} S={ref['S']} group={group} {mode}")
        decided = ~ref["undecided"]
        for mode in MODES[1:]:                       # mode agreement
            assert np.array_equal((dense[mode] != 0) & decided,
                                  (dense["edge"] != 0) & decided), mode


def check_graph_empty_cases(device):
    fx = graph_fixture(65, 63, 65)
    sp = fx["special"]
    for mode in MODES:
        # an empty edge list
        g = build(fx, 0, mode, device, edges=np.zeros((0, 2), dtype=np.int32))
        assert csr_to_dense(g, 65).sum() == 0 and g.col_idx.numel() == 0
        # lists that the threshold empties: constant genes only (weight 0),
        # and the whole list against a threshold no |PCC| <= 1 passes
        const = np.array([[sp["c_all"], 0], [0, sp["c_all"]],
                          [sp["c_all"], sp["c_all"]]], dtype=np.int32)
        for g in (build(fx, 0, mode, device, edges=const),
                  build(fx, 1, mode, device, thr=1.5)):
            assert csr_to_dense(g, 65).sum() == 0
            assert g.col_idx.numel() == 0 and g.weights.numel() == 0
            assert int(g.row_ptr.abs().sum()) == 0


# exact-arithmetic pair at the threshold: +-1 patterns of 8 samples around an
# integer mean; mean, std = 1 and PCC = 4/8 are exact in fp64
EXACT_X = np.array([1, 1, 1, 1, -1, -1, -1, -1], dtype=np.float64) + 4.0
EXACT_Y = np.array([1, 1, 1, -1, 1, -1, -1, -1], dtype=np.float64) + 9.0


def check_exact_threshold(device):
    """The strict rule at equality. On the exact pair every f32 operand is
    exact (means 4 and 9, std 1, products +-1, 1/S = 0.125), so the weight
    is exactly 0.5 in every mode: absent at thr = 0.5 (`>`, not `>=`),
    present with weight 0.5 just below it."""
    expr = np.stack([EXACT_X, EXACT_Y], axis=1).astype(np.float32)
    C, _m, _s = pcc64_matrix(expr)
    assert C[0, 1] == 0.5
    fx = dict(expr=expr, labels=np.zeros(8, dtype=np.int64), G=2,
              edges=np.array([[0, 1], [1, 0]], dtype=np.int32))
    for mode in MODES:
        g = build(fx, 0, mode, device, thr=0.5)
        assert g.col_idx.numel() == 0, (mode, npy(g.weights))
        assert npy(g.row_ptr).tolist() == [0, 0, 0]
        g = build(fx, 0, mode, device, thr=0.4999999)
        assert npy(g.row_ptr).tolist() == [0, 1, 2], mode
        assert npy(g.col_idx).tolist() == [1, 0], mode
        assert npy(g.weights).tolist() == [0.5, 0.5], (mode, npy(g.weights))


# =====================================================================
# B. path-set integration
# =====================================================================
LEN_PATH = 4
PG = 60                               # genes; 44.. never appear in a walk


def _csr(G, edge_w):
    """CSR tensors from {(src,dst): weight}."""
    rp = np.zeros(G + 1, dtype=np.int64)
    items = sorted(edge_w.items())
    for (s, _d), _w in items:
        rp[s + 1] += 1
    rp = np.cumsum(rp)
    return (torch.from_numpy(rp.astype(np.int32)),
            torch.tensor([d for (_s, d), _w in items], dtype=torch.int32),
            torch.tensor([w for _k, w in items], dtype=torch.float32))


def _hand_graph(group: int):
    """A forward chain 0..19 (the same deterministic walks in both groups,
    one of them exactly LEN_PATH long from every source below 17), two
    cliques 20..27 and 28..36 whose walks visit random 4-subsets in random
    order (repeats inside a group, not adjacent in walk order, and sets
    common to both groups), and 37..40 where the groups differ: good has
    37 -> 38, poor has no edge there (length-1 walks)."""
    rng = np.random.default_rng(50 + group)
    ew = {}
    for i in range(19):
        ew[(i, i + 1)] = 1.0
    for lo, hi in ((20, 28), (28, 37)):
        for a in range(lo, hi):
            for b in range(lo, hi):
                if a != b:
                    ew[(a, b)] = float(rng.integers(1, 5)) / 4.0
    if group == 0:
        ew[(37, 38)] = 1.0
        ew[(39, 40)] = 0.75
    else:
        ew[(40, 39)] = 1.0
    return _csr(PG, ew)


@functools.lru_cache(maxsize=None)
def base_walksets():
    """(good, poor) CPU WalkSets from ops.random_walks on the hand graphs."""
    out = []
    for group in (0, 1):
        rp, ci, w = _hand_graph(group)
        src = torch.arange(0, 44, dtype=torch.int32)
        nodes, lengths, hashes = ops.random_walks(rp, ci, w, src, 6, LEN_PATH,
                                                  1234 + group)
        out.append(WalkSet(nodes, lengths, hashes))
    assert len(out[0].hashes) <= 2000
    return tuple(out)


def permuted(ws: WalkSet, seed: int) -> WalkSet:
    p = torch.from_numpy(np.random.default_rng(seed).permutation(
        ws.nodes.shape[0]))
    return WalkSet(ws.nodes[p].contiguous(), ws.lengths[p].contiguous(),
                   ws.hashes[p].contiguous())


def crafted_hashes(good: WalkSet, poor: WalkSet, seed: int):
    """Replace the hash columns by i64 values with the same equal/unequal
    pattern across BOTH groups: INT64_MIN, INT64_MAX, -1, 0, 1 and random
    values of both signs, assigned in random order."""
    rng = np.random.default_rng(seed)
    allh = np.concatenate([npy(good.hashes), npy(poor.hashes)])
    uniq = np.unique(allh)
    vals = [I64_MIN, I64_MAX, I64_MIN + 1, I64_MAX - 1, -1, 0, 1]
    assert len(uniq) >= len(vals)
    seen = set(vals)
    while len(vals) < len(uniq):
        v = int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64))
        if v not in seen:
            seen.add(v)
            vals.append(v)
    vals = rng.permutation(np.array(vals, dtype=np.int64))
    new = vals[np.searchsorted(uniq, allh)]
    n = len(good.hashes)
    return (WalkSet(good.nodes, good.lengths, torch.from_numpy(new[:n].copy())),
            WalkSet(poor.nodes, poor.lengths, torch.from_numpy(new[n:].copy())))


def _path_sets(ws: WalkSet):
    nodes, lens = npy(ws.nodes), npy(ws.lengths)
    return {tuple(sorted(int(x) for x in nodes[i, :lens[i]]))
            for i in range(len(lens))}


def ref_integrate(good: WalkSet, poor: WalkSet, n_genes: int,
                  last_index: bool = False, tie_value: int = 2):
    """Ordered NumPy reference of integrate_pathsets: per group one
    representative per distinct hash (lowest row index), in ascending signed
    hash order; hashes seen in both groups dropped; good then poor."""
    reps = []
    for ws in (good, poor):
        h = npy(ws.hashes)
        first = {}
        for i, v in enumerate(h.tolist()):
            if last_index or v not in first:
                first[v] = i
        reps.append(first)
    common = set(reps[0]) & set(reps[1])
    genes, offsets, labels = [], [0], []
    cnt = np.zeros((2, n_genes), dtype=np.int64)
    for label, (ws, first) in enumerate(zip((good, poor), reps)):
        nodes, lens = npy(ws.nodes), npy(ws.lengths)
        for v in sorted(k for k in first if k not in common):
            i = first[v]
            row = nodes[i, :lens[i]]
            genes += row.tolist()
            offsets.append(offsets[-1] + int(lens[i]))
            labels.append(float(label))
            cnt[label, row] += 1
    freq = np.full(n_genes, 2, dtype=np.int64)
    freq[cnt[0] > cnt[1]] = 0
    freq[cnt[1] > cnt[0]] = 1
    freq[(cnt[0] == cnt[1]) & (cnt[0] > 0)] = tie_value
    return dict(genes=np.asarray(genes, dtype=np.int32),
                offsets=np.asarray(offsets, dtype=np.int32),
                labels=np.asarray(labels, dtype=np.float32), freq=freq,
                n_in_paths=int(((cnt[0] + cnt[1]) > 0).sum()), cnt=cnt)


def to_dev(ws: WalkSet, device) -> WalkSet:
    return WalkSet(ws.nodes.to(device), ws.lengths.to(device),
                   ws.hashes.to(device))


def check_integrate(good: WalkSet, poor: WalkSet, device, n_genes: int = PG):
    """integrate_pathsets on `device` against the literal port (as sets),
    the ordered NumPy reference and the CPU call (both bitwise)."""
    ps, freq, n_in = integrate_pathsets(to_dev(good, device),
                                        to_dev(poor, device), n_genes)
    assert ps.genes.device.type == device.type
    assert (ps.genes.dtype, ps.offsets.dtype, ps.labels.dtype, freq.dtype) == \
        (torch.int32, torch.int32, torch.float32, torch.int64)
    g, o, l, f = npy(ps.genes), npy(ps.offsets), npy(ps.labels), npy(freq)
    assert o[0] == 0 and o[-1] == len(g) and len(o) == len(l) + 1
    assert ps.n_genes == n_genes and f.shape == (n_genes,)
    got = []
    for p in range(len(l)):
        path = g[o[p]:o[p + 1]].tolist()
        assert len(path) >= 1 and len(set(path)) == len(path), path
        got.append((frozenset(path), int(l[p])))
    assert len(set(got)) == len(got)
    # literal port: sets with labels, frequencies, gene count. (With crafted
    # hashes equality of hashes still means equality of sets.)
    rows = lp.lp_integrate(_path_sets(good), _path_sets(poor), n_genes)
    want = {(frozenset(np.flatnonzero(r[:-1]).tolist()), int(r[-1]))
            for r in rows}
    assert set(got) == want and len(got) == rows.shape[0]
    names = [str(i) for i in range(n_genes)]
    gf = lp.lp_gene_freq(rows, names)
    want_f = np.array([gf.get(nm, 2) for nm in names], dtype=np.int64)
    assert np.array_equal(f, want_f)
    assert n_in == len(gf)
    # ordered reference: the representative rule fixes order and content
    ref = ref_integrate(good, poor, n_genes)
    assert np.array_equal(g, ref["genes"])
    assert np.array_equal(o, ref["offsets"])
    assert np.array_equal(l, ref["labels"])
    assert np.array_equal(f, ref["freq"]) and n_in == ref["n_in_paths"]
    # the CPU call on the same WalkSet
    cps, cfreq, cn = integrate_pathsets(good, poor, n_genes)
    assert torch.equal(ps.genes.cpu(), cps.genes)
    assert torch.equal(ps.offsets.cpu(), cps.offsets)
    assert torch.equal(ps.labels.cpu(), cps.labels)
    assert torch.equal(freq.cpu(), cfreq) and n_in == cn
    return ps, ref


def check_base_conditions():
    """What the hand-made walk sets must contain, from the reference alone."""
    good, poor = base_walksets()
    for ws in (good, poor):
        nodes, lens, h = npy(ws.nodes), npy(ws.lengths), npy(ws.hashes)
        assert (lens == 1).any() and (lens == LEN_PATH).any()
        assert np.all(nodes[lens == LEN_PATH] >= 0)        # no -1 padding
        # a repeat whose copies are not adjacent rows
        _u, inv, cnt = np.unique(h, return_inverse=True, return_counts=True)
        far = False
        for k in np.flatnonzero(cnt > 1):
            idx = np.flatnonzero(inv == k)
            far |= bool(np.any(np.diff(idx) > 1))
        assert far
        # equal sets walked in different orders (the representative matters)
        diff_order = False
        for k in np.flatnonzero(cnt > 1):
            idx = np.flatnonzero(inv == k)
            diff_order |= any(not np.array_equal(nodes[idx[0]], nodes[j])
                              for j in idx[1:])
        assert diff_order
    assert set(npy(good.hashes).tolist()) & set(npy(poor.hashes).tolist())
    ref = ref_integrate(good, poor, PG)
    assert len(ref["labels"]) > 20 and 0 < ref["labels"].sum() < len(ref["labels"])
    c = ref["cnt"]
    assert ((c[0] == c[1]) & (c[0] > 0)).any(), "no tied gene in the paths"
    assert ((c[0] + c[1]) == 0).any(), "no absent gene"
    assert (ref["freq"] == 0).any() and (ref["freq"] == 1).any()


def empty_walkset(L: int = LEN_PATH) -> WalkSet:
    return WalkSet(torch.zeros((0, L), dtype=torch.int32),
                   torch.zeros(0, dtype=torch.int32),
                   torch.zeros(0, dtype=torch.int64))


def check_integrate_edges(device):
    good, poor = base_walksets()
    # P = 0: every path common to both groups
    ps, freq, n_in = integrate_pathsets(to_dev(good, device),
                                        to_dev(permuted(good, 3), device), PG)
    assert ps.genes.numel() == 0 and ps.labels.numel() == 0
    assert npy(ps.offsets).tolist() == [0] and n_in == 0
    assert (ps.genes.dtype, ps.offsets.dtype, ps.labels.dtype, freq.dtype) == \
        (torch.int32, torch.int32, torch.float32, torch.int64)
    assert np.array_equal(npy(freq), np.full(PG, 2))
    # one group with zero walks, either side
    check_integrate(good, empty_walkset(), device)
    check_integrate(empty_walkset(), poor, device)
    # walks of length 1 only (single-gene sets; 0..9 vs 5..14: 5..9 common)
    def singles(lo, hi):
        n = hi - lo
        nodes = torch.full((n, LEN_PATH), -1, dtype=torch.int32)
        nodes[:, 0] = torch.arange(lo, hi, dtype=torch.int32)
        return WalkSet(nodes, torch.ones(n, dtype=torch.int32),
                       torch.arange(lo, hi, dtype=torch.int64) * 7919 - 40000)
    check_integrate(singles(0, 10), singles(5, 15), device)
    # a len_path mismatch between the groups
    wide = WalkSet(torch.cat([poor.nodes, torch.full_like(poor.nodes[:, :1], -1)],
                             dim=1).contiguous(), poor.lengths, poor.hashes)
    try:
        integrate_pathsets(to_dev(good, device), to_dev(wide, device), PG)
    except ValueError:
        pass
    else:
        raise AssertionError("len_path mismatch did not raise ValueError")


def ref_subset(g, o, l, idx):
    genes, offs = [], [0]
    for i in idx:
        genes += g[o[i]:o[i + 1]].tolist()
        offs.append(len(genes))
    return (np.asarray(genes, dtype=np.int32), np.asarray(offs, dtype=np.int32),
            l[np.asarray(idx, dtype=np.int64)] if len(idx) else l[:0])


def base_pathset(device) -> PathSet:
    good, poor = base_walksets()
    ps, _f, _n = integrate_pathsets(good, poor, PG)
    return PathSet(ps.genes.to(device), ps.offsets.to(device),
                   ps.labels.to(device), PG)


def check_subset(device):
    ps = base_pathset(device)
    g, o, l = npy(ps.genes), npy(ps.offsets), npy(ps.labels)
    P = ps.n_paths
    for idx in ([], list(range(P))[::-1], [3, 3, 0, P - 1, 3, 0], [P // 2]):
        sub = subset(ps, torch.tensor(idx, dtype=torch.int64, device=device))
        rg, ro, rl = ref_subset(g, o, l, idx)
        assert sub.genes.dtype == torch.int32 and sub.offsets.dtype == torch.int32
        assert np.array_equal(npy(sub.genes), rg), idx
        assert np.array_equal(npy(sub.offsets), ro), idx
        assert np.array_equal(npy(sub.labels), rl), idx
        assert sub.n_genes == PG and sub.genes.device.type == device.type


def check_trainer_helpers(device):
    """_first_touch_order (+ o2n), _locality_sort and _split on `device`
    against NumPy definitions and bitwise against the CPU result."""
    quiet = lambda *a, **k: None   # noqa: E731
    seed = 4
    cfg = G2VecConfig(hidden=64, epochs=1, early_stop=False, seed=seed,
                      device=device.type, gene_relabel="on")
    ps = base_pathset(device)
    g, o, l = npy(ps.genes), npy(ps.offsets), npy(ps.labels)
    P = ps.n_paths
    tr = CbowTrainer(cfg, PG, device, log=quiet)
    tr.setup(ps)
    order, o2n = npy(tr.gene_order), npy(tr.gene_o2n)
    first = np.full(PG, np.iinfo(np.int64).max)
    for pos in range(len(g) - 1, -1, -1):
        first[g[pos]] = pos                      # first position wins
    touched = np.flatnonzero(first < np.iinfo(np.int64).max)
    want = np.concatenate([touched[np.argsort(first[touched], kind="stable")],
                           np.setdiff1d(np.arange(PG), touched)])
    assert len(touched) < PG
    assert tr.gene_order.dtype == torch.int64
    assert np.array_equal(npy(tr._first_touch_order(ps)), want)
    assert np.array_equal(order, want)
    assert np.array_equal(o2n[want], np.arange(PG))       # the inverse
    # _locality_sort: stable by first gene
    ls = CbowTrainer._locality_sort(ps)
    idx = np.argsort(g[o[:-1]], kind="stable")
    rg, ro, rl = ref_subset(g, o, l, idx.tolist())
    assert np.array_equal(npy(ls.genes), rg)
    assert np.array_equal(npy(ls.offsets), ro)
    assert np.array_equal(npy(ls.labels), rl)
    # _split: torch.randperm seeded seed + 12345, pivot int(0.8 P)
    gen = torch.Generator()
    gen.manual_seed(seed + 12345)
    perm = torch.randperm(P, generator=gen).numpy()
    pivot = int(0.8 * P)
    a, b = tr._split(ps)
    for got, idx in ((a, perm[:pivot]), (b, perm[pivot:])):
        rg, ro, rl = ref_subset(g, o, l, idx.tolist())
        assert np.array_equal(npy(got.genes), rg)
        assert np.array_equal(npy(got.offsets), ro)
        assert np.array_equal(npy(got.labels), rl)
    assert (tr.n_tr_global, tr.n_vl_global) == (pivot, P - pivot)
    if device.type != "cpu":
        cpu = torch.device("cpu")
        cps = base_pathset(cpu)
        ctr = CbowTrainer(dataclasses.replace(cfg, device="cpu"), PG, cpu,
                          log=quiet)
        ctr.setup(cps)
        assert torch.equal(tr.gene_order.cpu(), ctr.gene_order)
        assert torch.equal(tr.gene_o2n.cpu(), ctr.gene_o2n)
        ca, cb = ctr._split(cps)
        cl = CbowTrainer._locality_sort(cps)
        for dv, cv in ((a, ca), (b, cb), (ls, cl)):
            assert torch.equal(dv.genes.cpu(), cv.genes)
            assert torch.equal(dv.offsets.cpu(), cv.offsets)
            assert torch.equal(dv.labels.cpu(), cv.labels)


# =====================================================================
# C. generate_paths: the two-stream overlap changes nothing
# =====================================================================
def load_study(files: dict, device):
    """(expr_t, labels_t, edge_idx_t, n_genes) as pipeline.run loads and
    preprocesses a file triple."""
    st = pipeline.load_study(
        G2VecConfig(expression_file=files["expression"],
                    clinical_file=files["clinical"],
                    network_file=files["network"], device=str(device)),
        log=lambda *a, **k: None)
    return st.expr_t, st.labels_t, st.edge_idx_t, st.n_genes


def check_generate_paths(files: dict, device, pcc_mode: str):
    expr, labels, edges, n_genes = load_study(files, device)
    cfg = G2VecConfig(len_path=20, num_repetition=2, seed=0,
                      device=device.type, pcc_mode=pcc_mode)
    quiet = lambda *a, **k: None   # noqa: E731
    ctx = single(device)
    first = generate_paths(cfg, expr, labels, edges, n_genes, ctx, quiet)
    # the same chain, issued by the test on the current stream
    ded = dedupe_edges(edges, n_genes)
    graphs, walks = [], []
    for group in (0, 1):
        g = build_group_graph(expr, labels, group, ded, n_genes,
                              threshold=cfg.pcc_threshold, mode=pcc_mode,
                              edges_deduped=True)
        graphs.append(g)
        walks.append(generate_walks(g, cfg.len_path, cfg.num_repetition,
                                    cfg.seed, group, (0, n_genes)))
    ps, freq, n_in = integrate_pathsets(walks[0], walks[1], n_genes)
    second = generate_paths(cfg, expr, labels, edges, n_genes, ctx, quiet)
    assert ps.n_paths > 50 and n_in > 10
    for (gps, gfreq, gn, stats) in (first, second):
        assert torch.equal(gps.genes, ps.genes)
        assert torch.equal(gps.offsets, ps.offsets)
        assert torch.equal(gps.labels, ps.labels)
        assert torch.equal(gfreq, freq) and gn == n_in
        assert stats["nnz_g0"] == int(graphs[0].col_idx.numel())
        assert stats["nnz_g1"] == int(graphs[1].col_idx.numel())
        assert stats["n_walks"] == 2 * 2 * n_genes
        assert gps.genes.device.type == device.type
