"""Fixtures and checks shared by the CPU and GPU tests of the rank statistics
(ops.rank_columns / ranksum_scores, scoring.ranksum_scores, the Spearman
graph and the rank-based permutation null).

The reference here is independent of cpu_ref and of scoring: ranks by direct
pair counting in int64 (less and equal per element, IEEE compares), the two
integer sums 2*W1 and 4*SSR from them, and z / auc from the textbook formula
in fp64.

Every check takes a torch device, so test_rank_cpu.py holds the CPU mirror
and test_gpu_rank.py the HIP kernels to the same assertions.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from g2vec_amd import ops, scoring
from steps56_cases import ulp_diff_f32

TG, SJ = ops.RANK_TG, ops.RANK_SJ
PASS = ops.RANK_IB * ops.RANK_WAVES          # samples per i-pass of a block
CAP_G = ops.RANK_MAX_BLOCKS * TG + 1         # one gene past the grid cap


# ------------------------------------------------------------- reference
def ref_rank2(x: np.ndarray) -> np.ndarray:
    """int64 [S, G]: R2 = 2*less + equal + 1 by direct counting, self
    included in equal."""
    x = np.asarray(x, dtype=np.float32)
    S, G = x.shape
    out = np.empty((S, G), dtype=np.int64)
    step = max(1, (1 << 24) // (S * S))
    for lo in range(0, G, step):
        c = x[:, lo:lo + step]
        less = (c[None, :, :] < c[:, None, :]).sum(axis=1, dtype=np.int64)
        equal = (c[None, :, :] == c[:, None, :]).sum(axis=1, dtype=np.int64)
        out[:, lo:lo + step] = 2 * less + equal + 1
    return out


def ref_ranks(x: np.ndarray) -> np.ndarray:
    """f32 ranks = R2 / 2: half-integers <= S, exact."""
    return (ref_rank2(x).astype(np.float64) / 2.0).astype(np.float32)


def ref_ranksum(x: np.ndarray, labels: np.ndarray):
    """(w2, q4, z, auc): int64 2*W1 and 4*SSR, fp64 |z| and auc."""
    r2 = ref_rank2(x)
    S = x.shape[0]
    m = (np.asarray(labels) == 1)
    n1 = int(m.sum())
    n0 = S - n1
    w2 = r2[m].sum(axis=0, dtype=np.int64)
    q4 = ((r2 - (S + 1)) ** 2).sum(axis=0, dtype=np.int64)
    G = x.shape[1]
    z = np.zeros(G)
    auc = np.full(G, 0.5)
    if n1 >= 2 and n0 >= 2:
        live = q4 > 0
        W1 = w2[live] / 2.0
        SSR = q4[live] / 4.0
        z[live] = np.abs(W1 - n1 * (S + 1) / 2.0) / np.sqrt(
            n1 * n0 / (S * (S - 1.0)) * SSR)
        auc[live] = (W1 - n1 * (n1 + 1) / 2.0) / (n1 * n0)
    return w2, q4, z, auc


# -------------------------------------------------------------- fixtures
PATTERNS = ("distinct", "ties", "constant", "two_valued", "ascending",
            "descending", "signed_zero", "inf", "subnormal")


def _pattern(rng, name: str, S: int, n: int) -> np.ndarray:
    if name == "distinct":
        # a random permutation per column scaled off the integers
        return (np.argsort(rng.random((S, n)), axis=0) * 0.37 - 5.0)
    if name == "ties":
        return rng.integers(0, 4, size=(S, n)).astype(np.float64)
    if name == "constant":
        return np.full((S, n), 3.25)
    if name == "two_valued":
        return rng.choice([-1.5, 2.0], size=(S, n))
    if name == "ascending":
        return np.repeat(np.arange(S, dtype=np.float64)[:, None], n, axis=1)
    if name == "descending":
        return np.repeat(-np.arange(S, dtype=np.float64)[:, None], n, axis=1)
    if name == "signed_zero":
        return rng.choice([-0.0, 0.0, 1.0, -1.0], size=(S, n))
    if name == "inf":
        return rng.choice([-np.inf, np.inf, 0.5, -2.0, 7.0], size=(S, n))
    assert name == "subnormal"
    tiny = float(np.float32(1.4e-45))
    return rng.integers(-3, 4, size=(S, n)) * tiny


S_VALUES = (1, 2, 3, PASS - 1, PASS, PASS + 1, 63, 64, 65, 135, SJ - 1, SJ,
            SJ + 1, 2 * SJ + 1)
G_VALUES = (1, TG - 1, TG, TG + 1, 130, 1003)
# every single-axis edge against a fixed value of the other axis: the S axis
# rides on G = TG + 1 (a second gene tile with one live column), the G axis
# on S = SJ + 1 (a second j-tile with one live sample); then the corners and
# the ragged second sweep past the grid cap
SHAPES = tuple(dict.fromkeys(
    [(S, TG + 1) for S in S_VALUES]
    + [(SJ + 1, G) for G in G_VALUES]
    + [(1, 1), (135, 130), (2 * SJ + 1, 130), (3, CAP_G)]))
CASES = tuple((S, G, bal) for (S, G) in SHAPES for bal in (False, True))


@functools.lru_cache(maxsize=None)
def values(S: int, G: int) -> np.ndarray:
    """expr f32 [S, G]; column c holds pattern (c + S) mod 9."""
    rng = np.random.default_rng(5000 + 100 * S + G)
    x = np.empty((S, G), dtype=np.float32)
    pat = (np.arange(G) + S) % len(PATTERNS)
    for k, name in enumerate(PATTERNS):
        cols = np.flatnonzero(pat == k)
        if cols.size:
            x[:, cols] = _pattern(rng, name, S, cols.size).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ranks_of(S: int, G: int) -> np.ndarray:
    r = ref_ranks(values(S, G))
    r.setflags(write=False)
    return r


def labels_of(S: int, balanced: bool) -> np.ndarray:
    """2 good vs the rest, or balanced; fixed positions from a seeded draw."""
    rng = np.random.default_rng(600 + S + int(balanced))
    n0 = S // 2 if balanced else min(2, S)
    lab = np.ones(S, dtype=np.int64)
    lab[rng.choice(S, size=n0, replace=False)] = 0
    return lab


@functools.lru_cache(maxsize=None)
def ranksum_case(S: int, G: int, balanced: bool):
    x = values(S, G)
    lab = labels_of(S, balanced)
    w2, q4, z, auc = ref_ranksum(x, lab)
    return dict(expr=x, labels=lab, w2=w2, q4=q4, z=z, auc=auc)


def tensor(a: np.ndarray, device="cpu") -> torch.Tensor:
    """A private copy of a (shared, read-only) fixture array on device."""
    return torch.from_numpy(np.array(a)).to(device)


def tied_integers(S: int, G: int, seed: int = 1) -> np.ndarray:
    rng = np.random.default_rng(seed)
    return rng.integers(0, 6, size=(S, G)).astype(np.float32)


# ---------------------------------------------------------------- checks
def check_ranks(S: int, G: int, device) -> None:
    x = tensor(values(S, G), device)
    r = ops.rank_columns(x)
    assert r.dtype == torch.float32 and r.shape == (S, G)
    assert r.device.type == torch.device(device).type
    got = r.cpu().numpy()
    assert got.tobytes() == ranks_of(S, G).tobytes()
    # the sum of a column's average ranks is S (S + 1) / 2
    assert np.array_equal(got.astype(np.float64).sum(axis=0),
                          np.full(G, S * (S + 1) / 2.0))


def check_ranksum(S: int, G: int, balanced: bool, device) -> None:
    case = ranksum_case(S, G, balanced)
    x = tensor(case["expr"], device)
    lab = tensor(case["labels"], device)
    z, auc = ops.ranksum_scores(x, lab)
    assert z.dtype == torch.float32 and auc.dtype == torch.float32
    assert z.shape == (G,) and auc.shape == (G,)
    z, auc = z.cpu().numpy(), auc.cpu().numpy()
    zh, ah = scoring.ranksum_scores(case["expr"], case["labels"])
    dz, da = ulp_diff_f32(z, zh), ulp_diff_f32(auc, ah)
    print("ulp z", dz, "ulp auc", da)
    assert dz <= 1 and da <= 1
    # and the host function against the counting reference, same bound
    assert ulp_diff_f32(zh, case["z"].astype(np.float32)) <= 1
    assert ulp_diff_f32(ah, case["auc"].astype(np.float32)) <= 1
    # constant columns: z = 0, auc = 0.5
    const = (case["expr"] == case["expr"][0]).all(axis=0)
    assert const.any() or G < len(PATTERNS)
    assert (z[const] == 0.0).all() and (auc[const] == 0.5).all()
    n1 = int(case["labels"].sum())
    if n1 < 2 or S - n1 < 2:
        assert (z == 0.0).all() and (auc == 0.5).all()
    # labels other than 0/1 are dropped before the ranking
    if S >= 5:
        lab2 = case["labels"].copy()
        lab2[[0, S // 2]] = (2, -1)
        keep = (lab2 == 0) | (lab2 == 1)
        z2, a2 = ops.ranksum_scores(x, torch.from_numpy(lab2).to(device))
        z3, a3 = ops.ranksum_scores(
            x[torch.from_numpy(keep).to(device)].contiguous(),
            torch.from_numpy(lab2[keep]).to(device))
        assert torch.equal(z2, z3) and torch.equal(a2, a3)


def check_repeatable(device) -> None:
    """Integer sums: z and auc are the same bits run to run."""
    x = torch.from_numpy(tied_integers(SJ + 7, 2 * TG + 3)).to(device)
    lab = torch.from_numpy(labels_of(SJ + 7, True)).to(device)
    z1, a1 = ops.ranksum_scores(x, lab)
    z2, a2 = ops.ranksum_scores(x, lab)
    assert torch.equal(z1, z2) and torch.equal(a1, a2)
    assert float(z1.max()) > 0.0


# --------------------------------------------------------------- spearman
def graph_inputs(S: int = 41, G: int = 70, seed: int = 3):
    """Dyadic expression (multiples of 1/8 in [-4, 4]) with correlated
    column blocks, balanced labels and a random directed edge list."""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(S, 7))
    x = base[:, rng.integers(0, 7, size=G)] + 0.6 * rng.normal(size=(S, G))
    x = np.clip(np.round(x * 8.0) / 8.0, -4.0, 4.0).astype(np.float32)
    labels = labels_of(S, True)
    edges = rng.integers(0, G, size=(900, 2)).astype(np.int64)
    edges = edges[edges[:, 0] != edges[:, 1]]
    return x, labels, edges


def build(x, labels, edges, group, device, corr, mode="edge"):
    from g2vec_amd.graph import build_group_graph
    return build_group_graph(torch.from_numpy(np.ascontiguousarray(x)).to(device),
                             torch.from_numpy(labels).to(device), group,
                             torch.from_numpy(edges).to(device), x.shape[1],
                             mode=mode, corr=corr)


def same_graph(a, b) -> bool:
    return (torch.equal(a.row_ptr, b.row_ptr)
            and torch.equal(a.col_idx, b.col_idx)
            and a.weights.cpu().numpy().tobytes()
            == b.weights.cpu().numpy().tobytes())


def preranked(x: np.ndarray, labels: np.ndarray, group: int) -> np.ndarray:
    """x with the group's rows replaced by their within-group reference
    ranks."""
    out = x.copy()
    rows = labels == group
    out[rows] = ref_ranks(x[rows])
    return out


def check_spearman_is_pearson_of_ranks(device, mode: str) -> None:
    x, labels, edges = graph_inputs()
    for group in (0, 1):
        sp = build(x, labels, edges, group, device, "spearman", mode)
        pe = build(preranked(x, labels, group), labels, edges, group, device,
                   "pearson", mode)
        assert sp.col_idx.numel() > 0
        assert same_graph(sp, pe)


# ----------------------------------------------------------- permutations
PERM_S, PERM_G, PERM_B = 135, 40, 200


@functools.lru_cache(maxsize=None)
def perm_case():
    """Tied integer data at S = 135 and the exact integer exceed counts of
    the rank sum over the relabellings of scoring.perm_masks."""
    S, G, B = PERM_S, PERM_G, PERM_B
    assert S ** 3 <= 2 ** 24      # every f32 sum of the centred ranks is exact
    x = tied_integers(S, G, seed=9)
    x[:, 0] = 2.0                 # constant gene: every relabelling exceeds
    rng = np.random.default_rng(12)
    labels = np.zeros(S, dtype=np.int64)
    labels[rng.choice(S, size=52, replace=False)] = 1
    n1 = int(labels.sum())
    r2 = ref_rank2(x)
    masks = scoring.perm_masks(labels, B, seed=21).astype(np.int64)
    dev_obs = np.abs((r2 * labels[:, None]).sum(axis=0) - n1 * (S + 1))
    dev_b = np.abs(masks @ r2 - n1 * (S + 1))           # [B, G]
    counts = (dev_b >= dev_obs[None, :]).sum(axis=0)
    return dict(expr=x, labels=labels, counts=counts)


def check_perm_counts(device) -> None:
    case = perm_case()
    ranks = ops.rank_columns(torch.from_numpy(case["expr"]).to(device))
    r = scoring.permutation_pvalues(ranks.cpu().numpy(), case["labels"],
                                    PERM_B, seed=21, device=device)
    assert np.array_equal(r["counts"], case["counts"])
    assert r["counts"][0] == PERM_B


# --------------------------------------------------------------- pipeline
RANK_COLS = ["GeneSymbol", "Lgroup", "d_score", "z_ranksum", "auc",
             "gene_score", "biomarker"]
PERM_COLS = ["p_perm", "q_bh", "p_maxT"]


def pipeline_cfg(tiny_files, tmp_path, device, name, **kw):
    from g2vec_amd.config import G2VecConfig
    base = dict(expression_file=tiny_files["expression"],
                clinical_file=tiny_files["clinical"],
                network_file=tiny_files["network"],
                result_name=str(tmp_path / name), len_path=15,
                num_repetition=3, epochs=25, device=device, seed=0)
    base.update(kw)
    return G2VecConfig(**base)


def check_rank_pipeline(tiny_files, tmp_path, device, **extra):
    """--corr spearman --score-stat ranksum --permutations 64: the table's
    columns, two byte-identical runs, biomarker column against the file."""
    from g2vec_amd.pipeline import run
    kw = dict(corr="spearman", score_stat="ranksum", permutations=64,
              write_scores=True, **extra)
    res = run(pipeline_cfg(tiny_files, tmp_path, device, "a", **kw))
    run(pipeline_cfg(tiny_files, tmp_path, device, "b", **kw))
    rows = [ln.split("\t") for ln in
            (tmp_path / "a_scores.txt").read_text().splitlines()]
    assert rows[0] == RANK_COLS + PERM_COLS
    body = rows[1:]
    assert len(body) == res["n_genes"]
    assert all(len(r) == len(rows[0]) for r in body)
    bio = (tmp_path / "a_biomarkers.txt").read_text().splitlines()[1:]
    assert sorted(r[0] for r in body if r[6] == "1") == bio
    for r in body:
        assert float(r[3]) >= 0.0 and 0.0 <= float(r[4]) <= 1.0
        assert 1.0 / 65 * (1 - 1e-5) <= float(r[7]) <= 1.0
    for suffix in ("_scores.txt", "_biomarkers.txt", "_lgroups.txt",
                   "_vectors.txt"):
        assert (tmp_path / ("a" + suffix)).read_bytes() == \
            (tmp_path / ("b" + suffix)).read_bytes(), suffix
    return bio
