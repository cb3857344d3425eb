"""Fixtures and checks shared by the CPU and GPU tests of the permutation
null of the gene t-scores (ops.col_moments / perm_t_stats / perm_t_counts,
scoring.perm_masks / permutation_pvalues).

The reference here is independent of cpu_ref: two-pass fp64 group means and
squared deviations per mask row, then t^2 — not the sums formula the kernel
and its mirror use. Exceedance follows the contract's tie rule,
stat_perm >= stat_obs * (1 - 2^-30).

Every check takes a torch device, so test_perm_cpu.py holds the CPU mirror
and test_gpu_perm.py the HIP kernels to the same assertions.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from g2vec_amd import scoring
from steps56_cases import ulp_diff_f32

TIE = 1.0 - 2.0 ** -30
REL = 1e-12                      # stat / maxstat against the fp64 reference


# ------------------------------------------------------------- reference
def ref_stats(expr: np.ndarray, masks: np.ndarray) -> np.ndarray:
    """t^2 f64 [B, G], two-pass: group means, then squared deviations."""
    x = expr.astype(np.float64)
    S = x.shape[0]
    out = np.zeros((masks.shape[0], x.shape[1]), dtype=np.float64)
    for b, m in enumerate(masks.astype(bool)):
        a, c = x[m], x[~m]                       # poor (1), good (0)
        n1, n0 = a.shape[0], c.shape[0]
        m1, m0 = a.mean(axis=0), c.mean(axis=0)
        ss = ((a - m1) ** 2).sum(axis=0) + ((c - m0) ** 2).sum(axis=0)
        pooled = ss / (S - 2.0)
        d = m0 - m1
        pos = pooled > 0.0
        out[b] = np.where(pos, d * d / np.where(pos, pooled, 1.0)
                          / (1.0 / n1 + 1.0 / n0), 0.0)
    return out


def ref_counts(stat: np.ndarray, stat_obs: np.ndarray) -> np.ndarray:
    return (stat >= stat_obs[None, :] * TIE).sum(axis=0)


def random_masks(rng, S: int, n1: int, B: int) -> np.ndarray:
    m = np.zeros((B, S), dtype=np.uint8)
    for b in range(B):
        m[b, rng.choice(S, size=n1, replace=False)] = 1
    return m


# ---------------------------------------------------------- exact fixtures
EXACT_S = (4, 5, 63, 64, 65, 135, 300)
EXACT_G = (1, 63, 64, 65, 130)
EXACT_B = (1, 15, 16, 17, 64, 65, 200)
# every single-axis edge against a fixed pair of the other two (the S axis
# rides on G = 65, B = 65: a second tile with one live row and one live
# column), plus the all-maxima case
EXACT_SHAPES = tuple(dict.fromkeys(
    [(S, 65, 65) for S in EXACT_S]
    + [(65, G, 17) for G in EXACT_G]
    + [(63, 63, B) for B in EXACT_B]
    + [(300, 130, 200), (5, 1, 1)]))
EXACT_CASES = tuple((S, G, B, bal) for (S, G, B) in EXACT_SHAPES
                    for bal in (False, True))


@functools.lru_cache(maxsize=None)
def exact_case(S: int, G: int, B: int, balanced: bool):
    """Integer expr f32 [S, G] in [-8, 8] (sums <= 64*S: exact in f32 in any
    order); column 0 constant, column 1 constant inside each observed group.
    Labels: 2 good vs the rest, or balanced. Mask row 0 is the observed
    labelling and, when the groups are equal in size, row 1 its mirror: both
    tie with the observed statistic in exact arithmetic.
    Returns dict(expr, labels, masks, stat, stat_obs, counts, maxstat)."""
    rng = np.random.default_rng(7000 + 1000 * S + 10 * G + B + int(balanced))
    expr = rng.integers(-8, 9, size=(S, G)).astype(np.float32)
    n0 = S // 2 if balanced else 2
    labels = np.ones(S, dtype=np.int64)
    labels[rng.choice(S, size=n0, replace=False)] = 0
    expr[:, 0] = 3.0
    if G > 1:
        expr[:, 1] = np.where(labels == 0, 2.0, -5.0)
    n1 = S - n0
    masks = random_masks(rng, S, n1, B)
    masks[0] = (labels == 1)
    if B > 1 and n1 == n0:
        masks[1] = (labels == 0)
    obs = (labels == 1).astype(np.uint8)[None, :]
    stat = ref_stats(expr, masks)
    stat_obs = ref_stats(expr, obs)[0]
    # precondition of the exact comparison: a relabelling either ties with
    # the observed statistic or is clearly apart from it
    live = stat_obs > 0.0
    rel = np.abs(stat[:, live] - stat_obs[live]) / stat_obs[live]
    assert not ((rel > 1e-12) & (rel < 1e-6)).any(), (S, G, B, balanced)
    return dict(expr=expr, labels=labels, masks=masks, stat=stat,
                stat_obs=stat_obs, counts=ref_counts(stat, stat_obs),
                maxstat=stat.max(axis=1))


def assert_rel(got: np.ndarray, ref: np.ndarray, rel: float = REL):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref)
    worst = float((err / np.where(ref != 0, np.abs(ref), 1.0)).max()) \
        if ref.size else 0.0
    print("max rel err", worst)
    assert (err <= rel * np.abs(ref)).all(), worst


def check_exact(ops, case, device):
    """The contract of the exact fixtures, on `device`."""
    dev = torch.device(device)
    expr = torch.from_numpy(case["expr"]).to(dev)
    masks = torch.from_numpy(case["masks"]).to(dev)
    obs = torch.from_numpy(
        (case["labels"] == 1).astype(np.uint8)[None, :]).to(dev)
    stat_obs = ops.perm_t_stats(expr, obs)
    assert stat_obs.dtype == torch.float64
    assert stat_obs.shape == (1, expr.shape[1])
    assert_rel(stat_obs[0].cpu().numpy(), case["stat_obs"])
    stat = ops.perm_t_stats(expr, masks)
    assert_rel(stat.cpu().numpy(), case["stat"])
    # the observed labelling as a mask row: identical bits
    assert torch.equal(stat[0], stat_obs[0])
    counts, maxstat = ops.perm_t_counts(expr, masks,
                                        stat_obs[0].contiguous())
    assert counts.dtype == torch.int32 and maxstat.dtype == torch.float64
    assert np.array_equal(counts.cpu().numpy(), case["counts"])
    assert_rel(maxstat.cpu().numpy(), case["maxstat"])
    # constant gene, and gene constant inside both observed groups: t = 0,
    # every relabelling exceeds
    B = masks.shape[0]
    assert float(stat_obs[0, 0]) == 0.0 and int(counts[0]) == B
    if expr.shape[1] > 1:
        assert float(stat_obs[0, 1]) == 0.0 and int(counts[1]) == B
    # |t| against the host t-scores
    t32 = stat_obs[0].sqrt().float().cpu().numpy()
    host = scoring.t_scores(case["expr"], case["labels"])
    assert ulp_diff_f32(t32, host) <= 1
    # counts mode == thresholding stats mode on the same masks
    thr = stat_obs[0] * TIE
    assert torch.equal(counts.long(), (stat >= thr).sum(dim=0))
    assert torch.equal(maxstat, stat.max(dim=1).values)


# ----------------------------------------------------- real-valued fixtures
REAL_SHAPES = ((65, 64), (135, 130), (300, 257))
REAL_B = 200
# Largest |t - t_ref| measured for the CPU mirror (f32 BLAS sums + the f64
# formula; 8.6e-7, 1.44e-6 and 1.64e-6 at the three shapes) against the
# two-pass fp64 reference over the fixtures below, and the bound the contract
# derives from it: 4x. The MFMA's k-ordered chain and the BLAS blocking
# differ in order but share the eps * sum|ab| error scale.
T_ERR_CPU_MIRROR = 1.64e-6
T_BOUND = 4.0 * T_ERR_CPU_MIRROR


@functools.lru_cache(maxsize=None)
def real_case(S: int, G: int):
    """Normal data, per-gene scale 0.2-3 and offset +-10, centred per gene in
    f64 before the f32 cast (the caller's job in the contract). The
    reference sees the same f32 values. Returns the dict of exact_case plus
    near [G]: relabellings whose reference |t| lies within T_BOUND of the
    gene's threshold."""
    rng = np.random.default_rng(90000 + 100 * S + G)
    scale = rng.uniform(0.2, 3.0, size=G)
    offset = rng.choice([-10.0, 10.0], size=G)
    x = rng.normal(size=(S, G)) * scale + offset
    expr = (x - x.mean(axis=0)).astype(np.float32)
    n1 = S // 3
    labels = np.zeros(S, dtype=np.int64)
    labels[rng.choice(S, size=n1, replace=False)] = 1
    masks = random_masks(rng, S, n1, REAL_B)
    obs = (labels == 1).astype(np.uint8)[None, :]
    stat = ref_stats(expr, masks)
    stat_obs = ref_stats(expr, obs)[0]
    t_thr = np.sqrt(stat_obs * TIE)
    near = (np.abs(np.sqrt(stat) - t_thr[None, :]) <= T_BOUND)
    # the counts comparison below is only informative while few pairs are
    # that close to their threshold
    assert near.mean() <= 0.01, (S, G, float(near.mean()))
    return dict(expr=expr, labels=labels, masks=masks, stat=stat,
                stat_obs=stat_obs, counts=ref_counts(stat, stat_obs),
                maxstat=stat.max(axis=1), near=near.sum(axis=0))


def real_t_error(ops, case, device) -> float:
    """Largest |t - t_ref| over the observed labelling and all mask rows."""
    dev = torch.device(device)
    expr = torch.from_numpy(case["expr"]).to(dev)
    masks = torch.from_numpy(case["masks"]).to(dev)
    obs = torch.from_numpy(
        (case["labels"] == 1).astype(np.uint8)[None, :]).to(dev)
    t_obs = ops.perm_t_stats(expr, obs)[0].sqrt().cpu().numpy()
    t = ops.perm_t_stats(expr, masks).sqrt().cpu().numpy()
    return max(float(np.abs(t_obs - np.sqrt(case["stat_obs"])).max()),
               float(np.abs(t - np.sqrt(case["stat"])).max()))


def check_real(ops, case, device):
    err = real_t_error(ops, case, device)
    print("max |t - t_ref|", err, "bound", T_BOUND)
    assert err <= T_BOUND
    dev = torch.device(device)
    expr = torch.from_numpy(case["expr"]).to(dev)
    masks = torch.from_numpy(case["masks"]).to(dev)
    obs = torch.from_numpy(
        (case["labels"] == 1).astype(np.uint8)[None, :]).to(dev)
    stat_obs = ops.perm_t_stats(expr, obs)[0].contiguous()
    counts, maxstat = ops.perm_t_counts(expr, masks, stat_obs)
    diff = np.abs(counts.cpu().numpy().astype(np.int64) - case["counts"])
    print("count differences", int(diff.sum()), "near pairs",
          int(case["near"].sum()))
    assert (diff <= case["near"]).all()
    t_max = np.sqrt(maxstat.cpu().numpy())
    assert np.abs(t_max - np.sqrt(case["maxstat"])).max() <= T_BOUND


# ------------------------------------------------------------ invariance
def check_row_permutation(ops, case, device):
    dev = torch.device(device)
    expr = torch.from_numpy(case["expr"]).to(dev)
    masks = torch.from_numpy(case["masks"]).to(dev)
    obs = torch.from_numpy(
        (case["labels"] == 1).astype(np.uint8)[None, :]).to(dev)
    stat_obs = ops.perm_t_stats(expr, obs)[0].contiguous()
    c1, m1 = ops.perm_t_counts(expr, masks, stat_obs)
    c2, m2 = ops.perm_t_counts(expr, masks, stat_obs)
    assert torch.equal(c1, c2) and torch.equal(m1, m2)      # run to run
    perm = torch.from_numpy(
        np.random.default_rng(5).permutation(masks.shape[0])).to(dev)
    c3, m3 = ops.perm_t_counts(expr, masks[perm].contiguous(), stat_obs)
    assert torch.equal(c3, c1)
    assert torch.equal(m3, m1[perm])


def check_chunk_invariance(case, device):
    kw = dict(B=200, seed=11, device=device)
    a = scoring.permutation_pvalues(case["expr"], case["labels"], chunk=64,
                                    **kw)
    b = scoring.permutation_pvalues(case["expr"], case["labels"], chunk=200,
                                    **kw)
    c = scoring.permutation_pvalues(case["expr"], case["labels"], chunk=200,
                                    **kw)
    for k in ("t_obs", "p", "q_bh", "p_maxT"):
        assert a[k].tobytes() == b[k].tobytes(), k
        assert b[k].tobytes() == c[k].tobytes(), k
    B = 200
    assert (a["p"] >= 1.0 / (B + 1)).all() and (a["p"] <= 1.0).all()
    assert (a["p_maxT"] >= a["p"]).all()
    assert (a["q_bh"] >= a["p"]).all() and (a["q_bh"] <= 1.0).all()


# -------------------------------------------------------- planted signal
@functools.lru_cache(maxsize=None)
def planted_case():
    """S = 80 balanced, 200 unit-variance genes, the first 10 shifted by
    2 sigma between the groups."""
    rng = np.random.default_rng(424242)
    S, G = 80, 200
    labels = np.zeros(S, dtype=np.int64)
    labels[rng.choice(S, size=40, replace=False)] = 1
    x = rng.normal(size=(S, G))
    x[:, :10] += 2.0 * labels[:, None]
    return x.astype(np.float32), labels


def check_planted(device):
    import kernel_edges as ke
    expr, labels = planted_case()
    B = 2000
    r = scoring.permutation_pvalues(expr, labels, B, seed=3, device=device)
    assert (r["p"][:10] == 1.0 / (B + 1)).all()
    assert (r["p_maxT"] >= r["p"]).all()
    assert (r["q_bh"][:10] <= 0.05).all()
    null_p = r["p"][10:]
    hist = np.bincount(np.minimum((null_p * 10).astype(int), 9),
                       minlength=10)
    exp = len(null_p) / 10.0
    chi2 = float(((hist - exp) ** 2 / exp).sum())
    limit = ke.chi2_upper_quantile(9)
    print("null uniformity chi2", chi2, "limit", limit)
    assert chi2 < limit


# -------------------------------------------------------------- pipeline
SCORE_COLS = ["GeneSymbol", "Lgroup", "d_score", "t_score", "gene_score",
              "biomarker"]
PERM_COLS = ["p_perm", "q_bh", "p_maxT"]


def check_pipeline(tiny_files, tmp_path, device, **extra):
    from g2vec_amd.config import G2VecConfig
    from g2vec_amd.pipeline import run

    def cfg(name, **kw):
        base = dict(expression_file=tiny_files["expression"],
                    clinical_file=tiny_files["clinical"],
                    network_file=tiny_files["network"],
                    result_name=str(tmp_path / name), len_path=15,
                    num_repetition=3, epochs=25, device=device, seed=0)
        base.update(extra)
        base.update(kw)
        return G2VecConfig(**base)

    log = str(tmp_path / "a.jsonl")
    res = run(cfg("a", permutations=64, log_jsonl=log))
    run(cfg("b", permutations=64))
    run(cfg("c"))
    rows = [ln.split("\t") for ln in
            (tmp_path / "a_scores.txt").read_text().splitlines()]
    assert rows[0] == SCORE_COLS + PERM_COLS
    body = rows[1:]
    assert len(body) == res["n_genes"]
    assert all(len(r) == len(rows[0]) for r in body)
    lg = [ln.split("\t") for ln in
          (tmp_path / "a_lgroups.txt").read_text().splitlines()[1:]]
    assert [r[0] for r in body] == [g for g, _ in lg]
    assert [r[1] for r in body] == [v for _, v in lg]
    bio = (tmp_path / "a_biomarkers.txt").read_text().splitlines()[1:]
    assert sorted(r[0] for r in body if r[5] == "1") == bio
    assert {r[5] for r in body} <= {"0", "1"}
    for r in body:
        assert (r[4] == "NA") == (r[1] == "2")
        float(r[2]), float(r[3])
        p, q, pm = float(r[6]), float(r[7]), float(r[8])
        # %.6g: six significant digits, so compare to a relative 1e-5
        lo = 1.0 - 1e-5
        assert lo / 65 <= p <= 1.0
        assert p * lo <= q <= 1.0 and p * lo <= pm <= 1.0
    # two runs byte-identical; the other outputs untouched by the flags
    assert (tmp_path / "a_scores.txt").read_bytes() == \
        (tmp_path / "b_scores.txt").read_bytes()
    for suffix in ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt"):
        assert (tmp_path / ("a" + suffix)).read_bytes() == \
            (tmp_path / ("c" + suffix)).read_bytes(), suffix
    assert not (tmp_path / "c_scores.txt").exists()
    import json
    recs = [json.loads(ln) for ln in open(log)]
    perm = [r for r in recs if r["event"] == "perm"]
    assert perm and perm[0]["B"] == 64 and perm[0]["seed"] == 0
    assert perm[0]["seconds"] >= 0 and perm[0]["n_q05"] >= 0
