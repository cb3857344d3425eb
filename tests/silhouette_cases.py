"""Fixtures and checks shared by the CPU and GPU tests of the L-group
silhouettes (ops.cluster_dist_sums, cluster_quality.silhouette, the
pipeline's silhouette / nearest_lgroup columns).

The reference is independent of cpu_ref: NumPy f64 direct differences,
sqrt(((x - y)**2).sum()), no Gram expansion, and the silhouette formulas in
f64.

Every check takes a torch device, so test_silhouette_cpu.py holds the CPU
mirror and test_gpu_silhouette.py the HIP kernels to the same assertions.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from neighbor_cases import chain_scores

# D against the reference on the exact fixtures: every dot, norm and d^2 is
# exact, so what is left is one f32 sqrt per pair (<= 1 ulp = 2^-23 of d) and
# f64 sums of non-negative terms (G * 2^-53).
EXACT_REL = 2.0 ** -22
SAB_ABS = 1e-6                 # s, a, b on the exact fixtures
# two splits of one call: only the order of at most G f64 additions of
# non-negative terms differs, G * 2^-53 <= 3.7e-12 ... far below at G <= 33000
SPLIT_REL = 1e-12
# reference means of two clusters closer than this (relative) are one value
# summed in two orders: a tie, the lowest index wins
TIE_REL = 1e-12


# ------------------------------------------------------------- reference
def ref_dist(Xq: np.ndarray, X: np.ndarray) -> np.ndarray:
    """f64 [Q, G] Euclidean distances by direct differences."""
    X64 = X.astype(np.float64)
    out = np.empty((Xq.shape[0], X.shape[0]), dtype=np.float64)
    for i, row in enumerate(Xq.astype(np.float64)):
        diff = X64 - row
        out[i] = np.sqrt((diff * diff).sum(axis=1))
    return out


def ref_sums(dist: np.ndarray, labels: np.ndarray, k: int, q_index=None
             ) -> np.ndarray:
    """D f64 [Q, k]: per-cluster sums of dist, each query's q_index left out."""
    dist = dist.copy()
    if q_index is not None:
        rows = np.nonzero(np.asarray(q_index) >= 0)[0]
        dist[rows, np.asarray(q_index)[rows]] = 0.0
    D = np.zeros((dist.shape[0], k), dtype=np.float64)
    for c in range(k):
        D[:, c] = dist[:, labels == c].sum(axis=1)
    return D


def ref_silhouette(D: np.ndarray, own: np.ndarray, n_c: np.ndarray):
    """(s, a, b, nearest) in f64, one query at a time; reference means within
    TIE_REL of the smallest are tied, and the lowest cluster index wins."""
    Q, k = D.shape
    s, a, b = np.zeros(Q), np.zeros(Q), np.zeros(Q)
    nearest = np.zeros(Q, dtype=np.int32)
    for i in range(Q):
        A = int(own[i])
        if n_c[A] >= 2:
            a[i] = D[i, A] / (n_c[A] - 1)
        cand = [(D[i, c] / n_c[c], c) for c in range(k)
                if c != A and n_c[c] > 0]
        lo = min(v for v, _ in cand)
        b[i], nearest[i] = lo, min(c for v, c in cand
                                   if v <= lo * (1.0 + TIE_REL))
        m = max(a[i], b[i])
        if n_c[A] >= 2 and m > 0:
            s[i] = (b[i] - a[i]) / m
    return s, a, b, nearest


# ---------------------------------------------------------- exact fixtures
EXACT_Q = (1, 63, 64, 65, 130)
EXACT_G = (2, 3, 63, 64, 65, 130, 1003, 33000)
EXACT_H = (4, 60, 64, 68, 128, 256, 1024)
EXACT_K = (2, 3, 8)
# every single-axis edge against a fixed triple of the other three (Q = 65: a
# second query tile with one live row; G = 130: a third candidate tile with
# two live columns; h = 68: a second K chunk of one MFMA step), and the
# largest product
EXACT_SHAPES = tuple(dict.fromkeys(
    [(Q, 130, 68, 3) for Q in EXACT_Q]
    + [(65, G, 68, 3) for G in EXACT_G]
    + [(65, 130, h, 3) for h in EXACT_H]
    + [(65, 130, 68, k) for k in EXACT_K]
    + [(130, 33000, 128, 8)]))
LAYOUTS = ("random", "empty", "singleton", "one_tile", "equal_rows",
           "two_of_eight")
# (Q, G, h, k, layout)
EXACT_CASES = tuple((Q, G, h, k, "random") for (Q, G, h, k) in EXACT_SHAPES) \
    + tuple((65, 130, 68, 8 if lay == "two_of_eight" else 3, lay)
            for lay in LAYOUTS[1:])
SPLIT_CASES = ((65, 1003, 68, 3), (65, 33000, 68, 3))
SPLITS = (1, 7, 16, 0)


def make_labels(rng, G: int, k: int, layout: str) -> np.ndarray:
    if layout == "random":
        if G < 4 * k:                    # every cluster it can fill, in turn
            return (np.arange(G) % k).astype(np.int32)
        lab = rng.integers(0, k, size=G)
        lab[:k] = np.arange(k)           # none empty
    elif layout == "empty":
        lab = rng.integers(0, k - 1, size=G)
        lab[lab == 1] = k - 1            # cluster 1 is empty
    elif layout == "singleton":
        lab = rng.integers(0, k - 1, size=G) * (k - 1)    # 0 or k - 1
        lab[2] = 1                       # row 2, a query, alone in cluster 1
    elif layout == "one_tile":
        lab = rng.integers(0, 2, size=G) * 2
        lab[70:100] = 1                  # inside candidate tile 1 (64 .. 127)
    elif layout == "equal_rows":
        lab = rng.integers(0, 2, size=G) * 2
        lab[5:40:3] = 1                  # their rows are made equal
    elif layout == "two_of_eight":
        lab = np.where(rng.integers(0, 2, size=G) == 0, 2, 5)
    else:
        raise ValueError(layout)
    return lab.astype(np.int32)


@functools.lru_cache(maxsize=None)
def exact_case(Q: int, G: int, h: int, k: int, layout: str = "random"):
    """Entries j/8 with |j| <= 16: every dot, squared norm and d^2 is a
    multiple of 1/64 below 2^15, exact in f32 in any summation order (asserted
    below). Rows 0 and G-1 of X are identical (a duplicate at distance exactly
    0) and row 1 is all zero where G >= 3. The queries are rows of X and
    exclude themselves: rows 0, 1, G-1, 2 and 5 first, then random ones.
    Returns dict(Xq, X, labels, q_index, k, n_c, D, s, a, b, nearest)."""
    rng = np.random.default_rng(
        61000 + 7 * Q + 100003 * G + 13 * h + 1009 * k
        + 17 * LAYOUTS.index(layout))
    X = (rng.integers(-16, 17, size=(G, h)) / 8.0).astype(np.float32)
    if G >= 3:
        X[1] = 0.0
    X[G - 1] = X[0]
    labels = make_labels(rng, G, k, layout)
    if layout == "equal_rows":
        X[labels == 1] = X[5]
    q_index = rng.integers(0, G, size=Q).astype(np.int32)
    for i, g in enumerate((0, min(1, G - 1), G - 1, min(2, G - 1),
                           min(5, G - 1))[:Q]):
        q_index[i] = g
    Xq = X[q_index].copy()
    # precondition of the derived bound
    for a_ in (Xq, X):
        assert np.array_equal(a_ * 8, np.round(a_ * 8)) and np.abs(a_).max() <= 2
    assert h * 16.0 <= 2.0 ** 15          # d^2 <= h * 4^2, norms and |dot| less
    dist = ref_dist(Xq, X)
    d2 = dist * dist
    assert np.abs(d2 * 64 - np.round(d2 * 64)).max() <= 1e-6
    n_c = np.bincount(labels, minlength=k)
    D = ref_sums(dist, labels, k, q_index)
    s, a, b, nearest = ref_silhouette(D, labels[q_index], n_c)
    # nearest must be decidable: every other mean is a tie or further behind
    # than both errors together, 2 * 2^-22 (doubled)
    for i in range(Q):
        means = [D[i, c] / n_c[c] for c in range(k)
                 if c != labels[q_index[i]] and n_c[c] > 0]
        for m in means:
            assert m <= b[i] * (1 + TIE_REL) or m > b[i] * (1 + 4 * EXACT_REL)
    return dict(Xq=Xq, X=X, labels=labels, q_index=q_index, k=k, n_c=n_c,
                D=D, s=s, a=a, b=b, nearest=nearest)


def run_sums(ops, case, device, grid_y=0):
    dev = torch.device(device)
    qi = case["q_index"]
    return ops.cluster_dist_sums(
        torch.from_numpy(case["Xq"]).to(dev),
        torch.from_numpy(case["X"]).to(dev),
        torch.from_numpy(case["labels"]).to(dev), case["k"],
        q_index=None if qi is None else torch.from_numpy(qi).to(dev),
        grid_y=grid_y)


def rel_err(D: np.ndarray, ref: np.ndarray) -> float:
    """Largest |D - ref| / ref; where ref == 0, D must be 0 too."""
    zero = ref == 0
    assert (D[zero] == 0).all()
    if zero.all():
        return 0.0
    return float((np.abs(D - ref)[~zero] / ref[~zero]).max())


def check_exact(ops, case, device, grid_y=0):
    """D within 2^-22 of the reference, empty clusters +0.0, nearest equal,
    s / a / b within 1e-6."""
    from g2vec_amd.cluster_quality import silhouette_from_sums
    Dt = run_sums(ops, case, device, grid_y)
    assert Dt.dtype == torch.float64 and tuple(Dt.shape) == case["D"].shape
    D = Dt.cpu().numpy()
    err = rel_err(D, case["D"])
    print("max rel |D - ref|", err, "bound", EXACT_REL)
    assert err <= EXACT_REL
    empty = case["n_c"] == 0
    assert (D[:, empty] == 0).all() and not np.signbit(D[:, empty]).any()
    got = silhouette_from_sums(D, case["labels"][case["q_index"]],
                               case["n_c"])
    assert got["nearest"].dtype == np.int32
    assert np.array_equal(got["nearest"], case["nearest"])
    for key in ("s", "a", "b"):
        e = float(np.abs(got[key] - case[key]).max())
        print("max |%s - ref|" % key, e)
        assert e <= SAB_ABS, key
    return Dt


def check_layout_properties(ops, device):
    """What each label layout is there for, at (65, 130, 68)."""
    from g2vec_amd.cluster_quality import silhouette_from_sums

    def run(layout, k=3):
        case = exact_case(65, 130, 68, k, layout)
        D = run_sums(ops, case, device).cpu().numpy()
        return case, D, silhouette_from_sums(
            D, case["labels"][case["q_index"]], case["n_c"])

    case, D, got = run("empty")
    assert case["n_c"][1] == 0 and (D[:, 1] == 0).all()
    assert (got["nearest"] != 1).all()
    case, D, got = run("singleton")
    assert case["n_c"][1] == 1 and case["q_index"][3] == 2
    assert D[3, 1] == 0 and got["s"][3] == 0 and got["a"][3] == 0
    case, D, got = run("equal_rows")
    own = case["labels"][case["q_index"]]
    assert (own == 1).any()
    assert (D[own == 1, 1] == 0).all() and (got["a"][own == 1] == 0).all()
    assert (got["s"][own == 1] == 1).all()
    case, D, got = run("two_of_eight", 8)
    assert (D[:, [0, 1, 3, 4, 6, 7]] == 0).all()
    assert set(got["nearest"].tolist()) <= {2, 5}
    # the duplicate of row 0 at index G-1 is a neighbour at distance exactly
    # 0, the row itself is left out: both sums equal the reference's
    case, D, got = run("random")
    assert case["q_index"][0] == 0 and case["q_index"][2] == 129
    assert rel_err(D[[0, 2]], case["D"][[0, 2]]) <= EXACT_REL


def check_splits(ops, case, device):
    """GPU launch splits: each within the bound of the reference, within
    1e-12 of each other, and the same split twice bitwise equal."""
    outs = [check_exact(ops, case, device, grid_y=gy) for gy in SPLITS]
    for gy, Dt in zip(SPLITS, outs):
        again = run_sums(ops, case, device, gy)
        assert torch.equal(Dt.view(torch.int64), again.view(torch.int64)), gy
    ref = outs[0].cpu().numpy()
    for Dt in outs[1:]:
        D = Dt.cpu().numpy()
        assert (np.abs(D - ref) <= SPLIT_REL * ref).all()


# ----------------------------------------------------- real-valued fixtures
REAL_SHAPES = ((64, 257, 64, 3), (130, 1003, 128, 3), (65, 3000, 1024, 8))
# Largest relative |D - ref| and absolute |s - ref| of each fixture, from the
# CPU mirror (f32 BLAS blocking) and from a NumPy k-ordered f32 fma chain (the
# MFMA's order) under the same norm and d formulas: (mirror, chain), as
# measure_real() prints them, rounded up. The bound is 4x the larger, the margin of the
# neighbour tests and for the same reason: another, equally valid summation
# order with the same error scale.
REAL_ERR_D = {(64, 257, 64, 3): (9.70e-8, 9.70e-8),
              (130, 1003, 128, 3): (7.82e-8, 7.87e-8),
              (65, 3000, 1024, 8): (7.95e-8, 1.07e-7)}
REAL_ERR_S = {(64, 257, 64, 3): (3.98e-8, 3.94e-8),
              (130, 1003, 128, 3): (3.18e-8, 3.17e-8),
              (65, 3000, 1024, 8): (3.08e-8, 4.70e-8)}
REAL_BOUND_D = {s: 4.0 * max(e) for s, e in REAL_ERR_D.items()}
REAL_BOUND_S = {s: 4.0 * max(e) for s, e in REAL_ERR_S.items()}


@functools.lru_cache(maxsize=None)
def real_case(Q: int, G: int, h: int, k: int):
    """k overlapping Gaussian blobs, no unit scale; the labels are the blob
    of origin, so clusters overlap and some silhouettes are negative. The
    f64 column mean is taken off before the f32 cast (X is what silhouette()
    forms from W = X + anything). Queries: Q distinct rows.
    Returns dict(X, W64, labels, q_index, k, n_c, D, s, a, b, nearest)."""
    rng = np.random.default_rng(73000 + G + h)
    centres = rng.normal(size=(k, h))
    labels = rng.integers(0, k, size=G).astype(np.int32)
    labels[:k] = np.arange(k)
    x = 3.0 * centres[labels] + 1.5 * rng.normal(size=(G, h))
    X = (x - x.mean(axis=0)).astype(np.float32)
    q_index = np.sort(rng.choice(G, size=Q, replace=False)).astype(np.int32)
    dist = ref_dist(X[q_index], X)
    n_c = np.bincount(labels, minlength=k)
    D = ref_sums(dist, labels, k, q_index)
    s, a, b, nearest = ref_silhouette(D, labels[q_index], n_c)
    return dict(Xq=X[q_index].copy(), X=X, labels=labels, q_index=q_index,
                k=k, n_c=n_c, D=D, s=s, a=a, b=b, nearest=nearest)


def chain_sums(case) -> np.ndarray:
    """D of the contract with the dots of chain_scores (ascending-k f32 fma)."""
    Xq, X = case["Xq"], case["X"]
    nq = (Xq.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    nx = (X.astype(np.float64) ** 2).sum(axis=1).astype(np.float32)
    sc = chain_scores(Xq, X)
    d2 = (nq[:, None] + nx[None, :]) - np.float32(2.0) * sc
    d = np.sqrt(np.maximum(d2, np.float32(0.0))).astype(np.float64)
    assert d2.dtype == np.float32
    return ref_sums(d, case["labels"], case["k"], case["q_index"])


def real_errors(ops, shape, device):
    """(rel D error of ops.cluster_dist_sums, abs s error of silhouette)."""
    from g2vec_amd.cluster_quality import silhouette
    case = real_case(*shape)
    D = run_sums(ops, case, device).cpu().numpy()
    got = silhouette(case["X"], case["labels"], case["k"],
                     rows=case["q_index"], device=device)
    return rel_err(D, case["D"]), float(np.abs(got["s"] - case["s"]).max())


def measure_real(ops):
    """Print the table REAL_ERR_D / REAL_ERR_S hold (CPU mirror and chain)."""
    from g2vec_amd.cluster_quality import silhouette_from_sums
    for shape in REAL_SHAPES:
        case = real_case(*shape)
        md, ms = real_errors(ops, shape, "cpu")
        Dc = chain_sums(case)
        got = silhouette_from_sums(Dc, case["labels"][case["q_index"]],
                                   case["n_c"])
        print(shape, "D rel (mirror, chain) = (%.3g, %.3g)" %
              (md, rel_err(Dc, case["D"])),
              "s abs (mirror, chain) = (%.3g, %.3g)" %
              (ms, float(np.abs(got["s"] - case["s"]).max())))


def check_real(ops, shape, device):
    from g2vec_amd.cluster_quality import silhouette
    case = real_case(*shape)
    ed, es = real_errors(ops, shape, device)
    print(device, shape, "max rel |D - ref|", ed, "bound", REAL_BOUND_D[shape],
          "max |s - ref|", es, "bound", REAL_BOUND_S[shape])
    assert ed <= REAL_BOUND_D[shape]
    assert es <= REAL_BOUND_S[shape]
    got = silhouette(case["X"], case["labels"], case["k"],
                     rows=case["q_index"], device=device)
    assert got["s"].dtype == np.float64 and got["nearest"].dtype == np.int32
    assert (np.abs(got["s"]) <= 1).all()
    # a and b have D's relative bound; nearest where the reference decides
    for key in ("a", "b"):
        assert (np.abs(got[key] - case[key])
                <= REAL_BOUND_D[shape] * case[key]).all()
    means = np.where(case["n_c"] > 0, case["D"] / np.maximum(case["n_c"], 1),
                     np.inf)
    means[np.arange(len(means)), case["labels"][case["q_index"]]] = np.inf
    two = np.sort(means, axis=1)[:, :2]
    clear = two[:, 1] > two[:, 0] * (1 + 4 * REAL_BOUND_D[shape])
    assert clear.sum() >= len(clear) // 2
    assert np.array_equal(got["nearest"][clear], case["nearest"][clear])
    own = case["labels"][case["q_index"]]
    for c in range(case["k"]):
        if (own == c).any():
            assert got["mean_by_cluster"][c] == got["s"][own == c].mean()
        else:
            assert np.isnan(got["mean_by_cluster"][c])
    assert got["mean"] == got["s"].mean()


def check_invariances(shape, device):
    """Centring (W + 1000 in f64), q_chunk and rows subsets."""
    from g2vec_amd.cluster_quality import silhouette
    case = real_case(*shape)
    X, lab, k, q = case["X"], case["labels"], case["k"], case["q_index"]
    base = silhouette(X, lab, k, rows=q, device=device)
    far = silhouette(X.astype(np.float64) + 1000.0, lab, k, rows=q,
                     device=device)
    e = float(np.abs(far["s"] - case["s"]).max())
    print("W + 1000: max |s - ref|", e, "bound", REAL_BOUND_S[shape])
    assert e <= REAL_BOUND_S[shape]
    ten = silhouette(torch.from_numpy(X).to(device), lab, k, rows=q,
                     q_chunk=64)
    for key in ("s", "a", "b", "nearest"):
        assert ten[key].tobytes() == base[key].tobytes(), key
    odd = silhouette(X, lab, k, rows=q, device=device, q_chunk=50)
    assert odd["s"].tobytes() == base["s"].tobytes()
    full = silhouette(X, lab, k, device=device)
    assert len(full["s"]) == len(X)
    for key in ("s", "a", "b", "nearest"):
        assert full[key][q].tobytes() == base[key].tobytes(), key
    sub = silhouette(X, lab, k, rows=q[::3], device=device)
    assert sub["s"].tobytes() == base["s"][::3].tobytes()


def check_sklearn(device):
    import pytest
    metrics = pytest.importorskip("sklearn.metrics")
    from g2vec_amd.cluster_quality import silhouette
    shape = (130, 1003, 128, 3)
    case = real_case(*shape)
    got = silhouette(case["X"], case["labels"], 3, device=device)
    ref = metrics.silhouette_samples(case["X"].astype(np.float64),
                                     case["labels"])
    e = float(np.abs(got["s"] - ref).max())
    print("max |s - sklearn|", e, "bound", REAL_BOUND_S[shape])
    assert e <= REAL_BOUND_S[shape]


# ---------------------------------------------------------------- guards
def check_wrapper_errors(ops, device):
    import pytest

    from g2vec_amd.cluster_quality import silhouette
    dev = torch.device(device)
    case = exact_case(65, 130, 68, 3)
    X = torch.from_numpy(case["X"]).to(dev)
    Xq = torch.from_numpy(case["Xq"]).to(dev)
    lab = torch.from_numpy(case["labels"]).to(dev)
    qi = torch.from_numpy(case["q_index"]).to(dev)
    good = dict(Xq=Xq, X=X, labels=lab, k=3, q_index=qi)

    def call(**kw):
        a = dict(good, **kw)
        return ops.cluster_dist_sums(a["Xq"], a["X"], a["labels"], a["k"],
                                     q_index=a["q_index"])

    call()
    nan = X.clone()
    nan[5, 3] = float("nan")
    inf = X.clone()
    inf[7, 0] = float("inf")
    low, high = lab.clone(), lab.clone()
    low[9] = -1
    high[11] = 3
    for kw in (dict(Xq=Xq.double()), dict(X=X.half()),            # dtypes
               dict(labels=lab.float()), dict(q_index=qi.float()),
               dict(Xq=Xq.t().contiguous().t()),                  # contiguity
               dict(X=X.t().contiguous().t()),
               dict(Xq=Xq[:, :64].contiguous()),                  # width
               dict(k=0), dict(k=9),
               dict(labels=low), dict(labels=high),
               dict(labels=lab[:-1]), dict(labels=lab.view(1, -1)),
               dict(q_index=qi[:-1]), dict(q_index=qi.view(-1, 1)),
               dict(X=nan), dict(X=inf), dict(Xq=nan[:65].contiguous())):
        with pytest.raises(ValueError):
            call(**kw)
    with pytest.raises(ValueError, match=r"labels\[9\] = -1"):
        call(labels=low)
    with pytest.raises(ValueError, match=r"labels\[11\] = 3"):
        call(labels=high)
    # fewer than two non-empty clusters, and silhouette's own arguments
    one = np.zeros(130, dtype=np.int32)
    for kw in (dict(labels=one), dict(labels=one + 2),
               dict(labels=case["labels"][:-1]),
               dict(labels=low.cpu().numpy()), dict(k=9), dict(k=0),
               dict(rows=[130]), dict(rows=[-1]), dict(q_chunk=0),
               dict(W=nan.cpu().numpy())):
        a = dict(dict(W=case["X"], labels=case["labels"], k=3), **kw)
        with pytest.raises(ValueError):
            silhouette(a.pop("W"), a.pop("labels"), device=device, **a)


# -------------------------------------------------------------- pipeline
SCORE_COLS = ["GeneSymbol", "Lgroup", "d_score", "t_score", "gene_score",
              "biomarker", "silhouette", "nearest_lgroup"]
PERM_COLS = ["p_perm", "q_bh", "p_maxT"]


def check_pipeline(tiny_files, tmp_path, device, monkeypatch):
    import json

    from g2vec_amd import cli, pipeline
    from g2vec_amd.cluster_quality import silhouette
    from g2vec_amd.config import G2VecConfig

    def cfg(name, **kw):
        base = dict(expression_file=tiny_files["expression"],
                    clinical_file=tiny_files["clinical"],
                    network_file=tiny_files["network"],
                    result_name=str(tmp_path / name), len_path=15,
                    num_repetition=3, epochs=25, device=device, seed=0)
        base.update(kw)
        return G2VecConfig(**base)

    log_a, log_c = str(tmp_path / "a.jsonl"), str(tmp_path / "c.jsonl")
    c = cfg("a", silhouette=True, log_jsonl=log_a)
    res = pipeline.run(c)
    assert c.write_scores                      # implied
    pipeline.run(cfg("b", silhouette=True, permutations=20))
    pipeline.run(cfg("c", write_scores=True, log_jsonl=log_c))
    rows = [ln.split("\t") for ln in
            (tmp_path / "a_scores.txt").read_text().splitlines()]
    assert rows[0] == SCORE_COLS
    body = rows[1:]
    assert len(body) == res["n_genes"]
    assert all(len(r) == len(SCORE_COLS) for r in body)
    head_b = (tmp_path / "b_scores.txt").read_text().splitlines()[0]
    assert head_b.split("\t") == SCORE_COLS + PERM_COLS
    # the flag adds two columns and nothing else
    plain = [ln.split("\t") for ln in
             (tmp_path / "c_scores.txt").read_text().splitlines()]
    assert plain[0] == SCORE_COLS[:6]
    assert [r[:6] for r in rows] == plain
    for suffix in ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt"):
        assert (tmp_path / ("a" + suffix)).read_bytes() == \
            (tmp_path / ("c" + suffix)).read_bytes(), suffix
    # the column against the statistic recomputed from the written files
    vec = np.loadtxt(tmp_path / "a_vectors.txt", skiprows=1,
                     usecols=range(1, 1 + res["W_ih"].shape[1]), ndmin=2)
    lg = np.array([int(ln.split("\t")[1]) for ln in
                   (tmp_path / "a_lgroups.txt").read_text().splitlines()[1:]])
    assert np.array_equal(lg, np.array([int(r[1]) for r in body]))
    col = np.array([float(r[6]) for r in body])
    near = np.array([int(r[7]) for r in body])
    again = silhouette(res["W_ih"], lg, 3, device=device)
    assert np.array_equal(col, np.array(
        [float("%.6f" % v) for v in again["s"]]))
    assert np.array_equal(near, again["nearest"])
    # from the written vectors: every entry moved by <= 5e-7, so every
    # distance, hence a and b, by <= sqrt(h) * 1e-6, and s = 1 - a/b (or
    # b/a - 1) by <= 2 * that / max(a, b) (to first order; doubled), plus
    # the column's own print quantum
    written = silhouette(vec, lg, 3, device=device)
    tol = 4e-6 * np.sqrt(vec.shape[1]) / np.maximum(again["a"], again["b"]) \
        + 1e-6
    print("max |column - s(written vectors)|",
          float(np.abs(col - written["s"]).max()), "tol min", float(tol.min()))
    assert (np.abs(col - written["s"]) <= tol).all()
    assert (near != lg).all()
    assert set(near.tolist()) <= {0, 1, 2}
    recs = [json.loads(ln) for ln in open(log_a)]
    ev = [r for r in recs if r["event"] == "silhouette"]
    assert len(ev) == 1
    ev = ev[0]
    assert abs(ev["mean"] - col.mean()) <= 1e-6
    for g in range(3):
        if (lg == g).any():
            assert abs(ev["mean_by_lgroup"][g] - col[lg == g].mean()) <= 1e-6
    bio = np.array([int(r[5]) for r in body]).astype(bool)
    assert abs(ev["mean_biomarkers"] - col[bio].mean()) <= 1e-6
    assert ev["n_negative"] == int((again["s"] < 0).sum())
    assert ev["seconds"] >= 0
    assert any(r["event"] == "phase" and r["name"] == "silhouette"
               for r in recs)
    assert "silhouette" in res["timers"]
    recs_c = [json.loads(ln) for ln in open(log_c)]
    assert not any(r["event"] == "silhouette" or
                   (r["event"] == "phase" and r["name"] == "silhouette")
                   for r in recs_c)
    # the command line reaches the same field
    a = cli.build_parser().parse_args(["e", "c", "n", "r", "--silhouette"])
    assert cli.args_to_config(a).silhouette
    assert cli.args_to_config(a).write_scores
    a = cli.build_parser().parse_args(["e", "c", "n", "r"])
    assert not cli.args_to_config(a).silhouette
    assert "silhouette" not in repr(G2VecConfig(silhouette=True))
    # one non-empty L-group: NA in both columns, and the run goes through
    real = pipeline.find_lgroups
    monkeypatch.setattr(
        pipeline, "find_lgroups",
        lambda *a_, **k_: np.full_like(real(*a_, **k_), 2))
    log_d = str(tmp_path / "d.jsonl")
    pipeline.run(cfg("d", silhouette=True, log_jsonl=log_d))
    body = [ln.split("\t") for ln in
            (tmp_path / "d_scores.txt").read_text().splitlines()]
    assert body[0] == SCORE_COLS
    assert all(r[6:] == ["NA", "NA"] for r in body[1:])
    assert not any(json.loads(ln)["event"] == "silhouette"
                   for ln in open(log_d))
