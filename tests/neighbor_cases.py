"""Fixtures and checks shared by the CPU and GPU tests of the nearest-gene
queries (ops.knn_topk, neighbors.nearest_genes, the pipeline's
<name>_neighbors.txt).

The reference is independent of cpu_ref: a NumPy f64 Xq @ X.T, the self mask
and np.lexsort on (index, -value), i.e. the contract's total order: value
descending, equal values by ascending candidate index.

Every check takes a torch device, so test_neighbors_cpu.py holds the CPU
mirror and test_gpu_neighbors.py the HIP kernels to the same assertions.
"""
from __future__ import annotations

import functools

import numpy as np
import torch


# ------------------------------------------------------------- reference
def ref_scores(Xq: np.ndarray, X: np.ndarray, q_index=None) -> np.ndarray:
    """f64 [Q, G] dots, the excluded candidate of each query at -inf."""
    sc = Xq.astype(np.float64) @ X.astype(np.float64).T
    if q_index is not None:
        rows = np.nonzero(np.asarray(q_index) >= 0)[0]
        sc[rows, np.asarray(q_index)[rows]] = -np.inf
    return sc


def ref_topk(sc: np.ndarray, k: int):
    """(idx i32 [Q, k], val f64 [Q, k]) of the scores of ref_scores: lexsort
    on (index, -value); tail idx -1 / val -inf."""
    Q, G = sc.shape
    idx = np.full((Q, k), -1, dtype=np.int32)
    val = np.full((Q, k), -np.inf, dtype=np.float64)
    if G == 0:
        return idx, val
    cand = np.broadcast_to(np.arange(G), (Q, G))
    order = np.lexsort((cand, -sc), axis=-1)[:, :k]
    v = np.take_along_axis(sc, order, axis=1)
    n = order.shape[1]
    idx[:, :n] = np.where(np.isneginf(v), -1, order)
    val[:, :n] = v
    return idx, val


# ---------------------------------------------------------- exact fixtures
EXACT_Q = (1, 63, 64, 65, 130)
EXACT_G = (1, 2, 63, 64, 65, 130, 1003, 33000)
EXACT_H = (4, 8, 60, 64, 68, 128, 1024)
EXACT_K = (1, 2, 10, 63, 64)
# every single-axis edge against a fixed triple of the other three (Q = 65: a
# second query tile with one live row; G = 130: a third candidate tile with
# two live columns; h = 68: a second K chunk of one MFMA step; the G axis at
# k = 10 covers k > G - 1 at G = 1, 2), plus the corners where two axes are
# large at once and k > G - 1 at the widest list
EXACT_SHAPES = tuple(dict.fromkeys(
    [(Q, 130, 68, 10) for Q in EXACT_Q]
    + [(65, G, 68, 10) for G in EXACT_G]
    + [(65, 130, h, 10) for h in EXACT_H]
    + [(65, 130, 68, k) for k in EXACT_K]
    + [(65, 63, 68, 64), (64, 64, 64, 64), (130, 1003, 1024, 63),
       (130, 33000, 128, 64), (1, 1, 4, 1)]
    # further K-chunk edges: 2 and 4 full chunks of 64, and one step either side
    + [(65, 130, h, 10) for h in (124, 132, 256, 260)]))
EXACT_CASES = tuple((Q, G, h, k, qi) for (Q, G, h, k) in EXACT_SHAPES
                    for qi in (False, True))


@functools.lru_cache(maxsize=None)
def exact_case(Q: int, G: int, h: int, k: int, with_q_index: bool):
    """Entries j/8 with |j| <= 16: every dot is a multiple of 1/64 below 2^12,
    exact in f32 in any summation order, and small integers give many equal
    dots, so the tie rule decides on nearly every row. Rows 0 and G-1 of X
    are identical and row 1 is all zero (where G >= 3 leaves room; G = 2:
    two identical rows). with_q_index: the queries are rows of X and exclude
    themselves (one of them carries -1: nothing excluded); else independent
    rows, q_index None.
    Returns dict(Xq, X, q_index, idx, val)."""
    rng = np.random.default_rng(
        31000 + 7 * Q + 100003 * G + 13 * h + 1009 * k + int(with_q_index))
    X = (rng.integers(-16, 17, size=(G, h)) / 8.0).astype(np.float32)
    if G >= 3:
        X[1] = 0.0
    if G >= 2:
        X[G - 1] = X[0]
    if with_q_index:
        q_index = rng.integers(0, G, size=Q).astype(np.int32)
        q_index[0] = 0                       # the duplicated row
        if Q >= 3:
            q_index[1] = min(1, G - 1)       # the zero row
            q_index[2] = G - 1
        Xq = X[q_index].copy()
        if Q >= 4:
            q_index[3] = -1
    else:
        q_index = None
        Xq = (rng.integers(-16, 17, size=(Q, h)) / 8.0).astype(np.float32)
        if Q >= 2:
            Xq[1] = 0.0
    # precondition of the exact comparison
    for a in (Xq, X):
        assert np.array_equal(a * 8, np.round(a * 8)) and np.abs(a).max() <= 2
    assert (np.abs(Xq.astype(np.float64)) @ np.abs(X.astype(np.float64)).T
            ).max() < 2.0 ** 12
    sc = ref_scores(Xq, X, q_index)
    assert np.array_equal(sc[np.isfinite(sc)] * 64,
                          np.round(sc[np.isfinite(sc)] * 64))
    idx, val = ref_topk(sc, k)
    return dict(Xq=Xq, X=X, q_index=q_index, idx=idx, val=val)


def run_knn(ops, case, device, k, grid_y=0):
    dev = torch.device(device)
    qi = case["q_index"]
    return ops.knn_topk(
        torch.from_numpy(case["Xq"]).to(dev), torch.from_numpy(case["X"]).to(dev),
        k, q_index=None if qi is None else torch.from_numpy(qi).to(dev),
        grid_y=grid_y)


def check_exact(ops, case, device, grid_y=0):
    """idx and val equal the reference exactly."""
    k = case["idx"].shape[1]
    idx, val = run_knn(ops, case, device, k, grid_y)
    assert idx.dtype == torch.int32 and val.dtype == torch.float32
    assert tuple(idx.shape) == case["idx"].shape == tuple(val.shape)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert np.array_equal(idx, case["idx"])
    assert np.array_equal(val.astype(np.float64), case["val"])
    # fewer candidates than k: the tail
    qi = case["q_index"]
    n_cand = case["X"].shape[0] - (0 if qi is None else (qi >= 0).astype(int))
    tail = np.arange(k)[None, :] >= np.broadcast_to(n_cand, (len(idx),))[:, None]
    assert (idx[tail] == -1).all() and np.isneginf(val[tail]).all()
    assert (idx[~tail] >= 0).all()


# ----------------------------------------------------- real-valued fixtures
# (Q, G, h, k) -> seed. On the two smaller shapes the seed is one for which
# the reference alone separates every row's top k + 1 by more than 2 * bound
# (asserted in real_case), so idx must EQUAL the reference there. At h = 1024
# / k = 64 the reference gaps fall to ~1e-7, below any f32 bound: rules 1-4
# of check_real only.
REAL_SEEDS = {(64, 257, 64, 10): 0, (130, 1003, 128, 10): 3,
              (65, 3000, 1024, 64): 0}
REAL_SHAPES = tuple(REAL_SEEDS)
STRICT_SHAPES = REAL_SHAPES[:2]
# Largest |val - ref| over all Q x G candidate scores of each fixture (a
# superset of the k selected, the excluded self apart), from the CPU
# mirror (f32 BLAS blocking) and from a NumPy k-ordered f32 fma chain (the
# MFMA's order): (mirror, chain). The bound is 4x the larger, the margin of
# the permutation tests and for the same reason: another, equally valid
# summation order with the same eps * sum|ab| error scale. It must stay
# below the derivable h * 2^-24 (asserted below).
# The smallest reference gaps among the top k + 1 of the strict fixtures
# are 3.4e-5 and 1.8e-5.
REAL_ERR = {(64, 257, 64, 10): (1.69e-7, 1.69e-7),
            (130, 1003, 128, 10): (2.67e-7, 2.67e-7),
            (65, 3000, 1024, 64): (1.67e-7, 7.12e-7)}
REAL_BOUND = {s: 4.0 * max(e) for s, e in REAL_ERR.items()}
for _s, _b in REAL_BOUND.items():
    assert _b < _s[2] * 2.0 ** -24, (_s, _b)


def chain_scores(Xq: np.ndarray, X: np.ndarray) -> np.ndarray:
    """f32 [Q, G]: acc = fma(a_k, b_k, acc) over ascending k. The f32 x f32
    product is exact in f64, so one f64 add rounded to f32 is the fma up to
    a double rounding that moves nothing at this scale."""
    acc = np.zeros((Xq.shape[0], X.shape[0]), dtype=np.float32)
    a64, b64 = Xq.astype(np.float64), X.astype(np.float64)
    for kk in range(Xq.shape[1]):
        acc = (acc.astype(np.float64)
               + a64[:, kk:kk + 1] * b64[:, kk][None, :]).astype(np.float32)
    return acc


def blob_rows(rng, G: int, h: int) -> np.ndarray:
    """Unit rows (f64 norm, f32 result) of overlapping Gaussian blobs."""
    n_blob = 8
    centres = rng.normal(size=(n_blob, h))
    x = centres[rng.integers(0, n_blob, size=G)] + 1.5 * rng.normal(size=(G, h))
    x /= np.sqrt((x * x).sum(axis=1))[:, None]
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def real_case(Q: int, G: int, h: int, k: int):
    """The queries are Q distinct rows of X and exclude themselves.
    Returns dict(Xq, X, q_index, sc (f64 [Q, G] reference), idx, val)."""
    shape = (Q, G, h, k)
    rng = np.random.default_rng(52000 + 1000 * REAL_SEEDS[shape] + h)
    X = blob_rows(rng, G, h)
    q_index = rng.choice(G, size=Q, replace=False).astype(np.int32)
    Xq = X[q_index].copy()
    sc = ref_scores(Xq, X, q_index)
    idx, val = ref_topk(sc, k)
    if shape in STRICT_SHAPES:
        top = ref_topk(sc, k + 1)[1]
        gap = float((top[:, :-1] - top[:, 1:]).min())
        assert gap > 2.0 * REAL_BOUND[shape], (shape, gap)
    return dict(Xq=Xq, X=X, q_index=q_index, sc=sc, idx=idx, val=val)


def real_error(ops, case, device) -> float:
    """Largest |val - ref[idx]| of a top-k run (k as the fixture's)."""
    k = case["idx"].shape[1]
    idx, val = run_knn(ops, case, device, k)
    idx, val = idx.cpu().numpy().astype(np.int64), val.cpu().numpy()
    ref = np.take_along_axis(case["sc"], idx, axis=1)
    return float(np.abs(val.astype(np.float64) - ref).max())


def check_real(ops, shape, device, grid_y=0):
    case = real_case(*shape)
    b = REAL_BOUND[shape]
    k = shape[3]
    idx, val = run_knn(ops, case, device, k, grid_y)
    idx = idx.cpu().numpy().astype(np.int64)
    val = val.cpu().numpy().astype(np.float64)
    sc, qi = case["sc"], case["q_index"]
    assert (idx >= 0).all()                          # k <= G - 1 here
    ref_at = np.take_along_axis(sc, idx, axis=1)
    print("max |val - ref[idx]|", float(np.abs(val - ref_at).max()),
          "max |val - ref_sorted|", float(np.abs(val - case["val"]).max()),
          "bound", b)
    # 1. the contract's order
    d = val[:, 1:] - val[:, :-1]
    assert (d <= 0).all()
    assert (idx[:, 1:] > idx[:, :-1])[d == 0].all()
    # 2. / 3. values against the reference, by candidate and by rank
    assert (np.abs(val - ref_at) <= b).all()
    assert (np.abs(val - case["val"]) <= b).all()
    # 4. a set of k distinct others, and nothing clearly better left out
    srt = np.sort(idx, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    assert (idx != qi[:, None]).all()
    left = sc.copy()
    np.put_along_axis(left, idx, -np.inf, axis=1)
    assert (left.max(axis=1) <= ref_at[:, -1] + 2.0 * b).all()
    if shape in STRICT_SHAPES:
        assert np.array_equal(idx, case["idx"])


# ------------------------------------------------------------ invariance
def check_q_chunk(shape, device):
    from g2vec_amd.neighbors import nearest_genes
    case = real_case(*shape)
    k = shape[3]
    a = nearest_genes(case["X"], case["q_index"], k, device=device, q_chunk=64)
    b = nearest_genes(case["X"], case["q_index"], k, device=device)
    c = nearest_genes(torch.from_numpy(case["X"]), case["q_index"], k,
                      metric="dot", device=device)
    assert a[0].dtype == np.int32 and a[1].dtype == np.float32
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes()
    if shape in STRICT_SHAPES:
        assert np.array_equal(a[0], case["idx"])
        assert np.array_equal(c[0], case["idx"])


def check_wrapper_errors(ops, device):
    from g2vec_amd.neighbors import nearest_genes
    import pytest
    dev = torch.device(device)
    case = exact_case(65, 130, 68, 10, True)
    X = torch.from_numpy(case["X"]).to(dev)
    bad = X.clone()
    bad[5, 3] = float("nan")
    with pytest.raises(ValueError):
        ops.knn_topk(X[:4].contiguous(), bad, 3)
    with pytest.raises(ValueError):
        ops.knn_topk(bad[4:6].contiguous(), X, 3)
    for k in (0, 65):
        with pytest.raises(ValueError):
            ops.knn_topk(X[:4].contiguous(), X, k)
        with pytest.raises(ValueError):
            nearest_genes(X, [0], k, device=device)
    with pytest.raises(ValueError):
        ops.knn_topk(X[:4, :8].contiguous(), X, 3)
    with pytest.raises(ValueError):
        nearest_genes(bad, [0, 1], 3, device=device)
    bad[5, 3] = float("inf")
    with pytest.raises(ValueError):
        nearest_genes(bad, [0, 1], 3, device=device)
    for q in ([130], [-1], [0, 129, 200]):
        with pytest.raises(ValueError):
            nearest_genes(X, q, 3, device=device)
    with pytest.raises(ValueError):
        nearest_genes(X, [0], 3, metric="euclid", device=device)


def check_zero_row_cosine(device):
    """A zero row stays zero under the cosine metric: similarity 0 with
    everything, so its neighbours are the lowest indices."""
    from g2vec_amd.neighbors import nearest_genes
    case = exact_case(65, 130, 68, 10, True)
    idx, sim = nearest_genes(case["X"], [1], 5, device=device)
    assert idx.tolist() == [[0, 2, 3, 4, 5]]
    assert (sim == 0).all()
    # the duplicated row's twin comes first, at cosine 1
    idx, sim = nearest_genes(case["X"], [0], 1, device=device)
    assert idx.tolist() == [[129]] and abs(float(sim[0, 0]) - 1.0) <= 1e-6


# -------------------------------------------------------------- pipeline
NBR_COLS = ["GeneSymbol", "Rank", "Neighbor", "Cosine", "NeighborLgroup",
            "NeighborBiomarker"]


def check_pipeline(tiny_files, tmp_path, device):
    import json

    from g2vec_amd.config import G2VecConfig
    from g2vec_amd.pipeline import run

    def cfg(name, **kw):
        base = dict(expression_file=tiny_files["expression"],
                    clinical_file=tiny_files["clinical"],
                    network_file=tiny_files["network"],
                    result_name=str(tmp_path / name), len_path=15,
                    num_repetition=3, epochs=25, device=device, seed=0)
        base.update(kw)
        return G2VecConfig(**base)

    K = 5
    log = str(tmp_path / "a.jsonl")
    res = run(cfg("a", neighbors=K, log_jsonl=log))
    run(cfg("b", neighbors=K))
    run(cfg("c"))
    run(cfg("d", neighbors=K, neighbors_of="all"))
    rows = [ln.split("\t") for ln in
            (tmp_path / "a_neighbors.txt").read_text().splitlines()]
    assert rows[0] == NBR_COLS
    body = rows[1:]
    bio = (tmp_path / "a_biomarkers.txt").read_text().splitlines()[1:]
    lg = dict(ln.split("\t") for ln in
              (tmp_path / "a_lgroups.txt").read_text().splitlines()[1:])
    assert len(body) == len(bio) * K
    assert all(len(r) == len(NBR_COLS) for r in body)
    for i, gene in enumerate(bio):                 # query order = the file's
        blk = body[i * K:(i + 1) * K]
        assert [r[0] for r in blk] == [gene] * K
        assert [r[1] for r in blk] == [str(j) for j in range(1, K + 1)]
        assert gene not in [r[2] for r in blk]
        assert len({r[2] for r in blk}) == K
        cos = [float(r[3]) for r in blk]
        assert all(a >= b for a, b in zip(cos, cos[1:]))
        assert all(-1.0 - 1e-6 <= c <= 1.0 + 1e-6 for c in cos)
        for r in blk:
            assert r[4] == lg[r[2]]
            assert r[5] == ("1" if r[2] in bio else "0")
    # two runs byte-identical; the other outputs untouched by the flag
    assert (tmp_path / "a_neighbors.txt").read_bytes() == \
        (tmp_path / "b_neighbors.txt").read_bytes()
    for suffix in ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt"):
        assert (tmp_path / ("a" + suffix)).read_bytes() == \
            (tmp_path / ("c" + suffix)).read_bytes(), suffix
    assert not (tmp_path / "c_neighbors.txt").exists()
    recs = [json.loads(ln) for ln in open(log)]
    ev = [r for r in recs if r["event"] == "neighbors"]
    assert ev and ev[0]["Q"] == len(bio) and ev[0]["k"] == K
    assert ev[0]["seconds"] >= 0
    assert any(r["event"] == "phase" and r["name"] == "neighbors"
               for r in recs)
    assert "neighbors" in res["timers"]
    all_rows = (tmp_path / "d_neighbors.txt").read_text().splitlines()[1:]
    assert len(all_rows) == res["n_genes"] * K
    genes = list(lg)
    assert [ln.split("\t")[0] for ln in all_rows[::K]] == genes


def check_validate():
    import pytest

    from g2vec_amd.config import G2VecConfig
    G2VecConfig(neighbors=64, neighbors_of="all").validate()
    assert G2VecConfig().neighbors == 0
    assert G2VecConfig().neighbors_of == "biomarkers"
    for kw in (dict(neighbors=65), dict(neighbors=-1),
               dict(neighbors=5, neighbors_of="some")):
        with pytest.raises(ValueError):
            G2VecConfig(**kw).validate()
