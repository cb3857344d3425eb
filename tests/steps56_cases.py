"""Inputs and fp64 references shared by test_steps56_cpu.py (mirrors) and
test_gpu_steps56.py (kernels). Plain module, imported as a sibling like
kernel_edges.py, whose exactness helpers it reuses.

k-means inputs are dyadic k/8 with |k| <= 32: every squared difference is a
multiple of 1/64, every column sum a multiple of 1/8, so any fp32 summation
order is exact and kernel, mirror and fp64 reference must agree BITWISE.
References are computed once per process and never modified."""
from __future__ import annotations

import functools

import numpy as np
import torch

import kernel_edges as ke
from g2vec_amd import scoring

KM_K = (2, 3, 8)


def blobs() -> np.ndarray:
    """The three blobs of test_cluster_scoring._embeddings (20 / 30 / 100
    rows, h = 8), restated so this module imports no test file."""
    rng = np.random.default_rng(0)
    a = rng.normal(0, 0.05, size=(20, 8)) + np.array([3.] + [0.] * 7)
    b = rng.normal(0, 0.05, size=(30, 8)) + np.array([0.] * 7 + [3.])
    c = rng.normal(0, 0.05, size=(100, 8))
    return np.concatenate([a, b, c]).astype(np.float32)


def blob_freq() -> np.ndarray:
    freq = np.full(150, 2, dtype=np.int64)
    freq[:20] = 0
    freq[20:50] = 1
    return freq


# -------------------------------------------------------------- k-means
def kmeans_step_ref64(X: torch.Tensor, C: torch.Tensor):
    """fp64 reference of one Lloyd step, independent of cpu_ref: returns
    (D f64[G, k], labels i64[G], sums f64[k, h], counts i64[k],
    inertia f64 scalar, C' f32[k, h]). Asserts the exactness
    preconditions through exact_ref."""
    Xd, Cd = X.double(), C.double()
    k = C.shape[0]
    D = torch.stack([((Xd - Cd[j]) ** 2).sum(dim=1) for j in range(k)], dim=1)
    D = ke.exact_ref(D, D, 1.0 / 64)      # all terms >= 0: sum|terms| = D
    # lowest index wins ties: numpy argmin returns the first minimum
    labels = torch.from_numpy(np.argmin(D.numpy(), axis=1))
    sums = torch.zeros(k, X.shape[1], dtype=torch.float64).index_add_(
        0, labels, Xd)
    asum = torch.zeros(k, X.shape[1], dtype=torch.float64).index_add_(
        0, labels, Xd.abs())
    sums = ke.exact_ref(sums, asum, 1.0 / 8)
    counts = torch.bincount(labels, minlength=k)
    inertia = D.gather(1, labels[:, None]).sum()          # exact in f64
    s32 = sums.numpy().astype(np.float32)
    c32 = counts.numpy().astype(np.float32)
    Cn = C.numpy().copy()
    for j in range(k):
        if counts[j] > 0:
            Cn[j] = s32[j] / c32[j]                      # fp32 division
    return D, labels, sums, counts, inertia, torch.from_numpy(Cn)


@functools.lru_cache(maxsize=None)
def _kmeans_X(G: int, h: int):
    return ke.dyadic(torch.Generator().manual_seed(h + G), (G, h), 32)


@functools.lru_cache(maxsize=None)
def kmeans_case(G: int, h: int, k: int):
    """(X, C, reference tuple) for dyadic X f32[G, h] (shared by every k)
    and C f32[k, h]."""
    X = _kmeans_X(G, h)
    C = ke.dyadic(torch.Generator().manual_seed(1000 * k + h), (k, h), 32)
    return X, C, kmeans_step_ref64(X, C)


@functools.lru_cache(maxsize=None)
def tie_case(h: int = 64, G: int = 37):
    """k = 3 with C[2] a copy of C[0]: every row ties between 0 and 2."""
    gen = torch.Generator().manual_seed(7)
    X = ke.dyadic(gen, (G, h), 32)
    C = ke.dyadic(gen, (3, h), 32)
    C[2] = C[0]
    return X, C, kmeans_step_ref64(X, C)


def step_outputs(X, C, device="cpu"):
    """Fresh out-arguments of ops.kmeans_step, poisoned so an element the
    op does not write shows."""
    G, h = X.shape
    k = C.shape[0]
    return dict(
        labels=torch.full((G,), -7, dtype=torch.int32, device=device),
        C_new=torch.full((k, h), -7.0, device=device),
        sums=torch.full((k, h), -7.0, device=device),
        counts=torch.full((k,), -7, dtype=torch.int32, device=device),
        n_changed=torch.full((1,), -7, dtype=torch.int32, device=device),
        inertia=torch.full((1,), -7.0, dtype=torch.float64, device=device))


def run_step(ops, X, C, prev, device="cpu"):
    out = step_outputs(X, C, device)
    ops.kmeans_step(X.to(device), C.to(device), prev.to(device),
                    out["labels"], out["C_new"], out["sums"], out["counts"],
                    out["n_changed"], out["inertia"])
    return {name: t.cpu() for name, t in out.items()}


def assert_step_matches(out, C, ref, prev):
    """labels equal; sums, counts, inertia and C' bitwise."""
    _D, labels, sums, counts, inertia, Cn = ref
    assert torch.equal(out["labels"].long(), labels)
    assert ke.bitwise_equal(out["sums"], sums)
    assert torch.equal(out["counts"].long(), counts)
    assert out["inertia"].dtype == torch.float64
    assert float(out["inertia"][0]) == float(inertia)
    assert torch.equal(out["C_new"], Cn)
    assert int(out["n_changed"][0]) == int((prev.long() != labels).sum())


# -------------------------------------------------------------- t-scores
T_S = (4, 5, 63, 64, 65, 135)


@functools.lru_cache(maxsize=None)
def t_case(S: int, G: int = 40, n_good: int = 2):
    """Integer-valued expr f32[S, G] in [-8, 8] and labels with n_good
    samples of label 0 (2-vs-rest by default), shuffled. Column 0 is
    constant, column 1 constant inside each group but different between
    them (d1 == 0). Returns (expr, labels i64, host t-scores f32)."""
    rng = np.random.default_rng(100 + S + G)
    expr = rng.integers(-8, 9, size=(S, G)).astype(np.float32)
    labels = np.ones(S, dtype=np.int64)
    labels[rng.choice(S, size=n_good, replace=False)] = 0
    expr[:, 0] = 3.0
    if G > 1:
        expr[:, 1] = np.where(labels == 0, 2.0, -5.0)
    host = scoring.t_scores(expr, labels)
    return torch.from_numpy(expr), torch.from_numpy(labels), host


def ulp_diff_f32(a: np.ndarray, b: np.ndarray) -> int:
    """Largest distance in fp32 ulps between two non-negative f32 arrays
    (adjacent floats of one sign have adjacent bit patterns)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    assert (a >= 0).all() and (b >= 0).all()
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int32).astype(np.int64)
                      - b.view(np.int32).astype(np.int64)).max())


# ------------------------------------------------------------ row norms
@functools.lru_cache(maxsize=None)
def norm_case(G: int, h: int):
    """(W f32[G, h] normal, f64 norms, numpy f32 norms)."""
    gen = torch.Generator().manual_seed(31 * h + G)
    W = torch.randn(G, h, generator=gen)
    ref64 = W.double().pow(2).sum(dim=1).sqrt().numpy()
    return W, ref64, np.linalg.norm(W.numpy(), axis=1)


def assert_norms_match(got: np.ndarray, ref64, ref_np):
    assert got.dtype == np.float32
    assert ulp_diff_f32(got, ref64.astype(np.float32)) <= 1
    np.testing.assert_allclose(got, ref_np, rtol=1e-6, atol=0)


# --------------------------------------------------------- biomarker set
@functools.lru_cache(maxsize=None)
def biomarker_case(num_biomarker: int = 5):
    """Seeded (emb, lg, expr, labels, genes) whose HOST gene scores sit more
    than 1e-4 apart across the top-N cut of both L-groups (asserted here on
    the host path), so a 1-ulp difference in d or t cannot move the cut."""
    rng = np.random.default_rng(2)
    G, S = 60, 24
    emb = rng.normal(size=(G, 64)).astype(np.float32)
    lg = np.array([0] * 20 + [1] * 20 + [2] * 20)
    expr = rng.normal(size=(S, G)).astype(np.float32)
    labels = np.array([0] * 11 + [1] * 13)
    genes = [f"G{i:02d}" for i in range(G)]
    for grp in (0, 1):
        sel = lg == grp
        d = scoring.transform_minmax(np.linalg.norm(emb[sel], axis=1))
        t = scoring.transform_minmax(scoring.t_scores(expr[:, sel], labels))
        score = np.sort(0.5 * (d + t))[::-1]
        gap = float(score[num_biomarker - 1] - score[num_biomarker])
        assert gap > 1e-4, (grp, gap)
    return emb, lg, expr, labels, genes
