"""L-group discovery (reference step 5, G2Vec.py:167-200).

KMeans (k=3, random_state=0 — the only seeded RNG in the reference) over
the gene embeddings; the largest cluster becomes "other" (2); the two
remaining clusters are labelled good (0) / poor (1).

The reference's good/poor disambiguation is DEAD CODE as shipped
(`freqIdx` is a Python list, so `freqIdx==0` is scalar False
and the frequency counts are always 0 — the `else` branch at
G2Vec.py:192-194 always runs, picking good = the larger remaining cluster
index). This module implements the INTENDED semantics by default and
reproduces the shipped behaviour under compat_lgroup_bug=True.
"""
from __future__ import annotations

import numpy as np


def kmeans_torch(X, k: int, seed: int = 0, iters: int = 300,
                 tol: float = 1e-6) -> np.ndarray:
    """Seeded Lloyd k-means with k-means++ init on torch tensors (runs on
    GPU when X is a CUDA tensor). The scalable backend for L-group
    clustering at 200k-1M genes, where sklearn's host KMeans would take
    hours; sklearn (random_state=0, reference parity) stays the default at
    bundled-dataset scale."""
    import torch

    n = X.shape[0]
    gen = torch.Generator().manual_seed(seed)
    idx = [int(torch.randint(n, (1,), generator=gen))]
    for _ in range(k - 1):
        d2 = torch.cdist(X, X[idx]).min(dim=1).values.clamp_(min=0) ** 2
        tot = float(d2.sum())
        probs = (d2 / tot).cpu() if tot > 0 else torch.full((n,), 1.0 / n)
        idx.append(int(torch.multinomial(probs, 1, generator=gen)))
    C = X[idx].clone()
    assign = torch.zeros(n, dtype=torch.long, device=X.device)
    for _ in range(iters):
        assign = torch.cdist(X, C).argmin(dim=1)
        newC = C.clone()
        for j in range(k):
            sel = assign == j
            if bool(sel.any()):
                newC[j] = X[sel].mean(dim=0)
        shift = float((newC - C).norm())
        C = newC
        if shift < tol:
            break
    return assign.cpu().numpy()


KMEANS_HIP_WIDTHS = (64, 128, 256, 512, 1024)   # the kernels' h = 64 * HPL


def _kpp_u01(seed: int, restart: int, draw: int) -> float:
    """Counter-based uniform in [0, 1) for k-means++ draw `draw` of restart
    `restart`: its own splitmix64 stream, warmed by one draw like the walk
    and init streams."""
    from .ops import cpu_ref
    with np.errstate(over="ignore"):
        ctr = np.uint64(restart) * np.uint64(1 << 20) + np.uint64(draw)
        state = np.uint64(seed) ^ np.uint64(
            ctr * np.uint64(0x94D049BB133111EB) + np.uint64(1))
    state, _ = cpu_ref.splitmix64(state)
    _, r = cpu_ref.splitmix64(state)
    return float(r >> np.uint64(11)) * (1.0 / 9007199254740992.0)


def _kpp_init(X, k: int, seed: int, restart: int):
    """Seeded k-means++: first centre floor(u*G), then D^2 sampling through
    kmeans_mind2_ + an f64 cumsum + searchsorted on X's device."""
    import torch

    from . import ops

    G = X.shape[0]
    idx = [min(int(_kpp_u01(seed, restart, 0) * G), G - 1)]
    d2 = torch.full((G,), float("inf"), dtype=torch.float32, device=X.device)
    for draw in range(1, k):
        ops.kmeans_mind2_(X, X[idx[-1]], d2)
        cum = torch.cumsum(d2.double(), 0)
        total = float(cum[-1])
        u = _kpp_u01(seed, restart, draw)
        if total > 0.0:
            target = torch.tensor([u * total], dtype=torch.float64,
                                  device=X.device)
            # right=True: first g with cum[g] > target, so rows at distance
            # 0 (the centres already chosen) are never drawn
            g = int(torch.searchsorted(cum, target, right=True))
        else:
            g = int(u * G)
        idx.append(min(g, G - 1))
    return X[idx].clone()


def _lloyd_buffers(X, k: int, max_iter: int):
    """Out-arguments of kmeans_step shared by every restart: sums, counts,
    inertia and one n_changed slot per step."""
    import torch
    dev = X.device
    return (torch.empty(k, X.shape[1], dtype=torch.float32, device=dev),
            torch.empty(k, dtype=torch.int32, device=dev),
            torch.empty(1, dtype=torch.float64, device=dev),
            torch.empty(max_iter, dtype=torch.int32, device=dev))


def _lloyd(X, C, max_iter: int, check_every: int, bufs):
    """Step from centroids C (updated in place) until no label changes or
    max_iter. Step i writes its n_changed into slot i; every check_every
    steps the new slots come back in one small D2H copy, and the first
    zero among them is the iteration count. Returns (labels, C, inertia,
    iterations)."""
    import torch

    from . import ops

    sums, counts, inertia, changed = bufs
    labels = torch.full((X.shape[0],), -1, dtype=torch.int32,
                        device=X.device)
    it, n_iter = 0, max_iter
    while it < max_iter:
        hi = min(it + check_every, max_iter)
        for i in range(it, hi):
            ops.kmeans_step(X, C, labels, labels, C, sums, counts,
                            changed[i:i + 1], inertia)
        zero = (changed[it:hi] == 0).nonzero().flatten().cpu()
        if zero.numel():
            n_iter = it + int(zero[0]) + 1
            break
        it = hi
    return labels, C, float(inertia[0]), n_iter


def kmeans_hip(X, k: int, seed: int = 0, n_init: int = 10,
               max_iter: int = 300, check_every: int = 4):
    """Seeded Lloyd k-means on the fused kmeans_step op: HIP kernels for a
    CUDA tensor, their CPU mirror for a CPU tensor. X: f32 [G, h] tensor.

    Each of the n_init restarts starts from a seeded k-means++ draw and
    steps until no label changes (or max_iter). n_changed is read back once
    every check_every steps — one small D2H per read, no per-step sync.
    A step with n_changed == 0 is a fixed point of a deterministic step
    (same labels -> same means -> same labels), so the steps run past it
    change nothing and the result is bitwise independent of check_every.
    The restart with the lowest inertia wins, ties to the lowest index.

    Returns (labels i32[G] tensor on X's device, centroids f32[k, h],
    inertia float, iterations int) of the winning restart; iterations
    counts the steps up to and including the first one without a change."""
    import torch

    if not (1 <= k <= 8):
        raise ValueError(f"kmeans_hip: k must be in [1, 8], got {k}")
    if n_init < 1 or max_iter < 1 or check_every < 1:
        raise ValueError("kmeans_hip: n_init, max_iter and check_every "
                         "must be >= 1")
    X = X.float().contiguous()
    G, h = X.shape
    if G < 1:
        raise ValueError("kmeans_hip: X has no rows")
    if h not in KMEANS_HIP_WIDTHS:
        # zero columns add (0 - 0)^2 = 0 to every distance: pad up to the
        # next kernel width (exact), trim the centroids on the way out
        wide = [w for w in KMEANS_HIP_WIDTHS if w >= h]
        if not wide:
            raise ValueError(f"kmeans_hip: h={h} exceeds "
                             f"{KMEANS_HIP_WIDTHS[-1]} columns")
        Xp = torch.zeros(G, wide[0], dtype=torch.float32, device=X.device)
        Xp[:, :h] = X
        X = Xp
    bufs = _lloyd_buffers(X, k, max_iter)
    best = None
    for restart in range(n_init):
        labels, C, val, n_iter = _lloyd(X, _kpp_init(X, k, seed, restart),
                                        max_iter, check_every, bufs)
        if best is None or val < best[2]:
            best = (labels, C[:, :h].contiguous(), val, n_iter)
    return best


def find_lgroups(embeddings, gene_freq: np.ndarray,
                 compat_lgroup_bug: bool = False, backend: str = "auto",
                 device=None, info=None) -> np.ndarray:
    """embeddings: f32 [G, h]; gene_freq: int [G] in {0 good,1 poor,2 other}.
    Returns int32 [G] with 0 good / 1 poor / 2 other.
    backend: 'sklearn' (reference parity: KMeans random_state=0) |
    'torch' (scalable, GPU-capable) | 'hip' (kmeans_hip: fused HIP Lloyd
    step; embeddings may be a torch tensor already on its device, which is
    then used in place) | 'auto' (sklearn up to 50k genes, torch above).
    info: optional dict; the hip backend records kmeans_inertia and
    kmeans_iterations in it."""
    if backend == "auto":
        backend = "sklearn" if embeddings.shape[0] <= 50_000 else "torch"
    if backend == "hip":
        import torch
        X = embeddings
        if not torch.is_tensor(X):
            X = torch.from_numpy(np.ascontiguousarray(X, dtype=np.float32))
            if device is not None:
                X = X.to(device)
        labels, _c, inertia, n_iter = kmeans_hip(X, 3, seed=0)
        km_idx = labels.cpu().numpy()
        if info is not None:
            info.update(kmeans_inertia=inertia, kmeans_iterations=n_iter)
    elif backend == "torch":
        import torch
        X = torch.from_numpy(np.ascontiguousarray(embeddings))
        if device is not None:
            X = X.to(device)
        km_idx = kmeans_torch(X, 3, seed=0)
    else:
        from sklearn.cluster import KMeans
        km = KMeans(n_clusters=3, random_state=0, n_init=10).fit(embeddings)
        km_idx = km.labels_

    # largest cluster -> 2 (strict > keeps the lowest index on ties,
    # G2Vec.py:174-180)
    sizes = [int(np.count_nonzero(km_idx == i)) for i in range(3)]
    largest = 0
    for i in (1, 2):
        if sizes[i] > sizes[largest]:
            largest = i
    remaining = [i for i in range(3) if i != largest]

    if compat_lgroup_bug:
        # shipped behaviour: gpDiff stays all-zero -> else branch ->
        # good = larger remaining index (G2Vec.py:192-194)
        good, poor = remaining[1], remaining[0]
    else:
        gp = np.zeros(3, dtype=np.float32)
        for i in remaining:
            n_good = int(np.count_nonzero((km_idx == i) & (gene_freq == 0)))
            n_poor = int(np.count_nonzero((km_idx == i) & (gene_freq == 1)))
            gp[i] = n_good - n_poor
        if gp[remaining[0]] > gp[remaining[1]]:
            good, poor = remaining[0], remaining[1]
        else:
            good, poor = remaining[1], remaining[0]

    out = np.zeros(embeddings.shape[0], dtype=np.int32)
    out[km_idx == good] = 0
    out[km_idx == poor] = 1
    out[km_idx == largest] = 2
    return out
