"""Synthetic data generators.

Two jobs:
1. `synth_expression_for(...)`: a seeded replacement for the reference's
   bundled ex_EXPRESSION.txt (absent from the mount): a
   module-factor model whose gene-gene correlations differ by prognosis
   group, so the per-group PCC graphs, random paths and CBOW training all
   carry real signal (val-ACC >= 0.88 is reachable, matching the published
   transcript's behaviour).
2. `synth_network` / `synth_clinical` / `synth_dataset`: fully synthetic
   configs at arbitrary scale (BASELINE.json scale configs: 50k/2M,
   200k/20M, 1M/100M).

Model: expr[g, s] = a * f[m(g), s] + noise, where m(g) is a module id,
f ~ N(0,1) per (module, sample), and the loading a is HIGH (1.5) when the
module is "active" for the sample's class (even modules for good, odd for
poor) and LOW (0.25) otherwise. Within an active module,
PCC ~= 1.5^2/(1.5^2+1) ~= 0.69 > 0.5, so the group graph keeps
within-module edges; inactive/cross-module PCC < 0.1 drops out.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

ACTIVE_LOADING = 1.8
INACTIVE_LOADING = 0.25


def module_activity(n_modules: int, shared_frac: float = 0.2) -> np.ndarray:
    """bool [K, 2]: is module k active (high loading) in class 0 / class 1.

    A `shared_frac` fraction of modules is active in BOTH classes — their
    co-expression structure (and hence their random paths) is common to the
    two group graphs, producing the ambiguous/duplicate paths that give the
    real dataset its graded difficulty (dedup drop + sub-1.0 ACC ceiling).
    The rest alternate good-only / poor-only."""
    act = np.zeros((n_modules, 2), dtype=bool)
    n_shared = int(round(n_modules * shared_frac))
    for m in range(n_modules):
        if m < n_shared:
            act[m] = (True, True)
        elif (m - n_shared) % 2 == 0:
            act[m, 0] = True
        else:
            act[m, 1] = True
    return act


def synth_expression(genes: Sequence[str], sample_labels: Sequence[int],
                     module: np.ndarray, seed: int,
                     shared_frac: float = 0.0,
                     off_frac: float = None) -> np.ndarray:
    """f32 [S, G] expression with class-dependent module correlation.

    off_frac controls difficulty: the loading a module keeps in its
    INACTIVE class, as a fraction of ACTIVE_LOADING. The default
    (INACTIVE_LOADING/ACTIVE_LOADING ~ 0.14) makes the two group graphs
    near-disjoint module cliques — paths are class-pure and the CBOW
    separates them in one or two epochs. Raising off_frac toward the
    |PCC|>0.5 threshold (a^2/(a^2+1) = 0.5 at a = 1) keeps the SAME
    modules partially co-expressed in both classes, so the two group
    graphs cover overlapping gene sets with different edge densities:
    walks from the two groups traverse shared genes, identical paths are
    dropped as common, and classification has to accumulate the graded
    per-gene frequency signal over many epochs — reproducing the
    published trajectory's slow 0.63 -> 0.88 climb (README.md:35-41)
    instead of a degenerate epoch-0 crossing."""
    rng = np.random.default_rng(seed + 777)
    S, G = len(sample_labels), len(genes)
    n_modules = int(module.max()) + 1 if G else 0
    f = rng.standard_normal((n_modules, S)).astype(np.float32)
    noise = rng.standard_normal((S, G)).astype(np.float32)
    labels = np.asarray(sample_labels, dtype=np.int64)
    act = module_activity(n_modules, shared_frac)        # [K, 2]
    mod_safe = np.clip(module, 0, None)
    # active[s, g] = act[module[g], labels[s]]
    active = act[:, :].T[labels][:, mod_safe]            # [S, G]
    # per-gene loading heterogeneity: weak-weak gene pairs fall below the
    # PCC threshold, so degrees vary and the label signal is graded
    hetero = rng.uniform(0.8, 1.25, size=G).astype(np.float32)[None, :]
    off_loading = (INACTIVE_LOADING if off_frac is None
                   else ACTIVE_LOADING * float(off_frac))
    a = np.where(active, ACTIVE_LOADING, off_loading).astype(np.float32) * hetero
    a[:, module < 0] = 0.0                               # dead genes: pure noise
    expr = a * f[mod_safe, :].T + noise
    return expr.astype(np.float32)


def synth_clinical(n_samples: int, n_poor: int, seed: int,
                   prefix: str = "SAMP") -> Tuple[List[str], List[int]]:
    rng = np.random.default_rng(seed + 31)
    labels = np.zeros(n_samples, dtype=np.int64)
    labels[rng.choice(n_samples, size=n_poor, replace=False)] = 1
    names = [f"{prefix}-{i:05d}" for i in range(n_samples)]
    return names, labels.tolist()


def synth_network(n_genes: int, n_edges: int, n_modules: int, seed: int,
                  within_frac: float = 0.55, module: np.ndarray = None,
                  gene_prefix: str = "GENE") -> Tuple[List[str], np.ndarray, np.ndarray]:
    """Random directed module-structured network.

    `within_frac` of edges connect two LIVE genes of the same module (these
    are the ones whose |PCC| can clear the 0.5 threshold in the module's
    active group); the rest are uniform random (they decorate the network
    like real interactions that don't co-express). Pass `module` (with -1 =
    dead) to share the assignment with the expression generator.
    Returns (gene names, edge index pairs i64 [E,2], module ids [G])."""
    rng = np.random.default_rng(seed)
    genes = [f"{gene_prefix}{i:07d}" for i in range(n_genes)]
    if module is None:
        module = rng.integers(0, n_modules, size=n_genes)
    # bucket LIVE genes by module for within-module sampling
    live = np.flatnonzero(module >= 0)
    order = live[np.argsort(module[live], kind="stable")]
    mod_sorted = module[order]
    starts = np.searchsorted(mod_sorted, np.arange(n_modules))
    ends = np.searchsorted(mod_sorted, np.arange(n_modules), side="right")
    n_within = int(n_edges * within_frac)
    # within-module edges
    src_m = rng.integers(0, n_modules, size=n_within)
    lo, hi = starts[src_m], ends[src_m]
    ok = hi > lo + 1
    src_m, lo, hi = src_m[ok], lo[ok], hi[ok]
    a = order[lo + rng.integers(0, np.maximum(hi - lo, 1))]
    b = order[lo + rng.integers(0, np.maximum(hi - lo, 1))]
    keep = a != b
    within = np.stack([a[keep], b[keep]], axis=1)
    # cross edges
    n_cross = n_edges - within.shape[0]
    a = rng.integers(0, n_genes, size=n_cross)
    b = rng.integers(0, n_genes, size=n_cross)
    keep = a != b
    cross = np.stack([a[keep], b[keep]], axis=1)
    edges = np.concatenate([within, cross], axis=0)
    return genes, edges, module


def synth_dataset(n_genes: int, n_edges: int, n_samples: int,
                  n_modules: int = 24, seed: int = 0, dead_frac: float = 0.5,
                  shared_frac: float = 0.0) -> Dict:
    """Fully synthetic in-memory dataset (scale configs). Returns dict with
    'expr' f32 [S,G], 'labels' i64 [S], 'genes', 'edge_idx' i64 [E,2],
    'module' [G]."""
    genes, edge_idx, module = synth_network(n_genes, n_edges, n_modules, seed)
    if dead_frac > 0:
        rng = np.random.default_rng(seed + 5)
        dead = rng.choice(n_genes, size=int(n_genes * dead_frac), replace=False)
        module = module.copy()
        module[dead] = -1
    names, labels = synth_clinical(n_samples, n_samples * 43 // 100, seed)
    expr = synth_expression(genes, labels, module, seed, shared_frac=shared_frac)
    return {"expr": expr, "labels": np.asarray(labels), "genes": genes,
            "samples": names, "edge_idx": edge_idx, "module": module}


def synth_pathset(n_genes: int, n_paths: int, n_modules: int = 16,
                  len_path: int = 80, mean_len: float = 21.0, seed: int = 0,
                  label_noise: float = 0.1):
    """A path set of the shape step 3 produces, without walking a graph (the
    trainer benchmarks need the shapes, not the biology): path p stays in
    one module (a contiguous gene range under a seeded permutation, like a
    walk inside one co-expression module), its genes are distinct, its
    length is geometric with mean ~mean_len capped at len_path (the ex_*
    sets average ~21 genes with a tail at len_path), and its label is the
    module's class with a share label_noise flipped. Returns (genes i32
    [nnz], offsets i32 [P + 1], labels f32 [P])."""
    rng = np.random.default_rng(seed)
    msize = n_genes // n_modules
    if msize < 1:
        raise ValueError("need at least one gene per module")
    cap = min(int(len_path), msize)
    lens = np.minimum(rng.geometric(1.0 / mean_len, size=n_paths), cap)
    module = rng.integers(0, n_modules, size=n_paths)
    start = rng.integers(0, msize, size=n_paths)
    offs = np.zeros(n_paths + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    if offs[-1] >= 2 ** 31:
        raise ValueError("path set exceeds the int32 instance index space")
    path_of = np.repeat(np.arange(n_paths), lens)
    k = np.arange(offs[-1]) - offs[path_of]              # position in path
    perm = rng.permutation(n_genes)
    genes = perm[module[path_of] * msize + (start[path_of] + k) % msize]
    labels = (module % 2).astype(np.float32)
    flip = rng.random(n_paths) < label_noise
    labels[flip] = 1.0 - labels[flip]
    return (genes.astype(np.int32), offs.astype(np.int32), labels)


# -------------------------------------------------- file emission (ex_* style)
def write_expression_tsv(path: str, genes: Sequence[str], samples: Sequence[str],
                         expr_sg: np.ndarray) -> None:
    """expr_sg: [S, G] — written gene-wise like the reference format
    (G2Vec.py:479-483)."""
    with open(path, "w") as f:
        f.write("PATIENT\t" + "\t".join(samples) + "\n")
        eg = expr_sg.T  # [G, S]
        for g, row in zip(genes, eg):
            f.write(g + "".join("\t%.4f" % v for v in row) + "\n")


def write_clinical_tsv(path: str, samples: Sequence[str],
                       labels: Sequence[int]) -> None:
    with open(path, "w") as f:
        f.write("PATIENT_BARCODE\tLABEL\n")
        for s, l in zip(samples, labels):
            f.write(f"{s}\t{int(l)}\n")


def write_network_tsv(path: str, genes: Sequence[str],
                      edge_idx: np.ndarray) -> None:
    with open(path, "w") as f:
        f.write("src\tdest\n")
        for a, b in edge_idx:
            f.write(f"{genes[int(a)]}\t{genes[int(b)]}\n")


def make_ex_style_files(outdir: str, n_genes: int = 7523, n_extra: int = 400,
                        n_edges: int = 298799, n_samples: int = 135,
                        n_poor: int = 58, n_modules: int = 16,
                        seed: int = 0, dead_frac: float = 0.5,
                        shared_frac: float = 0.0) -> Dict[str, str]:
    """Emit an ex_*-shaped file triple (expression / clinical / network).

    The network carries n_genes + n_extra genes; the expression matrix
    carries n_genes network genes plus its own extras, so the common-gene
    intersection is exactly n_genes — mirroring the README run's
    7,523-of-9,904 structure (README.md:26-28)."""
    import os
    rng = np.random.default_rng(seed)
    n_net = n_genes + n_extra
    all_net_genes = [f"GENE{i:05d}" for i in range(n_net)]
    # one module assignment shared by network and expression: only COMMON
    # genes (the first n_genes) can be live; dead_frac of those are noise
    module = np.full(n_net, -1, dtype=np.int64)
    live = rng.choice(n_genes, size=int(n_genes * (1.0 - dead_frac)),
                      replace=False)
    module[live] = rng.integers(0, n_modules, size=live.size)
    _, edge_idx, _ = synth_network(n_net, n_edges, n_modules, seed,
                                   module=module)
    # expression covers the first n_genes network genes + private extras
    expr_genes = all_net_genes[:n_genes] + [f"XG{i:05d}" for i in range(n_extra)]
    samples, labels = synth_clinical(n_samples, n_poor, seed, prefix="TCGA-SYN")
    module_expr = np.concatenate([module[:n_genes],
                                  np.full(n_extra, -1, dtype=np.int64)])
    expr = synth_expression(expr_genes, labels, module_expr, seed,
                            shared_frac=shared_frac)

    os.makedirs(outdir, exist_ok=True)
    paths = {
        "expression": os.path.join(outdir, "syn_EXPRESSION.txt"),
        "clinical": os.path.join(outdir, "syn_CLINICAL.txt"),
        "network": os.path.join(outdir, "syn_NETWORK.txt"),
    }
    write_expression_tsv(paths["expression"], expr_genes, samples, expr)
    write_clinical_tsv(paths["clinical"], samples, labels)
    write_network_tsv(paths["network"], all_net_genes, edge_idx)
    return paths
