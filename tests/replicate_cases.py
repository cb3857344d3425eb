"""Inputs and references shared by test_gpu_replicates.py (GPU) and
test_replicates_cpu.py (its CPU twins). Plain module, imported as a sibling
like kernel_edges.py.

The replica-batched ops promise that, per replica, every output is BITWISE
what the single-model op gives on the same device for that replica's slice.
So the references here are the single ops and the single trainer, driven
replica by replica, plus the fp64 references of kernel_edges for the exact
(dyadic) inputs."""
from __future__ import annotations

import functools

import numpy as np
import torch

import kernel_edges as ke
from g2vec_amd import ops
from g2vec_amd.models.cbow import CbowTrainer, _trunc_normal
from g2vec_amd.paths import PathSet

G = 997
P = 1003                      # not a multiple of 16
EMPTY_AT = 501                # the empty path: lo == hi > 0
# the sub-wave and round edges of the eval body (EVAL_U = 4 and 5)
LENGTHS = (1, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129,
           159, 160, 161, 512)
R_LIST = (1, 3, 4, 5, 16)     # tile tail, full tile, many tiles
R_MAX = max(R_LIST)
SPLITS = (0, 500, P)
SENTINEL = -7.0
INV_B = 1 / 500


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------ kernel level
@functools.lru_cache(maxsize=None)
def pathset():
    rng = np.random.default_rng(78)
    lens = np.array(LENGTHS)[np.arange(P) % len(LENGTHS)]
    lens[EMPTY_AT] = 0
    order = np.argsort(rng.random((P, G)), axis=1)   # distinct genes / path
    genes = np.concatenate([order[p, :lens[p]] for p in range(P)])
    offs = np.zeros(P + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    assert offs[EMPTY_AT] > 0 and offs[EMPTY_AT] == offs[EMPTY_AT + 1]
    assert set(LENGTHS) <= set(lens.tolist())
    labels = rng.integers(0, 2, size=P).astype(np.float32)
    return (torch.from_numpy(genes.astype(np.int32)),
            torch.from_numpy(offs.astype(np.int32)),
            torch.from_numpy(labels))


@functools.lru_cache(maxsize=None)
def _s_master(exact: bool):
    """[G, R_MAX]; the table of R replicas is its first R columns, so one
    set of per-column references serves every R."""
    gen = torch.Generator().manual_seed(7 if exact else 8)
    if exact:
        return ke.dyadic(gen, (G, R_MAX), 8)
    return torch.randn(G, R_MAX, generator=gen) * 0.3


def s_table(R: int, exact: bool = False) -> torch.Tensor:
    return _s_master(exact)[:, :R].contiguous()


@functools.lru_cache(maxsize=None)
def eval_ref64(col: int):
    """kernel_edges' fp64 reference for column col of the dyadic table."""
    genes, offs, labels = pathset()
    return ke.cbow_scalar_ref64(_s_master(True)[:, col].contiguous(), genes,
                                offs, labels, INV_B)


@functools.lru_cache(maxsize=None)
def _dO_master(exact: bool, n_paths: int):
    gen = torch.Generator().manual_seed(9 if exact else 10)
    if exact:
        return ke.dyadic(gen, (n_paths, R_MAX), 8)
    return torch.randn(n_paths, R_MAX, generator=gen) * 0.01


def dO_table(R: int, exact: bool = False, n_paths: int = P) -> torch.Tensor:
    return _dO_master(exact, n_paths)[:, :R].contiguous()


def scatter_ref64(genes, offs, dO_col, n_genes):
    """fp64 c = X^T dO for a dyadic (k/8) dO column, through ke.exact_ref."""
    counts = (offs[1:] - offs[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(len(counts)), counts)
    d = dO_col.double()[seg]
    c = torch.zeros(n_genes, dtype=torch.float64).index_add_(
        0, genes.long(), d)
    a = torch.zeros(n_genes, dtype=torch.float64).index_add_(
        0, genes.long(), d.abs())
    return ke.exact_ref(c, a, 1.0 / 8)


SLAB_P = 800_003              # two slabs at ops.SLAB_BYTES (786,432 paths)
SLAB_R = 3


@functools.lru_cache(maxsize=None)
def slab_pathset():
    """SLAB_P paths of length 1..3 over G genes, distinct within a path."""
    rng = np.random.default_rng(79)
    lens = 1 + (np.arange(SLAB_P) % 3)
    first = rng.integers(0, G, size=SLAB_P)
    step = rng.integers(1, G // 3, size=SLAB_P)
    k = np.concatenate([np.arange(n) for n in (1, 2, 3)] *
                       (SLAB_P // 3 + 1))[:int(lens.sum())]
    path_of = np.repeat(np.arange(SLAB_P), lens)
    genes = (first[path_of] + k * step[path_of]) % G   # 3 * step < G
    offs = np.zeros(SLAB_P + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    assert SLAB_P > ops.SLAB_BYTES // 4
    return (torch.from_numpy(genes.astype(np.int32)),
            torch.from_numpy(offs.astype(np.int32)))


ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 0.005, 0.9, 0.999, 1e-8


def adam_case(R: int, h: int):
    """Replica-major state [R, G, h] / [R, h] from ke.adam_inputs (one seed
    per replica) and three real-valued c_R [G, R], one per step."""
    parts = [ke.adam_inputs(G, h, 40 + r) for r in range(R)]
    W, m, v, _c, who, mO, vO = (torch.stack([p[i] for p in parts])
                                .contiguous() for i in range(7))
    gen = torch.Generator().manual_seed(50 + R)
    c_steps = [(torch.randn(G, R, generator=gen) * 0.01).contiguous()
               for _ in range(3)]
    return W, m, v, who, mO, vO, c_steps


def adam_single_chain(state, c_steps, r: int, device):
    """The single fused op stepped three times on replica r's slices."""
    W, m, v, who, mO, vO = (t[r].clone().to(device) for t in state)
    for t, c_R in enumerate(c_steps, start=1):
        ops.adam_rank1_fused(W, m, v, c_R[:, r].contiguous().to(device), who,
                             mO, vO, t, ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS)
    return W, m, v, who, mO, vO


# ------------------------------------------------------------ trainer level
def trainer_pathset(device) -> PathSet:
    """The 2000-path set of test_gpu_epoch_chain._trainer_pathset."""
    rng = np.random.default_rng(31)
    n = 2000
    lens = rng.integers(1, 40, size=n)
    lens[::7] = 80
    order = np.argsort(rng.random((n, G)), axis=1)
    genes = np.concatenate([order[p, :lens[p]] for p in range(n)])
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    labels = rng.integers(0, 2, size=n).astype(np.float32)
    return PathSet(torch.from_numpy(genes.astype(np.int32)).to(device),
                   torch.from_numpy(offs.astype(np.int32)).to(device),
                   torch.from_numpy(labels).to(device), G)


def replica_init(seed: int, r: int, n_genes: int, h: int, device):
    """Replica r's initial (W, who) in original gene order: the plain run's
    initialisation with seed + r."""
    std = 1.0 / (h ** 0.5)
    if device.type == "cuda":
        W = torch.empty(n_genes, h, dtype=torch.float32, device=device)
        who = torch.empty(h, dtype=torch.float32, device=device)
        ops.trunc_normal_(W, std, seed + r)
        ops.trunc_normal_(who, std, seed + r + 0x9E3779B9)
        return W, who
    gen = torch.Generator()
    gen.manual_seed(seed + r)
    W = _trunc_normal((n_genes, h), std, gen)
    who = _trunc_normal((h,), std, gen)
    return W, who


def single_state(cfg, ps, device, r: int):
    """(trainer, state) of a CbowTrainer for cfg.seed whose weights were
    overwritten with replica r's initialisation, with s_buf, dO_buf and
    W_keep recomputed from them."""
    quiet = lambda *a, **k: None   # noqa: E731
    tr = CbowTrainer(cfg, ps.n_genes, device, log=quiet)
    st = tr.setup(ps)
    if r > 0:
        W, who = replica_init(int(cfg.seed), r, ps.n_genes, cfg.hidden,
                              device)
        if tr.gene_order is not None:
            W = W[tr.gene_order]
        st.W.copy_(W)
        st.who.copy_(who)
        ops.gemv_rows(st.W, st.who, st.s_buf)
        _l, _c, d0 = ops.cbow_fwd_scalar(st.s_buf, st.tr.genes, st.tr.offsets,
                                         st.tr.labels, st.inv_b, True)
        st.dO_buf.copy_(d0)
        st.W_keep.copy_(st.W)
    return tr, st


def single_sync_run(tr, st, epochs: int, early_stop: bool):
    """CbowTrainer.train's synchronous loop on a prepared state."""
    before_val, before_tr, stop_epoch = -1.0, -1.0, -1
    hist = []
    for epoch in range(epochs):
        acc_tr, acc_val = tr.run_epoch(st)
        hist.append(acc_val)
        if early_stop and acc_val < before_val:
            stop_epoch = epoch - 1
            break
        before_val, before_tr = acc_val, acc_tr
        st.W_keep.copy_(st.W)
    return {"stop_epoch": stop_epoch, "acc_val": before_val,
            "acc_tr": before_tr, "hist": hist,
            "W_ih": tr._unrelabel(st.W_keep).clone()}
