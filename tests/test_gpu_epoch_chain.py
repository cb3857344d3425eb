"""The round-batched eval body (eval_counts_body), alone and inside the
trainer's epoch chain.

Exact fixtures (s = k/8) pin the counts to the fp64 reference; a
real-valued s pins the per-lane summation ORDER, bitwise, against
cbow_fwd_scalar_kernel — the in-tree definition of that order. Path
lengths sit on every round edge of the eval body for U = 4 and U = 5
(16U-1 / 16U / 16U+1 and 32U-1 / 32U / 32U+1), on the 16-lane sub-wave
edges, at len_path ~80 and at 512, with one empty path mid-stream."""
import functools

import numpy as np
import pytest
import torch

import kernel_edges as ke
from g2vec_amd import ops
from g2vec_amd.config import G2VecConfig
from g2vec_amd.models.cbow import CbowTrainer
from g2vec_amd.paths import PathSet

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = 997
P = 1003                      # not a multiple of 16
EMPTY_AT = 501                # the empty path: lo == hi > 0
LENGTHS = (1, 15, 16, 17,
           63, 64, 65, 127, 128, 129,        # U = 4 round edges
           79, 80, 81, 159, 160, 161,        # U = 5 round edges, len_path 80
           512)
SENTINEL = -7.0
INV_B = 1 / 500
GRID_CAPS = ("1", "2", None)  # None: the default cap
SPLITS = (0, 500, P)


@functools.lru_cache(maxsize=None)
def _pathset():
    rng = np.random.default_rng(77)
    lens = np.array(LENGTHS)[np.arange(P) % len(LENGTHS)]
    lens[EMPTY_AT] = 0
    order = np.argsort(rng.random((P, G)), axis=1)   # distinct genes / path
    genes = np.concatenate([order[p, :lens[p]] for p in range(P)])
    offs = np.zeros(P + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    assert offs[EMPTY_AT] > 0 and offs[EMPTY_AT] == offs[EMPTY_AT + 1]
    labels = rng.integers(0, 2, size=P).astype(np.float32)
    return (torch.from_numpy(genes.astype(np.int32)),
            torch.from_numpy(offs.astype(np.int32)),
            torch.from_numpy(labels))


@functools.lru_cache(maxsize=None)
def _s_exact():
    return ke.dyadic(torch.Generator().manual_seed(5), (G,), 8)


@functools.lru_cache(maxsize=None)
def _s_real():
    return torch.randn(G, generator=torch.Generator().manual_seed(6)) * 0.3


@functools.lru_cache(maxsize=None)
def _ref_exact():
    genes, offs, labels = _pathset()
    return ke.cbow_scalar_ref64(_s_exact(), genes, offs, labels, INV_B)


@functools.lru_cache(maxsize=None)
def _dev_pathset():
    return tuple(t.to(DEV) for t in _pathset())


def _set_variant(monkeypatch, variant, cap):
    for name in ("G2VEC_EVAL_GRID", "G2VEC_EVAL_LDS", "G2VEC_EVAL_LDS_GRID"):
        monkeypatch.delenv(name, raising=False)
    if variant == "lds":
        monkeypatch.setenv("G2VEC_EVAL_LDS", str(64 * 1024))
    if cap is not None:
        monkeypatch.setenv("G2VEC_EVAL_GRID", cap)
        monkeypatch.setenv("G2VEC_EVAL_LDS_GRID", cap)


def _eval(s_dev, p_split):
    genes, offs, labels = _dev_pathset()
    counts = torch.full((2,), -123.0, device=DEV)     # the fold overwrites
    dO = torch.full((P,), SENTINEL, device=DEV)
    ops.cbow_eval_counts_(s_dev, genes, offs, labels, p_split, counts,
                          dO=dO, inv_b=INV_B)
    return counts, dO


# ============================================================ eval body
@pytest.mark.parametrize("p_split", SPLITS)
@pytest.mark.parametrize("cap", GRID_CAPS)
@pytest.mark.parametrize("variant", ["subwave", "lds"])
def test_eval_body_exact_inputs(monkeypatch, variant, cap, p_split):
    """Dyadic s: every o is exact, so both counts equal the fp64
    reference's and dO is within the project's 1e-7 at inv_b = 1/500."""
    _set_variant(monkeypatch, variant, cap)
    _o, _loss, correct, dref = _ref_exact()
    counts, dO = _eval(_s_exact().to(DEV), p_split)
    counts, dO = counts.cpu(), dO.cpu()
    print("counts", counts.tolist())
    assert float(counts[0]) == float(correct[:p_split].sum())
    assert float(counts[1]) == float(correct[p_split:].sum())
    if p_split:
        err = float((dO[:p_split].double() - dref[:p_split]).abs().max())
        print("dO err", err)
        assert err <= ke.dO_tol(INV_B)
    assert bool((dO[p_split:] == SENTINEL).all())          # untouched


@functools.lru_cache(maxsize=None)
def _fwd_scalar_real():
    """cbow_fwd_scalar over ALL paths with the real-valued s: the order the
    eval body must reproduce. Computed once."""
    genes, offs, labels = _dev_pathset()
    _l, corr, dO = ops.cbow_fwd_scalar(_s_real().to(DEV), genes, offs, labels,
                                       INV_B, True)
    return corr.cpu(), dO.cpu()


@pytest.mark.parametrize("p_split", SPLITS)
@pytest.mark.parametrize("cap", ["2", None])
@pytest.mark.parametrize("variant", ["subwave", "lds"])
def test_eval_body_real_s_keeps_summation_order(monkeypatch, variant, cap,
                                                p_split):
    """Normal(0, 0.3) s: dO over the train split is BITWISE what
    cbow_fwd_scalar gives on the same device, and the counts are the sums
    of its `correct`."""
    _set_variant(monkeypatch, variant, cap)
    corr, dref = _fwd_scalar_real()
    counts, dO = _eval(_s_real().to(DEV), p_split)
    counts, dO = counts.cpu(), dO.cpu()
    assert torch.equal(dO[:p_split].view(torch.int32),
                       dref[:p_split].view(torch.int32))
    assert float(counts[0]) == float(corr[:p_split].sum())
    assert float(counts[1]) == float(corr[p_split:].sum())
    assert bool((dO[p_split:] == SENTINEL).all())


# ============================================================== trainer
def _trainer_pathset():
    rng = np.random.default_rng(31)
    n = 2000
    lens = rng.integers(1, 40, size=n)
    lens[::7] = 80
    order = np.argsort(rng.random((n, G)), axis=1)
    genes = np.concatenate([order[p, :lens[p]] for p in range(n)])
    offs = np.zeros(n + 1, dtype=np.int64)
    offs[1:] = np.cumsum(lens)
    labels = rng.integers(0, 2, size=n).astype(np.float32)
    return PathSet(torch.from_numpy(genes.astype(np.int32)).to(DEV),
                   torch.from_numpy(offs.astype(np.int32)).to(DEV),
                   torch.from_numpy(labels).to(DEV), G)


def test_trainer_epoch_chain_graph_paths_agree(monkeypatch):
    """6 epochs through run_epoch (eager, then the single-epoch graph) and
    6 through one eager epoch + a 5-epoch block graph: bitwise equal W,
    who and accuracy history."""
    _set_variant(monkeypatch, "subwave", None)
    ps = _trainer_pathset()
    dev = torch.device(DEV)
    cfg = G2VecConfig(hidden=64, epochs=6, early_stop=False, seed=3,
                      device="cuda")
    tr1 = CbowTrainer(cfg, G, dev, log=lambda *a, **k: None)
    st1 = tr1.setup(ps)
    hist1 = [tr1.run_epoch(st1)[1] for _ in range(6)]
    assert st1.graph is not None, "single-epoch graph not used"

    tr2 = CbowTrainer(cfg, G, dev, log=lambda *a, **k: None)
    st2 = tr2.setup(ps)
    hist2 = [tr2.run_epoch(st2)[1]]
    tr2._ensure_kgraph(st2, k=5)
    assert getattr(st2, "kgraph", None) is not None, "k-block graph not used"
    hist_k, stop, W2, who2, _ = tr2.run_epochs_pipelined(st2, 5,
                                                         early_stop=False)
    hist2 += list(hist_k)
    torch.cuda.synchronize()
    assert stop == -1 and hist1 == hist2
    assert torch.equal(st1.W.view(torch.int32), W2.view(torch.int32))
    assert torch.equal(st1.who.view(torch.int32), who2.view(torch.int32))
