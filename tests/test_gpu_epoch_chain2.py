"""The epoch chain's second cut: round-batched scatter and gw fold, the
GEMV that clears c, and the block graph's one deferred counts fold.

Every check is bitwise. The summation ORDER of the two rewritten kernels is
pinned against the untouched replica kernels at R = 1 (scatter_do_rep_kernel
and fold_gw_adam_rep_kernel spell the order as plain loops) on real-valued
inputs, where any re-association shows: scatter segments sit on every edge
of the 4-slot group and of the 8-slot round (SCAT_U = 8: 511 / 512 / 513 and
1023 / 1024 / 1025 instances), with lanes split between a full group and the
tail (e.g. 193, 300, 449); the fold's row counts sit on the 64-lane and
16-slot-round edges and past the 1024-block cap."""
import functools

import numpy as np
import pytest
import torch

import replicate_cases as rc
from g2vec_amd import ops
from g2vec_amd.config import G2VecConfig
from g2vec_amd.models.cbow import CbowTrainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


# ======================================================== 1. scatter order
SC_P = 4099
SC_G = 40
SEG_LENS = (1, 2, 63, 64, 65, 191, 192, 193, 255, 256, 257, 300, 448, 449,
            511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2085, 4099)
SLAB_CUT = 13                 # two-slab plan: segments [0, 13) and [13, 25)


@functools.lru_cache(maxsize=None)
def _scatter_case():
    """(inst_path, seg_start, genes_flat, genes_slab, dO): 25 segments of
    SEG_LENS instances each, every segment a sorted draw of distinct paths.
    genes_flat: 25 distinct genes of 40 in shuffled order (15 absent).
    genes_slab: distinct within each slab, with the first gene of slab 0
    owning the first segment of slab 1 too."""
    rng = np.random.default_rng(41)
    assert len(SEG_LENS) % 4 != 0 and max(SEG_LENS) == SC_P
    inst = np.concatenate([np.sort(rng.choice(SC_P, size=n, replace=False))
                           for n in SEG_LENS]).astype(np.int32)
    seg_start = np.zeros(len(SEG_LENS) + 1, dtype=np.int32)
    seg_start[1:] = np.cumsum(SEG_LENS)
    genes_flat = rng.permutation(SC_G)[:len(SEG_LENS)].astype(np.int32)
    a = rng.permutation(SC_G)[:SLAB_CUT]
    b = rng.permutation(SC_G)[:len(SEG_LENS) - SLAB_CUT]
    b = np.concatenate([[a[0]], b[b != a[0]]])[:len(SEG_LENS) - SLAB_CUT]
    genes_slab = np.concatenate([a, b]).astype(np.int32)
    assert len(genes_slab) == len(SEG_LENS) and len(set(b.tolist())) == len(b)
    assert set(a.tolist()) & set(b.tolist())
    scale = 10.0 ** rng.uniform(-3, 3, size=SC_P)
    dO = (rng.standard_normal(SC_P) * scale).astype(np.float32)
    return tuple(torch.from_numpy(x).to(DEV)
                 for x in (inst, seg_start, genes_flat, genes_slab, dO))


def _scatter_plan(slabbed: bool) -> ops.ScatterPlan:
    inst, seg_start, genes_flat, genes_slab, _dO = _scatter_case()
    if slabbed:
        return ops.ScatterPlan(inst, seg_start, genes_slab,
                               [0, SLAB_CUT, len(SEG_LENS)])
    return ops.ScatterPlan(inst, seg_start, genes_flat)


@functools.lru_cache(maxsize=None)
def _scatter_ref(slabbed: bool) -> torch.Tensor:
    """The replica kernel at R = 1: the in-tree definition of the order."""
    dO = _scatter_case()[4]
    c_R = ops.scatter_dO_rep(_scatter_plan(slabbed), dO[:, None].contiguous(),
                             SC_G)
    return _bits(c_R[:, 0])


def _check_absent_genes(c: torch.Tensor, plan: ops.ScatterPlan) -> None:
    absent = np.setdiff1d(np.arange(SC_G), plan.seg_gene.cpu().numpy())
    assert len(absent) > 0
    assert bool((_bits(c)[torch.from_numpy(absent)] == 0).all())   # +0.0


@pytest.mark.parametrize("slabbed", [False, True], ids=["flat", "two_slabs"])
def test_scatter_keeps_the_replica_kernels_order(slabbed):
    plan = _scatter_plan(slabbed)
    dO = _scatter_case()[4]
    c = ops.scatter_dO(None, None, dO, SC_G, plan=plan)
    diff = _bits(c) != _scatter_ref(slabbed)
    print("genes differing:", int(diff.sum()))
    assert not bool(diff.any())
    _check_absent_genes(c, plan)


@pytest.mark.parametrize("slabbed", [False, True], ids=["flat", "two_slabs"])
def test_scatter_into_a_zeroed_out_buffer(slabbed):
    plan = _scatter_plan(slabbed)
    dO = _scatter_case()[4]
    out = torch.zeros(SC_G, dtype=torch.float32, device=DEV)
    c = ops.scatter_dO(None, None, dO, SC_G, plan=plan, out=out)
    assert c.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(out), _scatter_ref(slabbed))
    _check_absent_genes(out, plan)


# =========================================================== 2. fold order
FOLD_BLOCKS = (1, 63, 64, 65, 129, 941, 1024, "over")
LR, B1, B2, EPS = 0.005, 0.9, 0.999, 1e-8


def _fold_G(h: int, blocks) -> int:
    """A row count whose fused Adam launch has that many blocks (rows per
    block = 256 / (h / 4), cap 1024); the last block is partial."""
    rpb = 256 // (h // 4)
    if blocks == "over":
        return 1024 * rpb + 37 * rpb + 5      # rows grid-strided past the cap
    return blocks * rpb - (3 if rpb > 3 and blocks > 1 else 0)


def _fold_inputs(G: int, h: int):
    gen = torch.Generator().manual_seed(1000 * h + G)
    W = torch.randn(G, h, generator=gen) * 0.3
    m = (torch.rand(G, h, generator=gen) - 0.5) * 0.2
    v = 0.001 + torch.rand(G, h, generator=gen) * 0.009
    who = torch.randn(h, generator=gen) * 0.1
    mO = (torch.rand(h, generator=gen) - 0.5) * 2e-3
    vO = 0.001 + torch.rand(h, generator=gen) * 0.009
    cs = [torch.randn(G, generator=gen) * 0.01 for _ in range(2)]
    return (W, m, v, who, mO, vO), cs


@pytest.mark.parametrize("blocks", FOLD_BLOCKS)
@pytest.mark.parametrize("h", [64, 128])
def test_fold_gw_adam_keeps_the_replica_kernels_order(h, blocks):
    """Two consecutive fused steps on real-valued W and c: all six tensors
    bitwise those of adam_rank1_rep at R = 1."""
    G = _fold_G(h, blocks)
    rpb = 256 // (h // 4)
    n_blocks = min(-(-G // rpb), 1024)
    assert n_blocks == (1024 if blocks == "over" else blocks)
    assert blocks != "over" or G > 1024 * rpb
    state, cs = _fold_inputs(G, h)
    single = [t.clone().to(DEV) for t in state]
    rep = [t.clone()[None].contiguous().to(DEV) for t in state]
    for t, c in enumerate(cs, start=1):
        c = c.to(DEV)
        W, m, v, who, mO, vO = single
        ops.adam_rank1_fused(W, m, v, c, who, mO, vO, t, LR, B1, B2, EPS)
        W, m, v, who, mO, vO = rep
        ops.adam_rank1_rep(W, m, v, c[:, None].contiguous(), who, mO, vO, t,
                           LR, B1, B2, EPS)
    for name, a, b in zip(("W", "m", "v", "who", "mO", "vO"), single, rep):
        n_diff = int((_bits(a) != _bits(b[0])).sum())
        print(name, "words differing:", n_diff)
        assert n_diff == 0, name


# ================================================================ 3. clear
@pytest.mark.parametrize("h", [64, 128, 256])
def test_gemv_rows_clear_leaves_out_alone_and_zeroes(h):
    G = 1001
    gen = torch.Generator().manual_seed(h)
    W = (torch.randn(G, h, generator=gen) * 0.3).to(DEV)
    x = (torch.randn(h, generator=gen) * 0.1).to(DEV)
    plain = torch.full((G,), -5.0, device=DEV)
    ops.gemv_rows(W, x, plain)
    out = torch.full((G,), -5.0, device=DEV)
    clear = torch.randn(G, generator=gen).to(DEV)
    clear[::7] = float("nan")
    clear[3] = -0.0
    ops.gemv_rows(W, x, out, clear=clear)
    assert torch.equal(_bits(out), _bits(plain))
    assert bool((_bits(clear) == 0).all())                 # +0.0 everywhere


# ======================================================== 4. deferred fold
N_S = 3


@functools.lru_cache(maxsize=None)
def _s_tables():
    gen = torch.Generator().manual_seed(61)
    return tuple((torch.randn(rc.G, generator=gen) * 0.3).to(DEV)
                 for _ in range(N_S))


@functools.lru_cache(maxsize=None)
def _dev_pathset():
    return tuple(t.to(DEV) for t in rc.pathset())


def _set_variant(monkeypatch, variant, cap):
    for name in ("G2VEC_EVAL_GRID", "G2VEC_EVAL_LDS", "G2VEC_EVAL_LDS_GRID"):
        monkeypatch.delenv(name, raising=False)
    if variant == "lds":
        monkeypatch.setenv("G2VEC_EVAL_LDS", str(64 * 1024))
    if cap is not None:
        monkeypatch.setenv("G2VEC_EVAL_GRID", cap)
        monkeypatch.setenv("G2VEC_EVAL_LDS_GRID", cap)


@pytest.mark.parametrize("p_split", rc.SPLITS)
@pytest.mark.parametrize("cap", ["2", None])
@pytest.mark.parametrize("variant", ["subwave", "lds"])
def test_deferred_fold_equals_per_eval_fold(monkeypatch, variant, cap,
                                            p_split):
    """Three evals into a [3, grid, 2] table + one fold_partials_rows_ give
    the counts and dO of three plain evals, bit for bit."""
    _set_variant(monkeypatch, variant, cap)
    genes, offs, labels = _dev_pathset()
    grid = ops.eval_grid(rc.P, rc.G)
    assert grid == (2 if cap else -(-rc.P // 16))
    plain_counts = torch.full((N_S, 2), -123.0, device=DEV)
    plain_dO = torch.full((N_S, rc.P), rc.SENTINEL, device=DEV)
    parts = torch.full((N_S, grid, 2), float("nan"), device=DEV)
    untouched = torch.full((2,), -123.0, device=DEV)
    dO = torch.full((N_S, rc.P), rc.SENTINEL, device=DEV)
    for k, s in enumerate(_s_tables()):
        ops.cbow_eval_counts_(s, genes, offs, labels, p_split,
                              plain_counts[k], dO=plain_dO[k],
                              inv_b=rc.INV_B)
        ops.cbow_eval_counts_(s, genes, offs, labels, p_split, untouched,
                              dO=dO[k], inv_b=rc.INV_B, partials=parts[k])
    assert bool((untouched == -123.0).all())       # no fold was launched
    counts = torch.full((N_S, 2), -123.0, device=DEV)
    ops.fold_partials_rows_(parts, counts)
    print("counts", counts.tolist())
    assert torch.equal(_bits(counts), _bits(plain_counts))
    assert torch.equal(_bits(dO), _bits(plain_dO))
    assert float(counts.sum()) > 0


def test_partials_of_the_wrong_row_count_is_refused(monkeypatch):
    _set_variant(monkeypatch, "subwave", None)
    genes, offs, labels = _dev_pathset()
    grid = ops.eval_grid(rc.P, rc.G)
    counts = torch.full((2,), -123.0, device=DEV)
    dO = torch.full((rc.P,), rc.SENTINEL, device=DEV)
    for rows in (grid - 1, grid + 1):
        bad = torch.full((rows, 2), -9.0, device=DEV)
        with pytest.raises(RuntimeError, match="partials"):
            ops.cbow_eval_counts_(_s_tables()[0], genes, offs, labels, 500,
                                  counts, dO=dO, inv_b=rc.INV_B, partials=bad)
        torch.cuda.synchronize()
        assert bool((bad == -9.0).all())           # nothing was launched
    assert bool((dO == rc.SENTINEL).all()) and bool((counts == -123.0).all())


# ============================================================ 5. invariant
def test_c_buf_is_zero_at_epoch_boundaries(monkeypatch):
    """After an eager epoch, a replayed per-epoch graph and a replayed block
    graph, the trainer's c buffer is all +0.0 again."""
    _set_variant(monkeypatch, "subwave", None)
    ps = rc.trainer_pathset(torch.device(DEV))
    cfg = G2VecConfig(hidden=64, epochs=6, early_stop=False, seed=3,
                      device="cuda")
    tr = CbowTrainer(cfg, rc.G, torch.device(DEV), log=lambda *a, **k: None)
    st = tr.setup(ps)
    assert st.c_buf is not None and bool((_bits(st.c_buf) == 0).all())
    for _ in range(3):                    # eager, capture + replay, replay
        tr.run_epoch(st)
        assert bool((_bits(st.c_buf) == 0).all())
    assert st.graph is not None, "single-epoch graph not used"
    tr._ensure_kgraph(st, k=4)
    assert st.kgraph is not None, "k-block graph not used"
    hist, stop, _W, _who, _acc = tr.run_epochs_pipelined(st, 4,
                                                         early_stop=False)
    torch.cuda.synchronize()
    assert stop == -1 and len(hist) == 4
    assert bool((_bits(st.c_buf) == 0).all())
