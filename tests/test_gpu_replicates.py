"""The replica-batched fast path on the GPU: every batched kernel against the
single-model kernel replica by replica (BITWISE, same device), the exact
inputs against the fp64 references of kernel_edges, ReplicaTrainer against
the single trainer's synchronous loop, and the --replicates CLI.

Shapes (replicate_cases): G = 997 and P = 1003 with path lengths on every
sub-wave and round edge of the eval body and one empty path; R in
{1, 3, 4, 5, 16} = a tile tail, a full tile, many tiles."""
import functools

import pytest
import torch

import kernel_edges as ke
import replicate_cases as rc
from g2vec_amd import ops
from g2vec_amd.config import G2VecConfig
from g2vec_amd.models.replicas import ReplicaTrainer

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GRID_CAPS = ("1", "2", None)      # None: the default cap
QUIET = lambda *a, **k: None      # noqa: E731


@functools.lru_cache(maxsize=None)
def _dev_pathset():
    return tuple(t.to(DEV) for t in rc.pathset())


def _clear_eval_env(monkeypatch, cap=None):
    for name in ("G2VEC_EVAL_GRID", "G2VEC_EVAL_LDS", "G2VEC_EVAL_LDS_GRID"):
        monkeypatch.delenv(name, raising=False)
    if cap is not None:
        monkeypatch.setenv("G2VEC_EVAL_GRID", cap)


def _eval_rep(s_R, p_split):
    genes, offs, labels = _dev_pathset()
    R = s_R.shape[1]
    counts_R = torch.full((R, 2), -123.0, device=DEV)   # the fold overwrites
    dO_R = torch.full((rc.P, R), rc.SENTINEL, device=DEV)
    ops.cbow_eval_counts_rep_(s_R.to(DEV), genes, offs, labels, p_split,
                              counts_R, dO_R=dO_R, inv_b=rc.INV_B)
    return counts_R.cpu(), dO_R.cpu()


# ================================================================== eval
@functools.lru_cache(maxsize=None)
def _eval_single(col: int, p_split: int):
    """ops.cbow_eval_counts_ on column col of the real-valued table, default
    grid: the single op's result does not depend on the grid cap."""
    genes, offs, labels = _dev_pathset()
    counts = torch.full((2,), -123.0, device=DEV)
    dO = torch.full((rc.P,), rc.SENTINEL, device=DEV)
    s = rc.s_table(rc.R_MAX)[:, col].contiguous().to(DEV)
    ops.cbow_eval_counts_(s, genes, offs, labels, p_split, counts, dO=dO,
                          inv_b=rc.INV_B)
    return counts.cpu(), dO.cpu()


@pytest.mark.parametrize("p_split", rc.SPLITS)
@pytest.mark.parametrize("cap", GRID_CAPS)
@pytest.mark.parametrize("R", rc.R_LIST)
def test_eval_rep_bitwise_per_replica(monkeypatch, R, cap, p_split):
    """Normal(0, 0.3) s_R: column r of dO_R over the train split is bitwise
    the single op's dO for s_R[:, r], counts_R[r] its counts; rows at or
    beyond p_split keep the sentinel."""
    _clear_eval_env(monkeypatch)
    refs = [_eval_single(r, p_split) for r in range(R)]
    _clear_eval_env(monkeypatch, cap)
    counts_R, dO_R = _eval_rep(rc.s_table(R), p_split)
    for r, (cnt, d) in enumerate(refs):
        assert torch.equal(rc.bits(dO_R[:p_split, r]), rc.bits(d[:p_split])), r
        assert counts_R[r].tolist() == cnt.tolist(), r
    assert bool((dO_R[p_split:] == rc.SENTINEL).all())


@pytest.mark.parametrize("p_split", rc.SPLITS)
@pytest.mark.parametrize("R", rc.R_LIST)
def test_eval_rep_exact_against_fp64(monkeypatch, R, p_split):
    """Dyadic s_R: every o is exact, so the counts equal the fp64
    reference's and dO_R is within ke.dO_tol of it."""
    _clear_eval_env(monkeypatch)
    counts_R, dO_R = _eval_rep(rc.s_table(R, exact=True), p_split)
    for r in range(R):
        _o, _loss, correct, dref = rc.eval_ref64(r)
        assert float(counts_R[r, 0]) == float(correct[:p_split].sum()), r
        assert float(counts_R[r, 1]) == float(correct[p_split:].sum()), r
        if p_split:
            err = float((dO_R[:p_split, r].double()
                         - dref[:p_split]).abs().max())
            print("replica", r, "dO err", err)
            assert err <= ke.dO_tol(rc.INV_B)


# =============================================================== scatter
@functools.lru_cache(maxsize=None)
def _plan():
    genes, offs, _ = _dev_pathset()
    return ops.build_scatter_plan(genes, offs, rc.G)


@pytest.mark.parametrize("exact", (False, True))
@pytest.mark.parametrize("R", rc.R_LIST)
def test_scatter_rep_bitwise_per_replica(R, exact):
    genes, offs, _ = _dev_pathset()
    dO_R = rc.dO_table(R, exact=exact)
    c_R = ops.scatter_dO_rep(_plan(), dO_R.to(DEV), rc.G).cpu()
    assert c_R.shape == (rc.G, R)
    for r in range(R):
        col = dO_R[:, r].contiguous()
        single = ops.scatter_dO(genes, offs, col.to(DEV), rc.G, plan=_plan())
        assert torch.equal(rc.bits(c_R[:, r]), rc.bits(single)), r
        if exact:
            cg, co, _ = rc.pathset()
            assert ke.bitwise_equal(c_R[:, r],
                                    rc.scatter_ref64(cg, co, col, rc.G)), r


def test_scatter_rep_slab_blocked_plan():
    """800,003 paths = two slabs at SLAB_BYTES, R = 3: slab by slab in
    ascending order like ops.scatter_dO, bitwise; exact against fp64."""
    cg, co = rc.slab_pathset()
    genes, offs = cg.to(DEV), co.to(DEV)
    plan = ops.build_scatter_plan(genes, offs, rc.G)
    assert plan.slab_seg_ptr is not None and len(plan.slab_seg_ptr) == 3
    for exact in (False, True):
        dO_R = rc.dO_table(rc.SLAB_R, exact=exact, n_paths=rc.SLAB_P)
        c_R = ops.scatter_dO_rep(plan, dO_R.to(DEV), rc.G).cpu()
        for r in range(rc.SLAB_R):
            col = dO_R[:, r].contiguous()
            single = ops.scatter_dO(genes, offs, col.to(DEV), rc.G, plan=plan)
            assert torch.equal(rc.bits(c_R[:, r]), rc.bits(single)), r
            if exact:
                assert ke.bitwise_equal(
                    c_R[:, r], rc.scatter_ref64(cg, co, col, rc.G)), r


# ========================================================= Adam tail, GEMV
@pytest.mark.parametrize("h", (64, 128))
@pytest.mark.parametrize("R", rc.R_LIST)
def test_adam_tail_and_gemv_rep_bitwise_per_replica(R, h):
    """Three fused steps (lr_t of t = 1..3) on G = 997 rows (no multiple of
    the rows per block), then the GEMV: W, m, v, who, mO, vO of replica r
    and s_R[:, r] are bitwise the single ops' on replica r's slices."""
    state0 = rc.adam_case(R, h)
    c_steps = state0[6]
    state = tuple(t.clone().to(DEV) for t in state0[:6])
    W, m, v, who, mO, vO = state
    for t, c_R in enumerate(c_steps, start=1):
        ops.adam_rank1_rep(W, m, v, c_R.to(DEV), who, mO, vO, t, rc.ADAM_LR,
                           rc.ADAM_B1, rc.ADAM_B2, rc.ADAM_EPS)
    s_R = torch.full((rc.G, R), rc.SENTINEL, device=DEV)
    ops.gemv_rows_rep_(W, who, s_R)
    names = ("W", "m", "v", "who", "mO", "vO")
    for r in range(R):
        ref = rc.adam_single_chain(state0[:6], c_steps, r, torch.device(DEV))
        for name, got, want in zip(names, state, ref):
            assert torch.equal(rc.bits(got[r]), rc.bits(want)), (name, r)
        out = torch.empty(rc.G, device=DEV)
        ops.gemv_rows(ref[0], ref[3], out)
        assert torch.equal(rc.bits(s_R[:, r]), rc.bits(out)), r


# =============================================================== trainer
TR_R = 4


def _cfg(**kw):
    base = dict(hidden=64, epochs=6, early_stop=False, seed=3, device="cuda")
    base.update(kw)
    return G2VecConfig(**base)


def test_trainer_six_epochs_bitwise_per_replica(monkeypatch):
    """Replica 0 is CbowTrainer stepped six times with run_epoch; replica
    r > 0 is a CbowTrainer state overwritten with replica r's initialisation
    (rc.single_state). W, who and both accuracy histories, bitwise."""
    _clear_eval_env(monkeypatch)
    dev = torch.device(DEV)
    ps = rc.trainer_pathset(dev)
    cfg = _cfg()
    rt = ReplicaTrainer(cfg, rc.G, dev, log=QUIET)
    st = rt.setup(ps, TR_R)
    hist = [rt.run_epoch(st) for _ in range(6)]
    assert st.graph is not None, "epoch-body graph not used"
    for r in range(TR_R):
        tr, s1 = rc.single_state(cfg, ps, dev, r)
        ref = [tr.run_epoch(s1) for _ in range(6)]
        assert [(a[r], v[r]) for a, v in hist] == ref, r
        assert torch.equal(rc.bits(st.W[r]), rc.bits(s1.W)), r
        assert torch.equal(rc.bits(st.who[r]), rc.bits(s1.who)), r


EARLY_SEED = 23     # GPU single-run stop epochs of replicas 0..3: 5, 3, 0, 0


def test_trainer_early_stop_per_replica(monkeypatch):
    """Up to 60 epochs with the reference stop rule: every replica's stop
    epoch, accuracies, history and returned W_ih are bitwise those of its
    single synchronous run. The seed is picked so that the references stop
    at different epochs: a frozen snapshot sits next to a still-training
    replica."""
    _clear_eval_env(monkeypatch)
    dev = torch.device(DEV)
    ps = rc.trainer_pathset(dev)
    cfg = _cfg(epochs=60, early_stop=True, seed=EARLY_SEED)
    refs = []
    for r in range(TR_R):
        tr, s1 = rc.single_state(cfg, ps, dev, r)
        refs.append(rc.single_sync_run(tr, s1, cfg.epochs, True))
    stops = [ref["stop_epoch"] for ref in refs]
    print("reference stop epochs", stops)
    assert any(0 <= s < cfg.epochs - 2 for s in stops)
    assert len(set(stops)) > 1
    res = ReplicaTrainer(cfg, rc.G, dev, log=QUIET).train(ps, TR_R)
    for r, ref in enumerate(refs):
        assert res[r].stop_epoch == ref["stop_epoch"], r
        assert res[r].acc_val == ref["acc_val"], r
        assert res[r].acc_tr == ref["acc_tr"], r
        assert res[r].acc_val_history == ref["hist"], r
        assert torch.equal(rc.bits(res[r].W_ih), rc.bits(ref["W_ih"])), r


def test_trainer_refuses_what_does_not_fit():
    dev = torch.device(DEV)
    ps = rc.trainer_pathset(dev)
    free, _total = torch.cuda.mem_get_info(dev)
    n_genes = int(free // (32 * 1024 * 16)) + 1       # R*G*h*16 > free
    big = type(ps)(ps.genes, ps.offsets, ps.labels, n_genes)
    rt = ReplicaTrainer(_cfg(hidden=1024), n_genes, dev, log=QUIET)
    with pytest.raises(ValueError, match="more than 80%"):
        rt.setup(big, 32)


# =================================================================== CLI
STANDARD = ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt", "_scores.txt",
            "_neighbors.txt")


def test_cli_replicates_on_gpu(tiny_files, tmp_path):
    from g2vec_amd.cli import main
    base = [tiny_files["expression"], tiny_files["clinical"],
            tiny_files["network"]]
    opts = ["-p", "15", "-r", "3", "-e", "25", "-s", "64", "-n", "10",
            "--seed", "0", "--device", "cuda", "--write-scores",
            "--neighbors", "3"]
    assert main(base + [str(tmp_path / "plain")] + opts) == 0
    assert main(base + [str(tmp_path / "rep")] + opts
                + ["--replicates", "3"]) == 0
    for sfx in STANDARD:
        assert (tmp_path / f"rep{sfx}").read_bytes() == \
            (tmp_path / f"plain{sfx}").read_bytes(), sfx
    n_genes = len((tmp_path / "rep_lgroups.txt").read_text().splitlines()) - 1
    stab = (tmp_path / "rep_stability.txt").read_text().splitlines()
    assert len(stab) == 1 + n_genes
    cons = (tmp_path / "rep_consensus_biomarkers.txt").read_text().splitlines()
    assert len(cons) == 1 + 10
