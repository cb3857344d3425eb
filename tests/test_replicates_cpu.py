"""--replicates on the CPU: the batched ops' mirrors and ReplicaTrainer
against the single ops / single trainer replica by replica, the stability
summary on hand-written inputs, the config guards and the CLI end to end."""
import numpy as np
import pytest
import torch

import kernel_edges as ke
import replicate_cases as rc
from g2vec_amd import ops, stability
from g2vec_amd.config import G2VecConfig
from g2vec_amd.models.replicas import ReplicaTrainer

CPU = torch.device("cpu")
RS = (1, 3)


# ============================================================ op mirrors
@pytest.mark.parametrize("p_split", rc.SPLITS)
@pytest.mark.parametrize("R", RS)
def test_eval_rep_equals_single_per_replica(R, p_split):
    genes, offs, labels = rc.pathset()
    s_R = rc.s_table(R)
    counts_R = torch.full((R, 2), -123.0)
    dO_R = torch.full((rc.P, R), rc.SENTINEL)
    ops.cbow_eval_counts_rep_(s_R, genes, offs, labels, p_split, counts_R,
                              dO_R=dO_R, inv_b=rc.INV_B)
    for r in range(R):
        cnt = torch.zeros(2)
        d = torch.empty(p_split)
        ops.cbow_eval_counts_(s_R[:, r].contiguous(), genes, offs, labels,
                              p_split, cnt, dO=d, inv_b=rc.INV_B)
        assert torch.equal(rc.bits(dO_R[:p_split, r]), rc.bits(d))
        assert torch.equal(counts_R[r], cnt)
    assert bool((dO_R[p_split:] == rc.SENTINEL).all())


@pytest.mark.parametrize("R", RS)
def test_eval_rep_exact_against_fp64(R):
    genes, offs, labels = rc.pathset()
    p_split = 500
    counts_R = torch.zeros(R, 2)
    dO_R = torch.zeros(rc.P, R)
    ops.cbow_eval_counts_rep_(rc.s_table(R, exact=True), genes, offs, labels,
                              p_split, counts_R, dO_R=dO_R, inv_b=rc.INV_B)
    for r in range(R):
        _o, _loss, correct, dref = rc.eval_ref64(r)
        assert float(counts_R[r, 0]) == float(correct[:p_split].sum())
        assert float(counts_R[r, 1]) == float(correct[p_split:].sum())
        err = float((dO_R[:p_split, r].double() - dref[:p_split]).abs().max())
        assert err <= ke.dO_tol(rc.INV_B)


@pytest.mark.parametrize("R", RS)
def test_scatter_rep_equals_single_per_replica(R):
    genes, offs, _ = rc.pathset()
    plan = ops.build_scatter_plan(genes, offs, rc.G)
    for exact in (False, True):
        dO_R = rc.dO_table(R, exact=exact)
        c_R = ops.scatter_dO_rep(plan, dO_R, rc.G)
        assert c_R.shape == (rc.G, R)
        for r in range(R):
            col = dO_R[:, r].contiguous()
            assert torch.equal(rc.bits(c_R[:, r]),
                               rc.bits(ops.scatter_dO(genes, offs, col, rc.G)))
            if exact:
                assert ke.bitwise_equal(
                    c_R[:, r], rc.scatter_ref64(genes, offs, col, rc.G))


def test_scatter_rep_slab_plan():
    genes, offs = rc.slab_pathset()
    plan = ops.build_scatter_plan(genes, offs, rc.G, _force_slabs=True)
    assert plan.slab_seg_ptr is not None and len(plan.slab_seg_ptr) == 3
    dO_R = rc.dO_table(rc.SLAB_R, exact=True, n_paths=rc.SLAB_P)
    c_R = ops.scatter_dO_rep(plan, dO_R, rc.G)
    for r in range(rc.SLAB_R):
        col = dO_R[:, r].contiguous()
        assert ke.bitwise_equal(c_R[:, r],
                                rc.scatter_ref64(genes, offs, col, rc.G))


@pytest.mark.parametrize("h", (64, 128))
@pytest.mark.parametrize("R", RS)
def test_adam_tail_and_gemv_rep_equal_single_per_replica(R, h):
    state0 = rc.adam_case(R, h)
    c_steps = state0[6]
    state = tuple(t.clone() for t in state0[:6])
    W, m, v, who, mO, vO = state
    for t, c_R in enumerate(c_steps, start=1):
        ops.adam_rank1_rep(W, m, v, c_R, who, mO, vO, t, rc.ADAM_LR,
                           rc.ADAM_B1, rc.ADAM_B2, rc.ADAM_EPS)
    s_R = torch.empty(rc.G, R)
    ops.gemv_rows_rep_(W, who, s_R)
    for r in range(R):
        ref = rc.adam_single_chain(state0[:6], c_steps, r, CPU)
        for got, want in zip(state, ref):
            assert torch.equal(rc.bits(got[r]), rc.bits(want))
        out = torch.empty(rc.G)
        ops.gemv_rows(ref[0], ref[3], out)
        assert torch.equal(rc.bits(s_R[:, r]), rc.bits(out))


def test_rep_ops_reject_bad_R():
    genes, offs, labels = rc.pathset()
    with pytest.raises(ValueError, match="R must be in"):
        ops.cbow_eval_counts_rep_(torch.zeros(rc.G, 33), genes, offs, labels,
                                  0, torch.zeros(33, 2))
    with pytest.raises(ValueError, match="R must be in"):
        ops.gemv_rows_rep_(torch.zeros(0, 4, 64), torch.zeros(0, 64),
                           torch.zeros(4, 0))


# =============================================================== trainer
def _cfg(**kw):
    base = dict(hidden=64, epochs=6, early_stop=False, seed=3, device="cpu")
    base.update(kw)
    return G2VecConfig(**base)


@pytest.mark.parametrize("R", RS)
def test_trainer_six_epochs_bitwise_per_replica(R):
    ps = rc.trainer_pathset(CPU)
    cfg = _cfg()
    rt = ReplicaTrainer(cfg, rc.G, CPU, log=lambda *a, **k: None)
    st = rt.setup(ps, R)
    hist = [rt.run_epoch(st) for _ in range(6)]
    for r in range(R):
        tr, s1 = rc.single_state(cfg, ps, CPU, r)
        ref = [tr.run_epoch(s1) for _ in range(6)]
        assert [(a[r], v[r]) for a, v in hist] == ref
        assert torch.equal(rc.bits(st.W[r]), rc.bits(s1.W))
        assert torch.equal(rc.bits(st.who[r]), rc.bits(s1.who))


EARLY_SEED = 23     # CPU single-run stop epochs of replicas 0..2: 7, 2, 6


@pytest.mark.parametrize("R", RS)
def test_trainer_early_stop_per_replica(R):
    ps = rc.trainer_pathset(CPU)
    cfg = _cfg(epochs=60, early_stop=True, seed=EARLY_SEED)
    res = ReplicaTrainer(cfg, rc.G, CPU, log=lambda *a, **k: None).train(ps, R)
    assert len(res) == R
    refs = []
    for r in range(R):
        tr, s1 = rc.single_state(cfg, ps, CPU, r)
        refs.append(rc.single_sync_run(tr, s1, cfg.epochs, True))
    print("stop epochs", [ref["stop_epoch"] for ref in refs])
    if R > 1:       # a frozen snapshot next to a still-training replica
        stops = [ref["stop_epoch"] for ref in refs]
        assert any(0 <= s < cfg.epochs - 2 for s in stops)
        assert len(set(stops)) > 1
    for r, ref in enumerate(refs):
        assert res[r].stop_epoch == ref["stop_epoch"]
        assert res[r].acc_val == ref["acc_val"]
        assert res[r].acc_tr == ref["acc_tr"]
        assert res[r].acc_val_history == ref["hist"]
        assert torch.equal(rc.bits(res[r].W_ih), rc.bits(ref["W_ih"]))


def test_trainer_relabel_is_undone_per_replica():
    """gene_relabel=on: replica r > 0 still is the plain run with seed + r."""
    ps = rc.trainer_pathset(CPU)
    cfg = _cfg(epochs=3, gene_relabel="on")
    res = ReplicaTrainer(cfg, rc.G, CPU, log=lambda *a, **k: None).train(ps, 2)
    for r in range(2):
        tr, s1 = rc.single_state(cfg, ps, CPU, r)
        assert tr.gene_order is not None
        ref = rc.single_sync_run(tr, s1, 3, False)
        assert torch.equal(rc.bits(res[r].W_ih), rc.bits(ref["W_ih"]))


def test_replica0_is_the_single_train_run_and_transcript_stops():
    """R = 3 on the runner-equivalence Fixture A: replica 0's TrainResult is
    the single train() result field for field (timings aside), and the
    transcript's per-replica lines carry the stop epochs of three single
    runs with seeds 1, 2, 3."""
    import dataclasses
    import re

    import runner_cases as rcase
    from g2vec_amd.models.cbow import CbowTrainer
    ps, cfg = rcase.fixture("A", early_stop=True)
    lines = []
    res = ReplicaTrainer(cfg, ps.n_genes, CPU, log=lines.append).train(ps, 3)
    single = CbowTrainer(cfg, ps.n_genes, CPU, log=rcase.quiet).train(ps)
    assert single.stop_epoch >= 8
    # "the single run with seed + r" is what the replica trainer means by
    # it: replicas share seed 1's split and differ in the weight seed only
    # (a train() with seed 2 would also reshuffle the split)
    singles = [rc.single_sync_run(*rc.single_state(cfg, ps, CPU, r),
                                  cfg.epochs, True) for r in range(3)]
    assert singles[0]["stop_epoch"] == single.stop_epoch
    for f in dataclasses.fields(single):
        got, want = getattr(res[0], f.name), getattr(single, f.name)
        if f.name == "W_ih":
            assert torch.equal(got, want)
        elif f.name == "epoch_times_s":
            assert len(got) == len(want) == res[0].epochs_run
        elif f.name == "wall_to_acc_s":
            assert (got is None) == (want is None)
        else:
            assert got == want, f.name
    stops = [int(m.group(2)) for m in
             (re.search(r"- Replica (\d\d): Epoch\(stop\): (-?\d+)\t", ln)
              for ln in lines) if m]
    assert stops == [s["stop_epoch"] for s in singles]
    assert lines[0] == ("     Start training 3 replicates of the modified "
                        "CBOW with early stopping")
    assert re.fullmatch(r"    Optimization Finish \(\d+\.\d{3} sec\)",
                        lines[-1])
    for r in range(3):
        assert lines[1 + r] == (
            "    - Replica %02d: Epoch(stop): %03d\tACC[val]=%.4f"
            "\tACC[tr]=%.4f" % (r, singles[r]["stop_epoch"],
                                singles[r]["acc_val"], singles[r]["acc_tr"]))


def test_synth_pathset_shape():
    """The benchmark's path sets: ids in range, distinct within a path,
    lengths in [1, len_path], seeded."""
    from g2vec_amd.utils.synth import synth_pathset
    genes, offs, labels = synth_pathset(1000, 500, n_modules=4, len_path=80,
                                        seed=5)
    again = synth_pathset(1000, 500, n_modules=4, len_path=80, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip((genes, offs, labels),
                                                    again))
    lens = np.diff(offs)
    assert offs[0] == 0 and lens.min() >= 1 and lens.max() <= 80
    assert genes.min() >= 0 and genes.max() < 1000 and len(genes) == offs[-1]
    assert set(np.unique(labels)) <= {0.0, 1.0}
    for p in range(500):
        row = genes[offs[p]:offs[p + 1]]
        assert len(set(row.tolist())) == len(row)


# ============================================================= stability
def test_stability_summarize_hand_written():
    # 4 replicas, 6 genes
    lg = np.array([[0, 1, 2, 0, 1, 2],
                   [0, 1, 2, 1, 1, 0],
                   [1, 1, 2, 0, 0, 0],
                   [1, 0, 2, 1, 0, 1]])
    # gene 0: 0,0,1,1 -> tie, mode 0; gene 2: never in L-group 0/1 -> NA
    # gene 3: 0,1,0,1 -> tie, mode 0; gene 4: 1,1,0,0 -> tie, mode 0
    # gene 5: 2,0,0,1 -> mode 0
    sel = np.array([[1, 1, 0, 1, 0, 0],
                    [1, 0, 0, 1, 1, 0],
                    [1, 1, 0, 0, 1, 0],
                    [0, 0, 0, 0, 1, 1]], dtype=bool)
    nan = np.nan
    # binary fractions: every mean below is exact
    gs = np.array([[0.50, 1.00, nan, 0.25, 0.25, nan],
                   [0.75, 0.75, nan, 0.25, 0.75, 0.125],
                   [0.50, 0.75, nan, 0.25, 0.50, 0.25],
                   [0.25, 0.50, nan, 0.25, 0.50, 0.375]])
    out = stability.summarize(lg, sel, gs, 3)
    assert out["lgroup"].tolist() == [0, 1, 2, 0, 1, 2]
    assert out["lgroup_mode"].tolist() == [0, 1, 2, 0, 0, 0]
    assert out["lgroup_agreement"].tolist() == [0.5, 0.75, 1.0, 0.5, 0.5, 0.5]
    assert out["selected"].tolist() == [3, 2, 0, 2, 3, 1]
    assert out["frequency"].tolist() == [0.75, 0.5, 0.0, 0.5, 0.75, 0.25]
    mgs = out["mean_gene_score"]
    assert np.isnan(mgs[2])
    assert np.delete(mgs, 2).tolist() == [0.5, 0.75, 0.25, 0.5, 0.25]
    # Selected 3: genes 0 and 4, both mean 0.5 -> lower index first; then
    # Selected 2: gene 1 (0.75) ahead of gene 3 (0.25)
    assert out["consensus"].tolist() == [0, 4, 1]
    assert stability.summarize(lg, sel, gs, 6)["consensus"].tolist() == \
        [0, 4, 1, 3, 5, 2]
    # NA sorts behind every defined score at equal Selected
    sel2 = sel.copy()
    sel2[:, 2] = sel[:, 5]
    assert stability.summarize(lg, sel2, gs, 6)["consensus"].tolist() == \
        [0, 4, 1, 3, 5, 2]
    # pairs of {0,1,3},{0,3,4},{0,1,4},{4,5}: 2/4, 2/4, 0/5, 2/4, 1/4, 1/4
    assert out["jaccard"] == pytest.approx((0.5 + 0.5 + 0 + 0.5 + 0.25 + 0.25)
                                           / 6)


# ================================================================ config
@pytest.mark.parametrize("kw, name", [
    (dict(trainer_path="general"), "trainer_path"),
    (dict(batch_size=64), "batch_size"),
    (dict(trainer_path="general", dtype="bf16"), "trainer_path"),
    (dict(earlystop_every=4), "earlystop_every"),
    (dict(train_ckpt="ck.pt"), "train_ckpt"),
    (dict(resume_train="ck.pt"), "resume_train"),
    (dict(load_model="m.pt"), "load_model"),
])
def test_validate_rejects_out_of_scope_by_name(kw, name):
    G2VecConfig(**kw).validate()                     # fine without the flag
    with pytest.raises(ValueError, match="conflicts with " + name):
        G2VecConfig(replicates=2, **kw).validate()


def test_validate_scope_names_dtype_and_activation():
    # validate() itself already ties these two to the general chain, so the
    # scope check is reached directly
    for kw, name in ((dict(dtype="bf16"), "dtype"),
                     (dict(activation="relu"), "activation")):
        cfg = G2VecConfig(replicates=2, **kw)
        with pytest.raises(ValueError, match="conflicts with " + name):
            cfg.check_replicate_scope()


@pytest.mark.parametrize("R", (0, 33, -1))
def test_validate_rejects_replicates_out_of_range(R):
    with pytest.raises(ValueError, match="replicates must be in"):
        G2VecConfig(replicates=R).validate()


def test_default_config_repr_unchanged_by_the_flag():
    assert "replicates" not in repr(G2VecConfig())
    G2VecConfig(replicates=32).validate()


# =================================================================== CLI
STANDARD = ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt", "_scores.txt",
            "_neighbors.txt")


def _cli(tiny_files, out, *extra):
    from g2vec_amd.cli import main
    argv = [tiny_files["expression"], tiny_files["clinical"],
            tiny_files["network"], str(out), "-p", "15", "-r", "3", "-e", "25",
            "-s", "64", "-n", "10", "--seed", "0", "--device", "cpu",
            "--write-scores", "--neighbors", "3"] + list(extra)
    assert main(argv) == 0


def test_cli_replicates_end_to_end(tiny_files, tmp_path, capsys):
    _cli(tiny_files, tmp_path / "plain")
    _cli(tiny_files, tmp_path / "rep", "--replicates", "3")
    transcript = capsys.readouterr().out
    _cli(tiny_files, tmp_path / "rep2", "--replicates", "3")
    for sfx in STANDARD:
        plain = (tmp_path / f"plain{sfx}").read_bytes()
        assert (tmp_path / f"rep{sfx}").read_bytes() == plain, sfx
    assert not (tmp_path / "plain_stability.txt").exists()
    for sfx in ("_stability.txt", "_consensus_biomarkers.txt"):
        assert (tmp_path / f"rep{sfx}").read_bytes() == \
            (tmp_path / f"rep2{sfx}").read_bytes()
    for r in range(3):
        assert "- Replica %02d: Epoch(stop):" % r in transcript

    genes = [ln.split("\t")[0] for ln in
             (tmp_path / "rep_lgroups.txt").read_text().splitlines()[1:]]
    rows = [ln.split("\t") for ln in
            (tmp_path / "rep_stability.txt").read_text().splitlines()]
    assert rows[0] == ["GeneSymbol", "Lgroup", "LgroupMode",
                       "LgroupAgreement", "Selected", "Frequency",
                       "MeanGeneScore"]
    assert [row[0] for row in rows[1:]] == genes
    for row in rows[1:]:
        assert 0 <= int(row[4]) <= 3
        assert row[5] == "%.4f" % (int(row[4]) / 3)
    bio = set((tmp_path / "rep_biomarkers.txt").read_text().split()[1:])
    assert all(int(row[4]) >= 1 for row in rows[1:] if row[0] in bio)
    cons = (tmp_path / "rep_consensus_biomarkers.txt").read_text().splitlines()
    assert cons[0] == "GeneSymbol" and len(cons) == 1 + 10
    assert len(set(cons[1:])) == 10 and set(cons[1:]) <= set(genes)


def test_jsonl_replicates_record(tiny_files, tmp_path):
    import json
    log = tmp_path / "m.jsonl"
    _cli(tiny_files, tmp_path / "o", "--replicates", "2", "--log-jsonl",
         str(log))
    recs = [json.loads(ln) for ln in log.read_text().splitlines()]
    rep = [r for r in recs if r["event"] == "replicates"]
    assert len(rep) == 1 and rep[0]["R"] == 2
    assert len(rep[0]["stop_epochs"]) == 2 and len(rep[0]["acc_val"]) == 2
    assert 0.0 <= rep[0]["jaccard"] <= 1.0 and rep[0]["seconds"] > 0
