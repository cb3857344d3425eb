"""Permutation null of the gene t-scores on the CPU: the cpu_ref mirrors
against the independent fp64 reference of perm_cases, the mask generator,
the host p-value arithmetic, the guards, the writer and the pipeline."""
import numpy as np
import pytest
import torch

import kernel_edges as ke
import perm_cases as pc
from g2vec_amd import ops, scoring
from g2vec_amd.config import G2VecConfig
from g2vec_amd.ops import cpu_ref


# ------------------------------------------------------------- the mirror
@pytest.mark.parametrize("S,G,B,balanced", pc.EXACT_CASES)
def test_exact_fixtures(S, G, B, balanced):
    pc.check_exact(ops, pc.exact_case(S, G, B, balanced), "cpu")


def test_exact_fixture_cross_covers_every_edge():
    shapes = pc.EXACT_SHAPES
    assert {s for s, _, _ in shapes} >= set(pc.EXACT_S)
    assert {g for _, g, _ in shapes} >= set(pc.EXACT_G)
    assert {b for _, _, b in shapes} >= set(pc.EXACT_B)
    assert (max(pc.EXACT_S), max(pc.EXACT_G), max(pc.EXACT_B)) in shapes


@pytest.mark.parametrize("S,G", pc.REAL_SHAPES)
def test_real_fixtures(S, G):
    pc.check_real(ops, pc.real_case(S, G), "cpu")


def test_col_moments_mirror():
    case = pc.exact_case(135, 65, 65, False)
    T, Q = ops.col_moments(torch.from_numpy(case["expr"]))
    x = case["expr"].astype(np.float64)
    assert T.dtype == torch.float64 and Q.dtype == torch.float64
    assert np.array_equal(T.numpy(), x.sum(axis=0))
    assert np.array_equal(Q.numpy(), (x * x).sum(axis=0))


def test_row_permutation_and_repeat():
    pc.check_row_permutation(ops, pc.exact_case(65, 65, 65, True), "cpu")
    pc.check_row_permutation(ops, pc.real_case(65, 64), "cpu")


def test_chunk_invariance():
    pc.check_chunk_invariance(pc.real_case(65, 64), "cpu")


# ------------------------------------------------------------------ masks
def test_splitmix64_vec_equals_scalar():
    rng = np.random.default_rng(0)
    states = rng.integers(0, 2 ** 63, size=64, dtype=np.uint64) * np.uint64(2) \
        + np.uint64(1)
    states[:3] = [0, 2 ** 64 - 1, 0x9E3779B97F4A7C15]
    ns, z = cpu_ref.splitmix64_vec(states)
    assert ns.dtype == np.uint64 and z.dtype == np.uint64
    for i, s in enumerate(states):
        s1, z1 = cpu_ref.splitmix64(np.uint64(s))
        assert int(ns[i]) == int(s1) and int(z[i]) == int(z1)
    # shape is kept
    ns2, z2 = cpu_ref.splitmix64_vec(states.reshape(8, 8))
    assert np.array_equal(z2.ravel(), z)


def test_perm_masks_rows():
    labels = np.array([0] * 50 + [1] * 30)
    m = scoring.perm_masks(labels, 300, seed=5)
    assert m.dtype == np.uint8 and m.shape == (300, 80)
    assert set(np.unique(m)) == {0, 1}
    assert (m.sum(axis=1) == 30).all()
    # each (seed, b) row is reproducible, whatever B it is drawn under
    assert np.array_equal(scoring.perm_masks(labels, 300, seed=5), m)
    assert np.array_equal(scoring.perm_masks(labels, 7, seed=5), m[:7])
    assert len({r.tobytes() for r in m}) == 300
    other = scoring.perm_masks(labels, 300, seed=6)
    assert not np.array_equal(other, m)
    with pytest.raises(ValueError):
        scoring.perm_masks(labels, 0, seed=5)


def test_perm_masks_key_is_the_scalar_stream():
    """Row b marks the n1 smallest keys; key (b, s) is the second draw of
    the scalar splitmix64 stream seeded seed ^ (((b << 32) | s) * M2 + 1)."""
    labels = np.array([1, 0, 0, 1, 0, 1, 0])
    seed, b = 9, 3
    keys = []
    with np.errstate(over="ignore"):
        for s in range(len(labels)):
            gid = np.uint64((b << 32) | s)
            st = np.uint64(seed) ^ np.uint64(gid * cpu_ref._SM64_M2
                                             + np.uint64(1))
            st, _ = cpu_ref.splitmix64(st)
            _, k = cpu_ref.splitmix64(st)
            keys.append(int(k))
    want = np.zeros(len(labels), dtype=np.uint8)
    want[np.argsort(np.array(keys, dtype=np.uint64), kind="stable")[:3]] = 1
    assert np.array_equal(scoring.perm_masks(labels, b + 1, seed)[b], want)


def test_perm_masks_label_frequencies():
    S, n1, N = 40, 15, 4000
    labels = np.array([1] * n1 + [0] * (S - n1))
    m = scoring.perm_masks(labels, N, seed=1)
    p = n1 / S
    obs = m.sum(axis=0).astype(np.float64)
    # row sums are fixed, so the S counts are exchangeable with covariance
    # -N p (1-p) / (S-1): this statistic is chi-square with S - 1 df
    chi2 = float(((obs - N * p) ** 2).sum() / (N * p * (1 - p))
                 * (S - 1) / S)
    limit = ke.chi2_upper_quantile(S - 1)
    print("chi2", chi2, "limit", limit)
    assert chi2 < limit


# ----------------------------------------------------------------- guards
def _guard_inputs():
    case = pc.exact_case(65, 65, 17, True)
    return (torch.from_numpy(case["expr"]), torch.from_numpy(case["masks"]),
            torch.from_numpy(case["stat_obs"]))


def test_guards_refuse():
    expr, masks, so = _guard_inputs()
    bad = [
        (expr.double(), masks, so),                         # dtype
        (expr, masks.int(), so),
        (expr, masks, so.float()),
        (expr.t().contiguous().t(), masks, so),             # contiguity
        (expr, masks.t().contiguous().t(), so),
        (expr, masks[:, :-1].contiguous(), so),             # S mismatch
        (expr[:3].contiguous(), masks[:, :3].contiguous(), so),   # S = 3
        (expr, masks, so[:-1].contiguous()),                # stat_obs shape
    ]
    for e, m, s in bad:
        with pytest.raises(ValueError):
            ops.perm_t_counts(e, m, s)
        if s is so:
            with pytest.raises(ValueError):
                ops.perm_t_stats(e, m)
    uneven = masks.clone()
    uneven[3, int(torch.nonzero(uneven[3] == 0)[0])] = 1    # unequal n1
    with pytest.raises(ValueError):
        ops.perm_t_stats(expr, uneven)
    one = torch.zeros(2, expr.shape[0], dtype=torch.uint8)
    one[:, 0] = 1                                           # a group of one
    with pytest.raises(ValueError):
        ops.perm_t_stats(expr, one)
    with pytest.raises(ValueError):
        ops.perm_t_stats(expr, (1 - one).contiguous())
    two = masks.clone()
    two[0, int(torch.nonzero(two[0] == 1)[0])] = 2          # not 0/1
    with pytest.raises(ValueError):
        ops.perm_t_stats(expr, two)


# --------------------------------------------------- p-value arithmetic
def test_bh_hand_example():
    p = np.array([0.005, 0.04, 0.03, 0.9, 0.035])
    # sorted 0.005 0.03 0.035 0.04 0.9 -> p*5/rank = 0.025 0.075 0.0583 0.05
    # 0.9; the running minimum from the top pulls ranks 2-3 down to 0.05
    want = np.array([0.025, 0.05, 0.05, 0.9, 0.05])
    np.testing.assert_allclose(scoring.bh_adjust(p), want, rtol=1e-15)
    assert scoring.bh_adjust(np.array([0.5, 1.0]))[1] == 1.0
    assert scoring.bh_adjust(np.array([])).shape == (0,)


def test_permutation_pvalues_rejects_b0():
    expr, labels = pc.planted_case()
    with pytest.raises(ValueError):
        scoring.permutation_pvalues(expr, labels, 0, seed=1, device="cpu")


def test_planted_signal():
    pc.check_planted("cpu")


def test_centring_makes_p_shift_invariant():
    expr, labels = pc.planted_case()
    a = scoring.permutation_pvalues(expr[:, :20].astype(np.float64), labels,
                                    100, seed=2)
    b = scoring.permutation_pvalues(expr[:, :20].astype(np.float64) + 1000.0,
                                    labels, 100, seed=2)
    assert np.array_equal(a["counts"], b["counts"])


# ------------------------------------------------- config, writer, pipeline
def test_config_fields():
    cfg = G2VecConfig()
    assert cfg.permutations == 0 and not cfg.write_scores
    assert cfg.perm_seed is None
    cfg = G2VecConfig(permutations=10)
    cfg.validate()
    assert cfg.write_scores
    with pytest.raises(ValueError):
        G2VecConfig(permutations=-1).validate()
    with pytest.raises(ValueError):
        G2VecConfig(perm_seed=-2).validate()


def test_cli_flags():
    from g2vec_amd.cli import args_to_config, build_parser
    base = ["e", "c", "n", "o"]
    cfg = args_to_config(build_parser().parse_args(base))
    assert cfg.permutations == 0 and not cfg.write_scores
    cfg = args_to_config(build_parser().parse_args(base + ["--write-scores"]))
    assert cfg.write_scores and cfg.permutations == 0
    cfg = args_to_config(build_parser().parse_args(
        base + ["--permutations", "100", "--perm-seed", "7"]))
    assert cfg.write_scores and cfg.permutations == 100
    assert cfg.perm_seed == 7


def test_score_genes_matches_select_biomarkers():
    import steps56_cases as sc
    emb, lg, expr, labels, genes = sc.biomarker_case()
    names = scoring.select_biomarkers(emb, lg, expr, labels, genes, 5)
    r = scoring.score_genes(emb, lg, expr, labels, genes, 5)
    assert r["biomarkers"] == names
    assert sorted(np.asarray(genes)[r["is_biomarker"]].tolist()) == names
    assert np.array_equal(np.isnan(r["gene_score"]), lg == 2)
    np.testing.assert_allclose(r["d_score"], np.linalg.norm(emb, axis=1),
                               rtol=1e-6)
    np.testing.assert_allclose(r["t_score"], scoring.t_scores(expr, labels),
                               rtol=1e-6)
    for grp in (0, 1):
        s = r["gene_score"][lg == grp]
        assert s.min() >= 0.0 and s.max() <= 1.0


def test_write_scores_format(tmp_path):
    from g2vec_amd import io as gio
    scores = {"d_score": np.array([1.5, 2.25, 0.0]),
              "t_score": np.array([0.1234567, 3.0, 1.0]),
              "gene_score": np.array([0.5, np.nan, 1.0]),
              "is_biomarker": np.array([True, False, False])}
    perm = {"p": np.array([1 / 3, 1.0, 0.001]),
            "q_bh": np.array([0.5, 1.0, 0.003]),
            "p_maxT": np.array([0.75, 1.0, 1e-5])}
    name = str(tmp_path / "w")
    out = gio.write_scores(name, ["A", "B", "C"], [0, 2, 1], scores, perm)
    assert out == name + "_scores.txt"
    assert open(out).read() == (
        "GeneSymbol\tLgroup\td_score\tt_score\tgene_score\tbiomarker\t"
        "p_perm\tq_bh\tp_maxT\n"
        "A\t0\t1.500000\t0.123457\t0.500000\t1\t0.333333\t0.5\t0.75\n"
        "B\t2\t2.250000\t3.000000\tNA\t0\t1\t1\t1\n"
        "C\t1\t0.000000\t1.000000\t1.000000\t0\t0.001\t0.003\t1e-05\n")
    gio.write_scores(name, ["A", "B", "C"], [0, 2, 1], scores)
    assert open(out).readline() == \
        "GeneSymbol\tLgroup\td_score\tt_score\tgene_score\tbiomarker\n"


def test_pipeline_scores_table(tiny_files, tmp_path):
    pc.check_pipeline(tiny_files, tmp_path, "cpu")


def test_pipeline_write_scores_without_permutations(tiny_files, tmp_path):
    from g2vec_amd.pipeline import run
    cfg = G2VecConfig(expression_file=tiny_files["expression"],
                      clinical_file=tiny_files["clinical"],
                      network_file=tiny_files["network"],
                      result_name=str(tmp_path / "s"), len_path=15,
                      num_repetition=3, epochs=25, device="cpu", seed=0,
                      write_scores=True)
    res = run(cfg)
    lines = (tmp_path / "s_scores.txt").read_text().splitlines()
    assert lines[0].split("\t") == pc.SCORE_COLS
    assert len(lines) == 1 + res["n_genes"]
