"""Rank statistics on the CPU: the cpu_ref mirrors of rank_columns /
ranksum_scores and the host scoring.ranksum_scores against the counting
reference of rank_cases.py and against SciPy, the Spearman graph, the
rank-based permutation null, and the config / CLI / pipeline surface."""
import dataclasses

import numpy as np
import pytest
import torch

import rank_cases as rc
from g2vec_amd import ops, scoring
from g2vec_amd.config import G2VecConfig
from g2vec_amd.ops import cpu_ref

DEV = "cpu"


# ------------------------------------------------- mirror against references
@pytest.mark.parametrize("S,G", rc.SHAPES)
def test_ranks_equal_counting_reference(S, G):
    rc.check_ranks(S, G, DEV)


@pytest.mark.parametrize("S,G,balanced", rc.CASES)
def test_ranksum_within_one_ulp_of_host(S, G, balanced):
    rc.check_ranksum(S, G, balanced, DEV)


@pytest.mark.parametrize("S,G,balanced", [c for c in rc.CASES
                                          if c[1] != rc.CAP_G])
def test_integer_sums_are_exact(S, G, balanced):
    case = rc.ranksum_case(S, G, balanced)
    w2, q4 = cpu_ref.ranksum_sums(rc.tensor(case["expr"]),
                                  rc.tensor(case["labels"]))
    assert w2.dtype == np.int64 and q4.dtype == np.int64
    assert np.array_equal(w2, case["w2"]) and np.array_equal(q4, case["q4"])
    assert np.array_equal(cpu_ref.rank2_columns(case["expr"]),
                          rc.ref_rank2(case["expr"]))


def test_repeatable():
    rc.check_repeatable(DEV)


def test_wrapper_refuses_bad_input():
    x = torch.from_numpy(rc.values(5, 3).copy())
    bad = x.clone()
    bad[2, 1] = float("nan")
    lab = torch.tensor([0, 1, 0, 1, 1])
    with pytest.raises(ValueError):
        ops.rank_columns(bad)
    with pytest.raises(ValueError):
        ops.ranksum_scores(bad, lab)
    with pytest.raises(ValueError):
        ops.rank_columns(x.double())
    with pytest.raises(ValueError):
        ops.rank_columns(x.t())
    with pytest.raises(ValueError):
        ops.rank_columns(x[:0])
    with pytest.raises(ValueError):
        ops.ranksum_scores(x, lab[:-1])
    with pytest.raises(ValueError):
        ops.ranksum_scores(x, lab.float())


def test_tile_constants_are_exported():
    assert (ops.RANK_TG, ops.RANK_WAVES) == (64, 4)
    assert ops.RANK_SJ >= 2 and ops.RANK_IB >= 1 and ops.RANK_MAX_BLOCKS >= 1


# ------------------------------------------------------- SciPy cross-checks
def _scipy_case():
    rng = np.random.default_rng(31)
    S, G = 57, 24
    x = rng.integers(0, 5, size=(S, G)).astype(np.float32)
    x[:, 1::3] = rng.normal(size=(S, len(range(1, G, 3))))
    lab = np.zeros(S, dtype=np.int64)
    lab[rng.choice(S, size=23, replace=False)] = 1
    return x, lab


def test_ranks_equal_scipy_rankdata():
    stats = pytest.importorskip("scipy.stats")
    for S, G in ((65, rc.TG + 1), (135, 130)):
        x = rc.values(S, G)
        want = stats.rankdata(x.astype(np.float64), method="average", axis=0)
        got = ops.rank_columns(rc.tensor(x)).numpy()
        assert np.array_equal(got.astype(np.float64), want)
        assert np.array_equal(scoring.average_ranks(x), want)


def test_ranksum_equals_scipy_mannwhitneyu():
    stats = pytest.importorskip("scipy.stats")
    x, lab = _scipy_case()
    n1, n0 = int(lab.sum()), int((lab == 0).sum())
    w2, q4 = cpu_ref.ranksum_sums(torch.from_numpy(x), torch.from_numpy(lab))
    z, auc = cpu_ref.ranksum_from_sums(w2, q4, n1, x.shape[0])      # fp64
    _, _, z_ref, auc_ref = rc.ref_ranksum(x, lab)
    for g in range(x.shape[1]):
        res = stats.mannwhitneyu(x[lab == 1, g].astype(np.float64),
                                 x[lab == 0, g].astype(np.float64),
                                 use_continuity=False, method="asymptotic")
        assert auc[g] == res.statistic / (n1 * n0)
        assert auc_ref[g] == auc[g]
        np.testing.assert_allclose(2.0 * stats.norm.sf(z[g]), res.pvalue,
                                   rtol=1e-12)
        np.testing.assert_allclose(2.0 * stats.norm.sf(z_ref[g]), res.pvalue,
                                   rtol=1e-12)


# ----------------------------------------------------------------- Spearman
@pytest.mark.parametrize("mode", ["edge", "gemm"])
def test_spearman_graph_is_pearson_graph_of_ranks(mode):
    rc.check_spearman_is_pearson_of_ranks(DEV, mode)


def test_spearman_graph_invariant_under_monotone_map():
    x, labels, edges = rc.graph_inputs()
    y = (x.astype(np.float64) ** 3 + x).astype(np.float32)
    # exact and strictly monotone on the k/8 grid
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) ** 3 + x)
    changed = False
    for group in (0, 1):
        a = rc.build(x, labels, edges, group, DEV, "spearman")
        b = rc.build(y, labels, edges, group, DEV, "spearman")
        assert a.col_idx.numel() > 0 and rc.same_graph(a, b)
        pa = rc.build(x, labels, edges, group, DEV, "pearson")
        pb = rc.build(y, labels, edges, group, DEV, "pearson")
        changed |= not rc.same_graph(pa, pb)
    assert changed


def test_outlier_makes_a_pearson_edge_but_no_spearman_edge():
    rng = np.random.default_rng(8)
    S = 40
    labels = np.array([0, 1] * (S // 2), dtype=np.int64)
    x = rng.normal(size=(S, 2)).astype(np.float32)
    rows0 = np.flatnonzero(labels == 0)
    r_clean = np.corrcoef(x[rows0, 0], x[rows0, 1])[0, 1]
    assert abs(r_clean) < 0.3                      # no edge before planting
    x[rows0[5]] = (60.0, 60.0)                     # one extreme sample
    edges = np.array([[0, 1]], dtype=np.int64)
    pe = rc.build(x, labels, edges, 0, DEV, "pearson")
    sp = rc.build(x, labels, edges, 0, DEV, "spearman")
    assert pe.col_idx.numel() == 1 and float(pe.weights[0]) > 0.9
    assert sp.col_idx.numel() == 0


def test_bad_corr_is_refused():
    x, labels, edges = rc.graph_inputs()
    with pytest.raises(ValueError):
        rc.build(x, labels, edges, 0, DEV, "kendall")


# -------------------------------------------------------------- permutation
def test_rank_permutation_counts_are_the_integer_counts():
    rc.check_perm_counts(DEV)


# ----------------------------------------------------------- config and CLI
def test_validate_refuses_bad_values():
    G2VecConfig(corr="spearman", score_stat="ranksum").validate()
    with pytest.raises(ValueError):
        G2VecConfig(corr="kendall").validate()
    with pytest.raises(ValueError):
        G2VecConfig(score_stat="auc").validate()
    with pytest.raises(ValueError):
        G2VecConfig(corr="spearman", load_paths="paths.pt").validate()
    G2VecConfig(corr="pearson", load_paths="paths.pt").validate()
    G2VecConfig(score_stat="ranksum", load_paths="paths.pt").validate()


def test_default_repr_unchanged_by_the_new_fields():
    base = G2VecConfig()
    assert base.corr == "pearson" and base.score_stat == "t"
    assert "corr" not in str(base) and "score_stat" not in str(base)
    other = dataclasses.replace(base, corr="spearman", score_stat="ranksum")
    assert str(other) == str(base)


def test_cli_flags():
    from g2vec_amd.cli import args_to_config, build_parser
    p = build_parser()
    cfg = args_to_config(p.parse_args(["e", "c", "n", "r"]))
    assert (cfg.corr, cfg.score_stat) == ("pearson", "t")
    cfg = args_to_config(p.parse_args(
        ["e", "c", "n", "r", "--corr", "spearman", "--score-stat", "ranksum"]))
    assert (cfg.corr, cfg.score_stat) == ("spearman", "ranksum")
    with pytest.raises(SystemExit):
        p.parse_args(["e", "c", "n", "r", "--corr", "kendall"])


def _cli_run(tiny_files, argv_extra, capsys):
    from g2vec_amd.cli import args_to_config, build_parser
    from g2vec_amd.pipeline import run
    argv = [tiny_files["expression"], tiny_files["clinical"],
            tiny_files["network"], "out", "-p", "15", "-r", "3", "-e", "25",
            "--device", DEV] + argv_extra
    run(args_to_config(build_parser().parse_args(argv)))
    return capsys.readouterr().out.splitlines()


def test_default_flags_leave_the_run_byte_identical(tiny_files, tmp_path,
                                                    monkeypatch, capsys):
    outs = {}
    for name, extra in (("p", []),
                        ("q", ["--corr", "pearson", "--score-stat", "t"])):
        (tmp_path / name).mkdir()
        monkeypatch.chdir(tmp_path / name)
        outs[name] = _cli_run(tiny_files, extra + ["--write-scores"], capsys)
    for suffix in ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt",
                   "_scores.txt"):
        assert (tmp_path / "p" / ("out" + suffix)).read_bytes() == \
            (tmp_path / "q" / ("out" + suffix)).read_bytes(), suffix
    head = (tmp_path / "p" / "out_scores.txt").read_text().splitlines()[0]
    assert head.split("\t")[3] == "t_score"
    p, q = outs["p"], outs["q"]
    at = p.index(">>> 0. Arguments")
    assert p[at + 1] == q[q.index(">>> 0. Arguments") + 1]
    assert not any("corr    :" in ln or "score   :" in ln for ln in p + q)


def test_rank_pipeline_scores_table(tiny_files, tmp_path, capsys):
    rc.check_rank_pipeline(tiny_files, tmp_path, DEV)
    out = capsys.readouterr().out.splitlines()
    assert out.count("    corr    : spearman") == 2       # once per run
    assert out.count("    score   : ranksum") == 2
