"""CPU mirrors and host glue of the device steps 5-6 (k-means L-groups,
d/t-scores): cpu_ref.kmeans_step / kmeans_mind2_ / row_norms / t_scores
against fp64 references written here and in steps56_cases.py,
cluster.kmeans_hip, select_biomarkers with precomputed scores, config and
CLI. No GPU needed; test_gpu_steps56.py runs the same cases on the kernels.

Tolerances: k-means inputs are dyadic, so everything is bitwise. t-scores
are f64 on both sides (about S roundings of 1e-16, far below the fp32
half-ulp 6e-8), so the fp32 results differ only where the f64 value sits on
a rounding boundary: 1 ulp. Row norms: 1 ulp of the f64 norm, and rtol 1e-6
against NumPy's pairwise f32 sum (about log2(h) * 6e-8 for h <= 1024)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kernel_edges as ke
import steps56_cases as sc
from g2vec_amd import cluster, ops, scoring
from g2vec_amd.config import G2VecConfig
from g2vec_amd.ops import cpu_ref


# ============================================================ kmeans_step
@pytest.mark.parametrize("k", sc.KM_K)
@pytest.mark.parametrize("G", [1, 5, 1003])
@pytest.mark.parametrize("h", [64, 1024])
def test_kmeans_step_mirror_exact(h, G, k):
    X, C, ref = sc.kmeans_case(G, h, k)
    prev = torch.zeros(G, dtype=torch.int32)
    out = sc.run_step(ops, X, C, prev)
    sc.assert_step_matches(out, C, ref, prev)


def test_kmeans_step_tie_lowest_index_and_empty_cluster_keeps_row():
    X, C, ref = sc.tie_case()
    labels = ref[1]
    assert int((labels == 0).sum()) > 0          # the tie is really taken
    assert int(ref[3][2]) == 0
    prev = torch.zeros(X.shape[0], dtype=torch.int32)
    out = sc.run_step(ops, X, C, prev)
    sc.assert_step_matches(out, C, ref, prev)
    assert int((out["labels"] == 2).sum()) == 0
    assert int(out["counts"][2]) == 0
    assert torch.equal(out["C_new"][2], C[2])
    assert torch.equal(out["sums"][2], torch.zeros(X.shape[1]))


@pytest.mark.parametrize("which", ["all", "none", "one"])
def test_kmeans_step_n_changed(which):
    X, C, ref = sc.kmeans_case(1003, 64, 3)
    labels = ref[1].int()
    prev = labels.clone()
    if which == "all":
        prev = (labels + 1) % 3
    elif which == "one":
        prev[517] = (prev[517] + 1) % 3
    out = sc.run_step(ops, X, C, prev)
    assert int(out["n_changed"][0]) == {"all": 1003, "none": 0, "one": 1}[which]


def test_kmeans_step_in_place_arguments():
    """prev may be labels and C_new may be C (how kmeans_hip steps)."""
    X, C, ref = sc.kmeans_case(1003, 64, 3)
    labels = torch.zeros(1003, dtype=torch.int32)
    Cw = C.clone()
    out = sc.step_outputs(X, C)
    ops.kmeans_step(X, Cw, labels, labels, Cw, out["sums"], out["counts"],
                    out["n_changed"], out["inertia"])
    assert torch.equal(labels.long(), ref[1])
    assert torch.equal(Cw, ref[5])
    assert int(out["n_changed"][0]) == int((ref[1] != 0).sum())


def test_kmeans_mind2_mirror_exact():
    X, C, ref = sc.kmeans_case(1003, 64, 3)
    D = ref[0]
    d2 = torch.full((1003,), float("inf"))
    ops.kmeans_mind2_(X, C[0].contiguous(), d2)
    assert ke.bitwise_equal(d2, D[:, 0])
    ops.kmeans_mind2_(X, C[1].contiguous(), d2)
    assert ke.bitwise_equal(d2, torch.minimum(D[:, 0], D[:, 1]))


# ============================================================= kmeans_hip
def _blobs_t():
    return torch.from_numpy(sc.blobs())


def test_find_lgroups_hip_equals_sklearn_on_blobs():
    emb, freq = sc.blobs(), sc.blob_freq()
    lg_sk = cluster.find_lgroups(emb, freq, backend="sklearn")
    info = {}
    lg_hip = cluster.find_lgroups(emb, freq, backend="hip", info=info)
    assert (lg_sk == lg_hip).all()
    assert info["kmeans_iterations"] >= 1 and info["kmeans_inertia"] > 0
    # a tensor is accepted for this backend, same answer
    lg_t = cluster.find_lgroups(_blobs_t(), freq, backend="hip")
    assert (lg_t == lg_hip).all()


def test_kmeans_hip_check_every_is_bitwise_invariant():
    X = _blobs_t()
    a = cluster.kmeans_hip(X, 3, seed=0, n_init=3, check_every=1)
    b = cluster.kmeans_hip(X, 3, seed=0, n_init=3, check_every=4)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3]


def test_kmeans_hip_same_seed_same_result_and_seed_matters():
    X = _blobs_t()
    a = cluster.kmeans_hip(X, 3, seed=5, n_init=2)
    b = cluster.kmeans_hip(X, 3, seed=5, n_init=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3]
    draws = {cluster._kpp_u01(s, r, d) for s in (0, 5) for r in (0, 1)
             for d in (0, 1, 2)}
    assert len(draws) == 12 and all(0.0 <= u < 1.0 for u in draws)


def test_kmeans_hip_more_restarts_never_worse():
    gen = torch.Generator().manual_seed(3)
    X = torch.randn(400, 64, generator=gen)      # no structure: local optima
    one = cluster.kmeans_hip(X, 3, seed=0, n_init=1)
    ten = cluster.kmeans_hip(X, 3, seed=0, n_init=10)
    assert ten[2] <= one[2]


def test_kmeans_hip_reaches_a_fixed_point_and_reports_true_inertia():
    X = _blobs_t()
    labels, C, inertia, n_iter = cluster.kmeans_hip(X, 3, seed=0, n_init=1)
    assert 1 <= n_iter < 300
    d = ((X.double()[:, None, :] - C.double()[None]) ** 2).sum(-1)
    assert torch.equal(d.argmin(dim=1).int(), labels)
    assert float(d.min(dim=1).values.sum()) == pytest.approx(inertia,
                                                            rel=1e-5)
    assert sorted(torch.bincount(labels.long()).tolist()) == [20, 30, 100]


def test_kmeans_hip_rejects_bad_arguments():
    X = _blobs_t()
    with pytest.raises(ValueError, match="k must be"):
        cluster.kmeans_hip(X, 9)
    with pytest.raises(ValueError, match="exceeds"):
        cluster.kmeans_hip(torch.zeros(4, 1025), 2)
    with pytest.raises(ValueError, match=">= 1"):
        cluster.kmeans_hip(X, 3, check_every=0)


# =============================================================== t_scores
@pytest.mark.parametrize("S", sc.T_S)
def test_t_scores_mirror_within_one_ulp_of_host(S):
    for n_good in (2, S // 2):
        expr, labels, host = sc.t_case(S, n_good=n_good)
        got = ops.t_scores(expr, labels).numpy()
        assert got.dtype == np.float32 and got.shape == host.shape
        assert sc.ulp_diff_f32(got, host) <= 1
        assert got[0] == 0.0 and got[1] == 0.0   # constant / d1 == 0 columns
        assert (got[2:] > 0).any()


def test_t_scores_group_of_one_is_all_zeros():
    expr, labels, host = sc.t_case(64, n_good=1)
    got = ops.t_scores(expr, labels).numpy()
    assert (host == 0).all() and (got == 0).all()
    got32 = ops.t_scores(expr, labels.int()).numpy()      # i32 labels too
    assert (got32 == 0).all()


# ============================================================== row_norms
@pytest.mark.parametrize("h", [64, 1024])
def test_row_norms_mirror(h):
    W, ref64, ref_np = sc.norm_case(1003, h)
    sc.assert_norms_match(ops.row_norms(W).numpy(), ref64, ref_np)


# ====================================================== select_biomarkers
def test_select_biomarkers_with_precomputed_scores():
    emb, lg, expr, labels, genes = sc.biomarker_case(5)
    host = scoring.select_biomarkers(emb, lg, expr, labels, genes, 5)
    d_all = cpu_ref.row_norms(torch.from_numpy(emb)).numpy()
    t_all = cpu_ref.t_scores(torch.from_numpy(expr),
                             torch.from_numpy(labels)).numpy()
    dev = scoring.select_biomarkers(emb, lg, expr, labels, genes, 5,
                                    d_all=d_all, t_all=t_all)
    assert len(host) == 10 and dev == host
    # the precomputed vectors are really what is ranked
    flipped = scoring.select_biomarkers(emb, lg, expr, labels, genes, 5,
                                        d_all=-d_all, t_all=-t_all)
    assert flipped != host


# ========================================================= config and CLI
def test_config_accepts_and_rejects_backends():
    G2VecConfig(kmeans_backend="hip", scoring_backend="device").validate()
    assert G2VecConfig().scoring_backend == "host"
    assert G2VecConfig().kmeans_backend == "auto"
    with pytest.raises(ValueError, match="kmeans_backend"):
        G2VecConfig(kmeans_backend="rocm").validate()
    with pytest.raises(ValueError, match="scoring_backend"):
        G2VecConfig(scoring_backend="gpu").validate()


def test_cli_parses_new_flags(tiny_files, tmp_path):
    from g2vec_amd.cli import args_to_config, build_parser
    argv = [tiny_files["expression"], tiny_files["clinical"],
            tiny_files["network"], str(tmp_path / "o")]
    cfg = args_to_config(build_parser().parse_args(
        argv + ["--kmeans", "hip", "--scoring", "device"]))
    assert cfg.kmeans_backend == "hip" and cfg.scoring_backend == "device"
    cfg = args_to_config(build_parser().parse_args(argv))
    assert cfg.kmeans_backend == "auto" and cfg.scoring_backend == "host"
    with pytest.raises(SystemExit):
        build_parser().parse_args(argv + ["--scoring", "gpu"])


def test_cli_cpu_run_with_hip_kmeans_and_device_scoring(tiny_files, tmp_path):
    """python -m g2vec_amd ... --device cpu --kmeans hip --scoring device
    writes the output triple (the CPU mirrors carry both backends)."""
    import json
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "cli")
    log = str(tmp_path / "m.jsonl")
    env = dict(os.environ)
    env["PYTHONPATH"] = repo + os.pathsep + env.get("PYTHONPATH", "")
    proc = subprocess.run(
        [sys.executable, "-m", "g2vec_amd", tiny_files["expression"],
         tiny_files["clinical"], tiny_files["network"], out,
         "-p", "15", "-r", "3", "-e", "25", "--device", "cpu",
         "--kmeans", "hip", "--scoring", "device", "--log-jsonl", log],
        cwd=repo, env=env, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-2000:]
    for suffix in ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt"):
        assert os.path.getsize(out + suffix) > 0
    with open(log) as fh:
        events = [json.loads(line) for line in fh]
    km = [e for e in events if e.get("event") == "kmeans"]
    assert len(km) == 1, [e.get("event") for e in events]
    assert km[0]["kmeans_iterations"] >= 1 and km[0]["kmeans_inertia"] >= 0
