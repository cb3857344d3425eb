"""HIP kernels of steps 5-6 (kmeans_step, kmeans_mind2_, row_norms,
t_scores) against the fp64 references of steps56_cases.py, plus
cluster.kmeans_hip and the pipeline with --kmeans hip --scoring device.
All tests need an MI355X; test_steps56_cpu.py runs the same cases on the
CPU mirrors and states where the tolerances come from.

Shapes: every HPL instantiation (h = 64..1024), k in {2, 3, 8}, and G below
one block's 4 waves (1, 3), as many rows as waves (4), ragged (5, 1003: odd
counts leave a wave with one row of its two-row pass) and 33000 rows: the
grid is capped at what is resident (at most 8 blocks per CU, 2048 blocks on
256 CUs; 256 at k*h = 8192) and a block takes 8 rows per pass, so the
grid-stride loop runs 3 to 17 passes and the fold reads every partial."""
import pytest
import torch

import kernel_edges as ke
import steps56_cases as sc
from g2vec_amd import cluster, ops, scoring
from g2vec_amd.config import G2VecConfig
from g2vec_amd.pipeline import load_study, run

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALL_H = (64, 128, 256, 512, 1024)


# ============================================================ kmeans_step
@pytest.mark.parametrize("k", sc.KM_K)
@pytest.mark.parametrize("G", [1, 3, 4, 5, 1003, 33000])
@pytest.mark.parametrize("h", ALL_H)
def test_kmeans_step_exact(h, G, k):
    X, C, ref = sc.kmeans_case(G, h, k)
    prev = torch.zeros(G, dtype=torch.int32)
    out = sc.run_step(ops, X, C, prev, DEV)
    sc.assert_step_matches(out, C, ref, prev)


def test_kmeans_step_tie_lowest_index_and_empty_cluster_keeps_row():
    X, C, ref = sc.tie_case()
    prev = torch.zeros(X.shape[0], dtype=torch.int32)
    out = sc.run_step(ops, X, C, prev, DEV)
    sc.assert_step_matches(out, C, ref, prev)
    assert int((out["labels"] == 2).sum()) == 0
    assert int(out["counts"][2]) == 0
    assert torch.equal(out["C_new"][2], C[2])


@pytest.mark.parametrize("which", ["all", "none", "one"])
def test_kmeans_step_n_changed(which):
    X, C, ref = sc.kmeans_case(1003, 64, 3)
    labels = ref[1].int()
    prev = labels.clone()
    if which == "all":
        prev = (labels + 1) % 3
    elif which == "one":
        prev[517] = (prev[517] + 1) % 3
    out = sc.run_step(ops, X, C, prev, DEV)
    assert int(out["n_changed"][0]) == {"all": 1003, "none": 0, "one": 1}[which]


def test_kmeans_step_in_place_arguments():
    X, C, ref = sc.kmeans_case(33000, 128, 3)
    labels = torch.zeros(33000, dtype=torch.int32, device=DEV)
    Cw = C.to(DEV)
    out = sc.step_outputs(X, C, DEV)
    ops.kmeans_step(X.to(DEV), Cw, labels, labels, Cw, out["sums"],
                    out["counts"], out["n_changed"], out["inertia"])
    assert torch.equal(labels.cpu().long(), ref[1])
    assert torch.equal(Cw.cpu(), ref[5])
    assert int(out["n_changed"][0]) == int((ref[1] != 0).sum())


@pytest.mark.parametrize("G", [5, 1003, 33000])
@pytest.mark.parametrize("h", ALL_H)
def test_kmeans_mind2_exact(h, G):
    X, C, ref = sc.kmeans_case(G, h, 3)
    D = ref[0]
    Xd = X.to(DEV)
    d2 = torch.full((G,), float("inf"), device=DEV)
    ops.kmeans_mind2_(Xd, C[0].contiguous().to(DEV), d2)
    assert ke.bitwise_equal(d2, D[:, 0])
    ops.kmeans_mind2_(Xd, C[1].contiguous().to(DEV), d2)
    assert ke.bitwise_equal(d2, torch.minimum(D[:, 0], D[:, 1]))


# ============================================================= kmeans_hip
def test_kmeans_hip_gpu_matches_cpu_mirror_on_blobs():
    X = torch.from_numpy(sc.blobs())
    cl, cc, ci, cn = cluster.kmeans_hip(X, 3, seed=0)
    gl, gc, gi, gn = cluster.kmeans_hip(X.to(DEV), 3, seed=0)
    assert gl.is_cuda and gc.is_cuda
    assert torch.equal(gl.cpu(), cl)
    err = float((gc.cpu() - cc).abs().max())
    print("centroid err", err, "inertia", gi, ci, "iters", gn, cn)
    assert err <= 1e-6
    lg = cluster.find_lgroups(X.to(DEV), sc.blob_freq(), backend="hip")
    assert (lg == cluster.find_lgroups(sc.blobs(), sc.blob_freq(),
                                       backend="sklearn")).all()


def test_kmeans_hip_check_every_is_bitwise_invariant_on_gpu():
    gen = torch.Generator().manual_seed(4)
    X = torch.randn(3000, 128, generator=gen).to(DEV)   # many Lloyd steps
    a = cluster.kmeans_hip(X, 3, seed=0, n_init=2, check_every=1)
    b = cluster.kmeans_hip(X, 3, seed=0, n_init=2, check_every=4)
    assert a[3] > 4                       # ran past one check interval
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[2] == b[2] and a[3] == b[3]


# =============================================================== t_scores
@pytest.mark.parametrize("S", sc.T_S + (300,))
def test_t_scores_within_one_ulp_of_host(S):
    for n_good in (2, S // 2):
        expr, labels, host = sc.t_case(S, n_good=n_good)
        got = ops.t_scores(expr.to(DEV), labels.to(DEV)).cpu().numpy()
        assert sc.ulp_diff_f32(got, host) <= 1
        assert got[0] == 0.0 and got[1] == 0.0
    expr, labels, host = sc.t_case(S, n_good=1)
    got = ops.t_scores(expr.to(DEV), labels.int().to(DEV)).cpu().numpy()
    assert (host == 0).all() and (got == 0).all()


@pytest.mark.parametrize("G", [1, 255, 257, 1003, 70000])
def test_t_scores_gene_counts(G):
    expr, labels, host = sc.t_case(65, G=G, n_good=30)
    got = ops.t_scores(expr.to(DEV), labels.to(DEV)).cpu().numpy()
    assert got.shape == (G,)
    assert sc.ulp_diff_f32(got, host) <= 1


def test_t_scores_more_samples_than_one_label_tile():
    """S = 2500 spans three 1024-sample label tiles."""
    expr, labels, host = sc.t_case(2500, G=300, n_good=1100)
    got = ops.t_scores(expr.to(DEV), labels.to(DEV)).cpu().numpy()
    assert sc.ulp_diff_f32(got, host) <= 1


# ============================================================== row_norms
@pytest.mark.parametrize("G", [1, 1003, 33000])
@pytest.mark.parametrize("h", ALL_H)
def test_row_norms(h, G):
    W, ref64, ref_np = sc.norm_case(G, h)
    sc.assert_norms_match(ops.row_norms(W.to(DEV)).cpu().numpy(), ref64,
                          ref_np)


# ========================================================= binding guards
def _step_args(G=40, h=64, k=3):
    X, C, _ = sc.kmeans_case(1003, h, k)
    X, C = X[:G].contiguous().to(DEV), C.to(DEV)
    prev = torch.zeros(G, dtype=torch.int32, device=DEV)
    out = sc.step_outputs(X, C, DEV)
    return [X, C, prev, out["labels"], out["C_new"], out["sums"],
            out["counts"], out["n_changed"], out["inertia"]]


def _assert_untouched(args):
    for t in args[3:]:
        assert bool((t == -7).all()), "an output was written"


@pytest.mark.parametrize("case,match", [
    ("x_f64", "X must be float32"),
    ("labels_i64", "labels must be int32"),
    ("inertia_f32", "inertia must be float64"),
    ("x_noncontig", "X must be contiguous"),
    ("k9", "k must be in"),
    ("h96", "hidden must be"),
    ("c_cols", "C must have"),
    ("labels_short", "one element per X row"),
    ("cnew_shape", "C_new must have"),
])
def test_kmeans_step_binding_guards(case, match):
    args = _step_args()
    if case == "x_f64":
        args[0] = args[0].double()
    elif case == "labels_i64":
        args[3] = torch.full((40,), -7, dtype=torch.int64, device=DEV)
    elif case == "inertia_f32":
        args[8] = torch.full((1,), -7.0, device=DEV)
    elif case == "x_noncontig":
        args[0] = torch.zeros(64, 40, device=DEV).t()
    elif case == "k9":
        args[1] = torch.zeros(9, 64, device=DEV)
    elif case == "h96":
        args[0] = torch.zeros(40, 96, device=DEV)
        args[1] = torch.zeros(3, 96, device=DEV)
    elif case == "c_cols":
        args[1] = torch.zeros(3, 128, device=DEV)
    elif case == "labels_short":
        args[3] = torch.full((39,), -7, dtype=torch.int32, device=DEV)
    elif case == "cnew_shape":
        args[4] = torch.full((2, 64), -7.0, device=DEV)
    with pytest.raises(RuntimeError, match=match):
        ops.kmeans_step(*args)
    torch.cuda.synchronize()
    _assert_untouched(args)


def test_other_binding_guards():
    X = torch.zeros(10, 64, device=DEV)
    d2 = torch.full((10,), -7.0, device=DEV)
    with pytest.raises(RuntimeError, match="hidden must be"):
        ops.kmeans_mind2_(torch.zeros(10, 96, device=DEV),
                          torch.zeros(96, device=DEV), d2)
    with pytest.raises(RuntimeError, match="one element per X column"):
        ops.kmeans_mind2_(X, torch.zeros(128, device=DEV), d2)
    with pytest.raises(RuntimeError, match="one element per X row"):
        ops.kmeans_mind2_(X, torch.zeros(64, device=DEV), d2[:9])
    with pytest.raises(RuntimeError, match="d2 must be float32"):
        ops.kmeans_mind2_(X, torch.zeros(64, device=DEV), d2.double())
    with pytest.raises(RuntimeError, match="hidden must be"):
        ops.row_norms(torch.zeros(10, 96, device=DEV))
    with pytest.raises(RuntimeError, match="W must be contiguous"):
        ops.row_norms(torch.zeros(64, 10, device=DEV).t())
    expr = torch.zeros(6, 10, device=DEV)
    with pytest.raises(RuntimeError, match="labels must be int32 or int64"):
        ops.t_scores(expr, torch.zeros(6, device=DEV))
    with pytest.raises(RuntimeError, match="one element per sample"):
        ops.t_scores(expr, torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="expr must be float32"):
        ops.t_scores(expr.double(), torch.zeros(6, dtype=torch.int64,
                                                device=DEV))
    torch.cuda.synchronize()
    assert bool((d2 == -7).all())


# ============================================================= end to end
def _cfg(tiny_files, name, **kw):
    base = dict(expression_file=tiny_files["expression"],
                clinical_file=tiny_files["clinical"],
                network_file=tiny_files["network"], result_name=name,
                len_path=15, num_repetition=3, epochs=25, device="cuda",
                seed=0)
    base.update(kw)
    return G2VecConfig(**base)


def _read(path):
    with open(path, "rb") as fh:
        return fh.read()


def test_pipeline_with_hip_kmeans_and_device_scoring(tiny_files, tmp_path):
    outs = []
    for i in range(2):
        name = str(tmp_path / f"run{i}")
        res = run(_cfg(tiny_files, name, kmeans_backend="hip",
                       scoring_backend="device"))
        outs.append((name, res))
        for suffix in ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt"):
            assert len(_read(name + suffix)) > 0
    (a, ra), (b, rb) = outs
    assert _read(a + "_lgroups.txt") == _read(b + "_lgroups.txt")
    assert _read(a + "_biomarkers.txt") == _read(b + "_biomarkers.txt")

    # same W and L-groups fed to both scoring backends: same biomarkers
    st = load_study(_cfg(tiny_files, a), log=lambda *a_, **k_: None)
    W, lg = ra["W_ih"], ra["lgroups"]
    host = scoring.select_biomarkers(W, lg, st.expr, st.labels, st.genes, 50)
    d_all = ops.row_norms(torch.from_numpy(W).to(DEV)).cpu().numpy()
    t_all = ops.t_scores(st.expr_t, st.labels_t).cpu().numpy()
    dev = scoring.select_biomarkers(W, lg, st.expr, st.labels, st.genes, 50,
                                    d_all=d_all, t_all=t_all)
    assert dev == host and dev == ra["biomarkers"]
