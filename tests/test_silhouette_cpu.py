"""L-group silhouettes on the CPU: cpu_ref.cluster_dist_sums (the mirror of
the HIP kernels) through ops.cluster_dist_sums, cluster_quality.silhouette and
the pipeline's scores table, against the f64 reference of silhouette_cases.py.
The same assertions hold the kernels in test_gpu_silhouette.py."""
import json

import numpy as np
import pytest
import torch

import silhouette_cases as sc
from g2vec_amd import ops

DEV = "cpu"


@pytest.mark.parametrize("Q,G,h,k,layout", sc.EXACT_CASES)
def test_exact_fixtures(Q, G, h, k, layout):
    sc.check_exact(ops, sc.exact_case(Q, G, h, k, layout), DEV)


def test_label_layouts():
    sc.check_layout_properties(ops, DEV)


@pytest.mark.parametrize("shape", sc.REAL_SHAPES)
def test_real_fixtures(shape):
    sc.check_real(ops, shape, DEV)


@pytest.mark.parametrize("shape", sc.REAL_SHAPES)
def test_recorded_errors_hold(shape):
    """The figures the bounds are 4x of: the k-ordered chain is a fixed
    computation and reproduces its record; the mirror's BLAS blocking may
    differ between builds but stays inside the bound."""
    from g2vec_amd.cluster_quality import silhouette_from_sums
    case = sc.real_case(*shape)
    Dc = sc.chain_sums(case)
    e_d = sc.rel_err(Dc, case["D"])
    got = silhouette_from_sums(Dc, case["labels"][case["q_index"]],
                               case["n_c"])
    e_s = float(np.abs(got["s"] - case["s"]).max())
    m_d, m_s = sc.real_errors(ops, shape, DEV)
    print("chain", e_d, e_s, "mirror", m_d, m_s, "recorded",
          sc.REAL_ERR_D[shape], sc.REAL_ERR_S[shape])
    assert e_d <= sc.REAL_ERR_D[shape][1] and e_s <= sc.REAL_ERR_S[shape][1]
    assert m_d <= sc.REAL_BOUND_D[shape] and m_s <= sc.REAL_BOUND_S[shape]


@pytest.mark.parametrize("shape", sc.REAL_SHAPES)
def test_centring_q_chunk_and_rows(shape):
    sc.check_invariances(shape, DEV)


def test_against_sklearn():
    sc.check_sklearn(DEV)


def test_reference_formulas():
    """The reference itself on a case worked by hand: points 0, 1 | 5 | 9 on
    a line, the last cluster empty."""
    X = np.array([[0.0], [1.0], [5.0], [9.0]])
    lab = np.array([0, 0, 1, 2])
    D = sc.ref_sums(sc.ref_dist(X, X), lab, 4, np.arange(4))
    assert D.tolist() == [[1, 5, 9, 0], [1, 4, 8, 0], [9, 0, 4, 0],
                          [17, 4, 0, 0]]
    s, a, b, near = sc.ref_silhouette(D, lab, np.bincount(lab, minlength=4))
    assert a.tolist() == [1, 1, 0, 0] and b.tolist() == [5, 4, 4, 4]
    assert near.tolist() == [1, 1, 2, 1]
    assert s.tolist() == [0.8, 0.75, 0, 0]          # singletons: s = 0
    # a tie between two clusters: the lowest index
    D = np.array([[0.0, 6.0, 3.0]])
    assert sc.ref_silhouette(D, np.array([0]), np.array([1, 2, 1]))[3][0] == 1


def test_mirror_blocks():
    """More candidates than one block of the mirror holds, every distance 2:
    the sums are 2 * (cluster size - self)."""
    X = torch.zeros(9000, 4)
    X[::2, 0] = 2.0
    lab = (torch.arange(9000) % 2).int()
    qi = torch.tensor([0, 1, 8999] * 30, dtype=torch.int32)
    D = ops.cluster_dist_sums(X[qi.long()].contiguous(), X, lab, 2, q_index=qi)
    assert D[0].tolist() == [0.0, 9000.0]
    assert D[1].tolist() == [9000.0, 0.0]
    assert D[2].tolist() == [9000.0, 0.0]
    assert torch.equal(D[:3], D[87:])


def test_wrapper_errors():
    sc.check_wrapper_errors(ops, DEV)


def test_write_scores_columns(tmp_path):
    from g2vec_amd import io as gio
    genes = ["A", "B"]
    scores = dict(d_score=[1.0, 2.0], t_score=[0.5, 0.25],
                  gene_score=[0.75, np.nan], is_biomarker=[1, 0],
                  silhouette=np.array([0.5, -0.125]),
                  nearest_lgroup=np.array([1, 0]))
    perm = dict(p=[0.5, 1.0], q_bh=[1.0, 1.0], p_maxT=[0.25, 1.0])
    out = gio.write_scores(str(tmp_path / "x"), genes, [0, 2], scores, perm)
    assert open(out).read().splitlines() == [
        "\t".join(sc.SCORE_COLS + sc.PERM_COLS),
        "A\t0\t1.000000\t0.500000\t0.750000\t1\t0.500000\t1\t0.5\t1\t0.25",
        "B\t2\t2.000000\t0.250000\tNA\t0\t-0.125000\t0\t1\t1\t1"]
    scores["silhouette"] = scores["nearest_lgroup"] = None
    out = gio.write_scores(str(tmp_path / "y"), genes, [0, 2], scores)
    assert open(out).read().splitlines()[1:] == [
        "A\t0\t1.000000\t0.500000\t0.750000\t1\tNA\tNA",
        "B\t2\t2.000000\t0.250000\tNA\t0\tNA\tNA"]


def test_pipeline_silhouette_columns(tiny_files, tmp_path, monkeypatch):
    sc.check_pipeline(tiny_files, tmp_path, DEV, monkeypatch)


def test_run_without_the_flag_is_unchanged(tmp_path, capsys):
    """No flag, no trace: the golden run's biomarkers and L-groups byte for
    byte, its vectors as the golden test pins them, the scores table with
    its six columns and rows that agree with those files, no silhouette
    record and no silhouette word in the transcript, the arguments line
    included."""
    import pathlib

    from g2vec_amd.config import G2VecConfig
    from g2vec_amd.pipeline import run
    from g2vec_amd.utils.synth import make_ex_style_files
    files = make_ex_style_files(str(tmp_path), n_genes=120, n_extra=20,
                                n_edges=2500, n_samples=60, n_poor=26,
                                n_modules=5, seed=9)
    log = str(tmp_path / "g.jsonl")
    run(G2VecConfig(expression_file=files["expression"],
                    clinical_file=files["clinical"],
                    network_file=files["network"],
                    result_name=str(tmp_path / "g"), len_path=12,
                    num_repetition=3, hidden=64, epochs=15, num_biomarker=10,
                    seed=7, device="cpu", write_scores=True, log_jsonl=log))
    golden = pathlib.Path(__file__).parent / "golden"
    for sfx in ("biomarkers", "lgroups"):
        assert (tmp_path / f"g_{sfx}.txt").read_bytes() == \
            (golden / f"tiny_{sfx}.txt").read_bytes(), sfx
    # the vectors as test_golden_output_triple pins them: layout and gene
    # column byte for byte, numbers to its 2e-6 (host BLAS summation order)
    got = (tmp_path / "g_vectors.txt").read_text().splitlines()
    want = (golden / "tiny_vectors.txt").read_text().splitlines()
    assert len(got) == len(want) and got[0] == want[0]
    got_rows = [ln.split("\t") for ln in got[1:]]
    want_rows = [ln.split("\t") for ln in want[1:]]
    assert [r[0] for r in got_rows] == [r[0] for r in want_rows]
    assert [len(r) for r in got_rows] == [len(r) for r in want_rows]
    got_v = np.array([r[1:] for r in got_rows], dtype=np.float64)
    want_v = np.array([r[1:] for r in want_rows], dtype=np.float64)
    assert np.abs(got_v - want_v).max() <= 2e-6
    # the scores table agrees with the two pinned files row by row
    body = [ln.split("\t") for ln in
            (tmp_path / "g_scores.txt").read_text().splitlines()[1:]]
    lg_rows = (golden / "tiny_lgroups.txt").read_text().splitlines()[1:]
    assert ["\t".join(r[:2]) for r in body] == lg_rows
    bio = set((golden / "tiny_biomarkers.txt").read_text().splitlines()[1:])
    assert {r[0] for r in body if r[5] == "1"} == bio
    assert all(len(r) == 6 for r in body)
    head = (tmp_path / "g_scores.txt").read_text().splitlines()[0]
    assert head.split("\t") == ["GeneSymbol", "Lgroup", "d_score", "t_score",
                                "gene_score", "biomarker"]
    assert "silhouette" not in open(log).read()
    assert "silhouette" not in capsys.readouterr().out
    events = [json.loads(ln)["event"] for ln in open(log)]
    assert events[0] == "phase" and events[-1] == "done"
