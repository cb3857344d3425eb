"""Nearest-gene queries on the CPU: cpu_ref.knn_topk (the mirror of the HIP
kernel) through ops.knn_topk, neighbors.nearest_genes and the pipeline's
<name>_neighbors.txt, against the fp64 reference of neighbor_cases.py. The
same assertions hold the kernels in test_gpu_neighbors.py."""
import numpy as np
import pytest
import torch

import neighbor_cases as nc
from g2vec_amd import ops

DEV = "cpu"


@pytest.mark.parametrize("Q,G,h,k,with_q_index", nc.EXACT_CASES)
def test_exact_fixtures(Q, G, h, k, with_q_index):
    nc.check_exact(ops, nc.exact_case(Q, G, h, k, with_q_index), DEV)


@pytest.mark.parametrize("shape", nc.REAL_SHAPES)
def test_real_fixtures(shape):
    nc.check_real(ops, shape, DEV)


@pytest.mark.parametrize("shape", nc.REAL_SHAPES)
def test_recorded_errors_hold(shape):
    """The figures the bound is 4x of: the mirror's and the k-ordered
    chain's largest error over every candidate score of the fixture."""
    case = nc.real_case(*shape)
    live = np.isfinite(case["sc"])
    mirror = (torch.from_numpy(case["Xq"])
              @ torch.from_numpy(case["X"]).t()).numpy().astype(np.float64)
    chain = nc.chain_scores(case["Xq"], case["X"]).astype(np.float64)
    e_m = float(np.abs(mirror - case["sc"])[live].max())
    e_c = float(np.abs(chain - case["sc"])[live].max())
    print("mirror", e_m, "chain", e_c, "recorded", nc.REAL_ERR[shape])
    # the chain is a fixed computation; the mirror's blocking may differ
    # between BLAS builds but stays inside the bound
    assert e_c <= nc.REAL_ERR[shape][1]
    assert max(e_m, e_c) <= nc.REAL_BOUND[shape]


def test_reference_tie_rule():
    """The reference itself: equal values by ascending index, -0.0 == +0.0,
    self excluded, short tail."""
    sc = np.array([[1.0, 2.0, 2.0, -0.0, 0.0, -np.inf]])
    idx, val = nc.ref_topk(sc, 6)
    assert idx.tolist() == [[1, 2, 0, 3, 4, -1]]
    assert np.isneginf(val[0, -1])


def test_mirror_blocks_and_ties():
    """More candidates than one block of the mirror holds, all dots equal:
    the result is the lowest indices, self skipped."""
    X = torch.ones(70000, 4)
    qi = torch.tensor([0, 3, 69999] * 30, dtype=torch.int32)
    idx, val = ops.knn_topk(X[qi.long()].contiguous(), X, 4, q_index=qi)
    assert idx[0].tolist() == [1, 2, 3, 4]
    assert idx[1].tolist() == [0, 1, 2, 4]
    assert idx[2].tolist() == [0, 1, 2, 3]
    assert (val == 4.0).all()


def test_q_chunk_invariance():
    for shape in nc.STRICT_SHAPES:
        nc.check_q_chunk(shape, DEV)


def test_wrapper_errors():
    nc.check_wrapper_errors(ops, DEV)


def test_cosine_zero_and_twin_rows():
    nc.check_zero_row_cosine(DEV)


def test_write_neighbors_omits_missing(tmp_path):
    from g2vec_amd import io as gio
    genes = ["A", "B", "C"]
    idx = np.array([[2, 1, -1]], dtype=np.int32)
    sim = np.array([[0.5, -0.25, -np.inf]], dtype=np.float32)
    out = gio.write_neighbors(str(tmp_path / "x"), genes, [0], idx, sim,
                              [0, 1, 2], ["C"])
    assert out.endswith("x_neighbors.txt")
    assert open(out).read().splitlines() == [
        "\t".join(nc.NBR_COLS), "A\t1\tC\t0.500000\t2\t1",
        "A\t2\tB\t-0.250000\t1\t0"]


def test_cli_flags():
    from g2vec_amd.cli import args_to_config, build_parser
    a = build_parser().parse_args(["e", "c", "n", "r", "--neighbors", "7",
                                   "--neighbors-of", "all"])
    cfg = args_to_config(a)
    assert cfg.neighbors == 7 and cfg.neighbors_of == "all"


def test_validate():
    nc.check_validate()


def test_pipeline_neighbors_table(tiny_files, tmp_path):
    nc.check_pipeline(tiny_files, tmp_path, DEV)
