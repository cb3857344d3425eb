"""Rank statistics on the GPU: rank_columns_kernel and ranksum_scores_kernel
held to the assertions the CPU mirror passes in test_rank_cpu.py (fixtures
and counting reference: rank_cases.py), plus the launch edges with
sentinel-filled outputs, the binding's guards, the Spearman graph and the
rank-based permutation null on the device, and one pipeline run."""
import numpy as np
import pytest
import torch

import rank_cases as rc
from g2vec_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_garbage():
    """The pipeline runs below leave reference cycles that hold device
    tensors; collect them here, so that tests which compare
    torch.cuda.memory_allocated() around a call do not see them freed by a
    collection that happens to run inside that call."""
    yield
    import gc
    gc.collect()


def test_tile_constants_match_the_kernel():
    nat = ops.native()
    assert (nat.RK_TG, nat.RK_SJ, nat.RK_IB, nat.RK_WAVES,
            nat.RK_MAX_BLOCKS) == (ops.RANK_TG, ops.RANK_SJ, ops.RANK_IB,
                                   ops.RANK_WAVES, ops.RANK_MAX_BLOCKS)


# --------------------------------------------------- against the references
@pytest.mark.parametrize("S,G", rc.SHAPES)
def test_ranks_equal_counting_reference(S, G):
    rc.check_ranks(S, G, DEV)


@pytest.mark.parametrize("S,G,balanced", rc.CASES)
def test_ranksum_within_one_ulp_of_host(S, G, balanced):
    rc.check_ranksum(S, G, balanced, DEV)


def test_repeatable():
    rc.check_repeatable(DEV)


# ------------------------------------------ every output element is written
@pytest.mark.parametrize("S,G", [(rc.SJ + 1, rc.TG + 1), (rc.PASS + 1, 1),
                                 (1, rc.TG + 1), (1, 1)])
def test_every_output_element_is_written(S, G):
    """A second gene tile with one live column, a last j-tile and a last
    i-pass with one live sample, G = 1 and S = 1: outputs pre-filled with a
    sentinel."""
    nat = ops.native()
    x = rc.tensor(rc.values(S, G), DEV)
    ranks = torch.full((S, G), -7.0, dtype=torch.float32, device=DEV)
    nat.rank_columns_(x, ranks)
    assert (ranks >= 1.0).all()
    assert ranks.cpu().numpy().tobytes() == rc.ranks_of(S, G).tobytes()
    lab = rc.tensor(rc.labels_of(S, True), DEV).int()
    z = torch.full((G,), -7.0, dtype=torch.float32, device=DEV)
    auc = torch.full((G,), -7.0, dtype=torch.float32, device=DEV)
    nat.ranksum_scores_(x, lab, z, auc)
    assert (z >= 0.0).all() and (auc >= 0.0).all() and (auc <= 1.0).all()


# ------------------------------------ binding guards leave outputs untouched
def test_binding_guards_leave_outputs_untouched():
    S, G = 65, rc.TG + 1
    nat = ops.native()
    x = rc.tensor(rc.values(S, G), DEV)
    lab = rc.tensor(rc.labels_of(S, True), DEV).int()
    ranks = torch.full((S, G), -7.0, dtype=torch.float32, device=DEV)
    z = torch.full((G,), -7.0, dtype=torch.float32, device=DEV)
    auc = torch.full((G,), -7.0, dtype=torch.float32, device=DEV)
    for bad in (x.double(),                       # dtype
                x.t().contiguous().t(),           # contiguity
                x[:0],                            # S = 0
                x.cpu(),                          # a CPU tensor
                x[0]):                            # not [S, G]
        with pytest.raises(RuntimeError):
            nat.rank_columns_(bad, ranks)
        with pytest.raises(RuntimeError):
            nat.ranksum_scores_(bad, lab, z, auc)
    for bad_out in (ranks.double(), ranks[:-1], ranks[:, :-1],
                    ranks.t().contiguous().t(), ranks.cpu()):
        with pytest.raises(RuntimeError):
            nat.rank_columns_(x, bad_out)
    lab_two = lab.clone()
    lab_two[3] = 2
    for bad_lab in (lab.long(), lab[:-1].contiguous(),       # dtype, length
                    torch.cat([lab, lab])[::2], lab.cpu(),
                    lab_two):                                # not 0/1
        with pytest.raises(RuntimeError):
            nat.ranksum_scores_(x, bad_lab, z, auc)
    for bz, ba in ((z.double(), auc), (z, auc.double()),
                   (z[:-1].contiguous(), auc), (z, auc[:-1].contiguous()),
                   (z.cpu(), auc)):
        with pytest.raises(RuntimeError):
            nat.ranksum_scores_(x, lab, bz, ba)
    torch.cuda.synchronize()
    assert (ranks == -7.0).all() and (z == -7.0).all() and (auc == -7.0).all()
    # and the wrapper's own checks, on device tensors
    nan = x.clone()
    nan[7, 3] = float("nan")
    with pytest.raises(ValueError):
        ops.rank_columns(nan)
    with pytest.raises(ValueError):
        ops.ranksum_scores(nan, lab)
    with pytest.raises(ValueError):
        ops.ranksum_scores(x, lab.cpu())


# ------------------------------------------------------ graph on the device
@pytest.mark.parametrize("mode", ["edge", "gemm"])
def test_spearman_graph_is_pearson_graph_of_ranks(mode):
    rc.check_spearman_is_pearson_of_ranks(DEV, mode)


# ----------------------------------------------------------- CPU against GPU
def test_ranks_equal_on_cpu_and_gpu():
    for S, G in ((135, 130), (2 * rc.SJ + 1, 130)):
        x = rc.tensor(rc.values(S, G))
        assert torch.equal(ops.rank_columns(x),
                           ops.rank_columns(x.to(DEV)).cpu())


def test_rank_permutation_counts_equal_the_cpu_mirror():
    from g2vec_amd import scoring
    rc.check_perm_counts(DEV)
    case = rc.perm_case()
    ranks = ops.rank_columns(rc.tensor(case["expr"])).numpy()
    kw = dict(B=rc.PERM_B, seed=21)
    cpu = scoring.permutation_pvalues(ranks, case["labels"], device="cpu",
                                      **kw)
    gpu = scoring.permutation_pvalues(ranks, case["labels"], device=DEV,
                                      **kw)
    assert np.array_equal(cpu["counts"], gpu["counts"])


# ----------------------------------------------------------------- pipeline
def test_rank_pipeline_on_the_device(tiny_files, tmp_path):
    from g2vec_amd.pipeline import run
    bio = rc.check_rank_pipeline(tiny_files, tmp_path, DEV,
                                 scoring_backend="device")
    run(rc.pipeline_cfg(tiny_files, tmp_path, DEV, "h", corr="spearman",
                        score_stat="ranksum", permutations=64,
                        scoring_backend="host"))
    host = (tmp_path / "h_biomarkers.txt").read_text().splitlines()[1:]
    assert bio == host
