"""The step-3 glue on the device against the fp64 / literal references of
step3_cases: build_group_graph through the pcc_edges and corr_gemm kernels
(mode "auto" takes the MFMA branch up to S_group = 288), integrate_pathsets
and subset on device tensors, the trainer's device helpers, and
generate_paths' two-stream overlap. CPU twins: test_step3_glue_cpu.py."""
import pytest
import torch

import step3_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape", sc.GRAPH_SHAPES, ids=str)
def test_group_graph_matches_fp64_on_gpu(dev, shape):
    sc.check_reference_conditions(*shape)
    sc.check_graph_case(*shape, dev)


def test_group_graph_empty_cases_on_gpu(dev):
    sc.check_graph_empty_cases(dev)


def test_exact_threshold_is_strict_on_gpu(dev):
    sc.check_exact_threshold(dev)


@pytest.mark.parametrize("variant", ["base", "permuted", "crafted",
                                     "crafted_permuted"])
def test_integrate_matches_literal_port_on_gpu(dev, variant):
    sc.check_base_conditions()
    good, poor = sc.base_walksets()
    if "permuted" in variant:
        good, poor = sc.permuted(good, 1), sc.permuted(poor, 2)
    if "crafted" in variant:
        good, poor = sc.crafted_hashes(good, poor, 5)
    sc.check_integrate(good, poor, dev)


def test_integrate_edge_cases_on_gpu(dev):
    sc.check_integrate_edges(dev)


def test_subset_matches_numpy_slicing_on_gpu(dev):
    sc.check_subset(dev)


def test_trainer_helpers_match_numpy_on_gpu(dev):
    sc.check_trainer_helpers(dev)


@pytest.mark.parametrize("pcc_mode", ["edge", "auto"])
def test_generate_paths_equals_its_chain_on_gpu(dev, tiny_files, pcc_mode):
    sc.check_generate_paths(tiny_files, dev, pcc_mode)
