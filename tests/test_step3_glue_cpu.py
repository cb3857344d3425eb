"""CPU twins of test_gpu_step3_glue.py: the step-3 glue (per-group graph,
path-set integration, generate_paths, the trainer's device helpers) against
the fp64 / literal references of step3_cases, on the CPU mirror. Also the
checks that need no device: the fixtures' own conditions and the proof that
the references tell a wrong implementation from a right one."""
import numpy as np
import pytest
import torch

import step3_cases as sc

CPU = torch.device("cpu")


# ------------------------------------------------------------------ A
@pytest.mark.parametrize("shape", sc.GRAPH_SHAPES, ids=str)
def test_graph_fixture_conditions(shape):
    sc.check_reference_conditions(*shape)


@pytest.mark.parametrize("shape", sc.GRAPH_SHAPES, ids=str)
def test_group_graph_matches_fp64(shape):
    """Holds the mirror (all three modes) to the derived band: a failure
    here means the derivation in step3_cases is wrong."""
    sc.check_graph_case(*shape, CPU)


def test_group_graph_empty_cases():
    sc.check_graph_empty_cases(CPU)


def test_exact_threshold_is_strict():
    sc.check_exact_threshold(CPU)


# ------------------------------------------------------------------ B
def test_walkset_fixture_conditions():
    sc.check_base_conditions()


@pytest.mark.parametrize("variant", ["base", "permuted", "crafted",
                                     "crafted_permuted"])
def test_integrate_matches_literal_port(variant):
    good, poor = sc.base_walksets()
    if "permuted" in variant:
        good, poor = sc.permuted(good, 1), sc.permuted(poor, 2)
    if "crafted" in variant:
        good, poor = sc.crafted_hashes(good, poor, 5)
    sc.check_integrate(good, poor, CPU)


def test_integrate_edge_cases():
    sc.check_integrate_edges(CPU)


def test_subset_matches_numpy_slicing():
    sc.check_subset(CPU)


def test_trainer_helpers_match_numpy():
    sc.check_trainer_helpers(CPU)


# ------------------------------------------------------------------ C
@pytest.mark.parametrize("pcc_mode", ["edge", "auto"])
def test_generate_paths_equals_its_chain(tiny_files, pcc_mode):
    sc.check_generate_paths(tiny_files, CPU, pcc_mode)


# ------------------------------------------- the references can tell
def _raises(fn, *a, **k) -> bool:
    try:
        fn(*a, **k)
    except AssertionError:
        return True
    return False


def test_wrong_graph_variants_are_caught():
    """A reference built with the wrong rule, posing as the implementation,
    must fail the banded comparison."""
    for shape in sc.GRAPH_SHAPES[2:]:
        fxs = sc.graph_fixture(*shape)
        for group in (0, 1):
            ref = sc.graph_reference(*shape, group)
            if ref["S"] < 3:
                continue
            # the true rule passes its own comparison
            sc.compare_banded(ref["A"], ref)
            # 1/(S-1): |PCC| grows by about thr/S > the planted distance
            wrong = sc.ref_adjacency(fxs["expr"], fxs["labels"], group,
                                     fxs["edges"], shape[0],
                                     norm_s_minus_1=True)
            assert _raises(sc.compare_banded, wrong, ref), (shape, group)
    # >= differs from > only at equality, which no band can see: it is
    # told apart on an exact-arithmetic pair (|PCC64| == 0.5 exactly), on
    # which check_exact_threshold holds the implementation to the strict
    # rule; here: the two rules do differ on that pair
    expr = np.stack([sc.EXACT_X, sc.EXACT_Y], axis=1).astype(np.float32)
    labels = np.zeros(8, dtype=np.int64)
    edges = [(0, 1), (1, 0)]
    C, _m, _s = sc.pcc64_matrix(expr)
    assert C[0, 1] == 0.5
    right = sc.ref_adjacency(expr, labels, 0, edges, 2)
    wrong = sc.ref_adjacency(expr, labels, 0, edges, 2, ge=True)
    assert right.sum() == 0.0 and (wrong != 0).sum() == 2


def test_wrong_integration_variants_are_caught():
    good, poor = sc.base_walksets()
    ref = sc.ref_integrate(good, poor, sc.PG)
    last = sc.ref_integrate(good, poor, sc.PG, last_index=True)
    assert np.array_equal(last["offsets"], ref["offsets"])
    assert not np.array_equal(last["genes"], ref["genes"])
    tie0 = sc.ref_integrate(good, poor, sc.PG, tie_value=0)
    assert not np.array_equal(tie0["freq"], ref["freq"])
