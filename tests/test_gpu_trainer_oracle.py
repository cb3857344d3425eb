"""CbowTrainer's whole training run on the device against the fp64 trainer
of trainer_cases: weights, per-epoch correct counts, stop epoch and the
weights an early stop returns, through the fast and general kernel chains,
the per-epoch hipGraph, the k-block graph and the three early-stop runners.
CPU twins: test_trainer_oracle_cpu.py."""
import pytest
import torch

import trainer_cases as tc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_training_run_matches_fp64_trainer_on_gpu(name):
    tc.check_config(name, torch.device("cuda", 0))
