"""CPU twins of test_gpu_trainer_oracle.py: the mirror trainer's whole run
against the fp64 trainer of trainer_cases, and the proof that the oracle
can tell a wrong training rule from the right one."""
import numpy as np
import pytest
import torch

import trainer_cases as tc

CPU = torch.device("cpu")


@pytest.mark.parametrize("name", list(tc.CONFIGS))
def test_training_run_matches_fp64_trainer(name):
    tc.check_config(name, CPU)


def _init(name):
    cfg = tc.make_cfg(name, CPU)
    W0, who0 = tc.replica_init(int(cfg.seed), 0, tc.G, cfg.hidden, CPU)
    return W0.numpy(), who0.numpy(), int(cfg.seed)


@pytest.mark.parametrize("variant", ["inv_b_P", "no_bias_corr", "eps_in_sqrt",
                                     "acc_before", "dip_weights"])
def test_wrong_oracles_are_caught(variant):
    """Each deliberately wrong rule must leave the true oracle by more than
    10 x the bound, or by a count, on the fixtures the tests use."""
    caught = []
    for name in ("full_eager", "b97", "es_train"):
        W0, who0, seed = _init(name)
        okw = dict(tc.CONFIGS[name][2])
        right = tc.oracle(W0, who0, seed, **okw)
        wrong = tc.oracle(W0, who0, seed, variant=variant, **okw)
        dW = float(np.abs(wrong["W_final"] - right["W_final"]).max())
        counts = (wrong["val"] != right["val"] or wrong["tr"] != right["tr"]
                  or wrong["stop_epoch"] != right["stop_epoch"])
        print(f"{variant} on {name}: max|dW|={dW:.2e} counts differ={counts}")
        caught.append(dW > 10 * tc.BOUND or counts)
    if variant == "inv_b_P":
        # 1/P only differs from 1/P_train where the batch is the split
        assert caught[0] and caught[2]
    elif variant == "dip_weights":
        assert caught[2]                 # needs an early stop
    else:
        assert all(caught)
