"""Fixtures shared by the runner-equivalence tests (CPU, GPU, replicas):
small seeded path sets whose synchronous run dips at a known epoch."""
import numpy as np
import torch

from g2vec_amd.config import G2VecConfig
from g2vec_amd.paths import PathSet

# name -> (data rng seed, genes, paths, trainer seed, CPU sync stop epoch)
FIXTURES = {
    "A": (3, 40, 120, 1, 10),   # dip in a later block for k = 2, 3, 8
    "B": (9, 60, 240, 2, 1),    # dip in the first block
    "C": (7, 30, 120, 1, 3),
}
EPOCHS = 40


def quiet(*a, **k):
    pass


def pathset(rng_seed, G, P, device=torch.device("cpu")) -> PathSet:
    rng = np.random.default_rng(rng_seed)
    genes, offs, labels = [], [0], []
    for _ in range(P):
        L = int(rng.integers(1, 14))
        genes += rng.choice(G, L, replace=False).tolist()
        offs.append(offs[-1] + L)
        labels.append(float(rng.integers(0, 2)))
    return PathSet(torch.tensor(genes, dtype=torch.int32, device=device),
                   torch.tensor(offs, dtype=torch.int32, device=device),
                   torch.tensor(labels, device=device), G)


def fixture(name, device=torch.device("cpu"), **cfg_kw):
    """(path set, config) of one named fixture."""
    rng_seed, G, P, seed, _stop = FIXTURES[name]
    kw = dict(hidden=64, epochs=EPOCHS, seed=seed, device=device.type)
    kw.update(cfg_kw)
    return pathset(rng_seed, G, P, device), G2VecConfig(**kw)


def sync_reference(tr, st, n_epochs, early_stop=True):
    """run_epoch loop with the reference dip rule applied here: (val
    history with the dip epoch, stop epoch, last-good W clone)."""
    hist, before, keep = [], -1.0, st.W.clone()
    for e in range(n_epochs):
        _a_tr, a_val = tr.run_epoch(st)
        hist.append(a_val)
        if early_stop and a_val < before:
            return hist, e - 1, keep
        before = a_val
        keep.copy_(st.W)
    return hist, -1, keep
