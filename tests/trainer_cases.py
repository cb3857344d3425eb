"""An fp64 trainer, written from the reference net's definition, and the
checks that hold CbowTrainer's whole training run to it: N-epoch weight
trajectories, per-epoch correct counts, the stop epoch and the weights an
early stop returns. Shared by test_trainer_oracle_cpu.py (CPU mirror) and
test_gpu_trainer_oracle.py (HIP kernels, hipGraph and the epoch runners).

The oracle is plain NumPy fp64 on a dense multi-hot X[P, G]; it shares no
code with g2vec_amd.ops.cpu_ref or the trainer. It takes the initial weights
as inputs (replicate_cases.replica_init draws them the way the trainer does
on that device; trunc_normal_ has its own parity tests).

The bound is measured, not chosen
---------------------------------
measure_mirror() runs the CPU mirror trainer of every configuration against
the oracle (each from the mirror's own initial weights) and reports
max|W - W64| and max|o - o64|. The bound that mirror and kernels alike must
keep is 4 x the largest mirror deviation over all configurations, the factor
perm_cases uses between its mirror and its kernel. Figures of the run that
set the constants below (CPU mirror, 8 epochs unless named otherwise; who
only where the driver exposes it, H only on the general path):

    configuration        |W-W64| |who-who64|   |o-o64|   |H-H64|
    full_graph          6.42e-08          -   4.74e-07         -
    full_eager          6.42e-08          -   4.74e-07         -
    run_epoch_graph     6.42e-08   2.68e-08   4.74e-07         -
    run_epoch_eager     6.42e-08   2.68e-08   4.74e-07         -
    b97                 1.83e-07          -   1.91e-06         -
    general_none        6.42e-08          -   4.74e-07  2.82e-07
    general_relu        2.22e-07          -   2.82e-07  3.14e-07
    general_b97         6.20e-07          -   1.97e-06  7.30e-07
    general_relu_b97    2.14e-07          -   1.21e-06  3.82e-07
    general_run_epoch   6.42e-08   2.68e-08   4.74e-07  2.82e-07
    relabel             6.42e-08          -   3.55e-07         -
    h128                5.68e-08          -   6.37e-07         -
    es_train            4.18e-08          -   2.21e-07         -
    es_pipelined        4.18e-08   1.52e-08   2.21e-07         -
    es_kgranular        4.18e-08          -   2.21e-07         -
    es_sync_general     4.18e-08          -   1.98e-07  2.32e-07
    kblock20 (20 ep.)   1.26e-07   4.86e-08   1.33e-06         -

MI355X, test_gpu_trainer_oracle.py (the device's own seeds and initial
weights), max|W - W64|: full / run_epoch / general_none / relabel 3.30e-07,
b97 1.32e-06 (the largest), general_b97 1.29e-06, general_relu 4.58e-07,
general_relu_b97 1.12e-06, h128 3.08e-07, es_* 1.24e-07, kblock20
8.08e-07; max|who - who64| 1.10e-07 to 5.88e-07 (kblock20).

`PYTHONPATH=. python tests/trainer_cases.py` prints the mirror's table again;
measure_mirror() runs on one thread so that the figures can be reproduced. The
logit deviation is mostly the weight deviation carried through the forward
(up to 14 genes x 64 columns), which is why it exceeds max|W - W64|.

Fixture conditions (check_fixture_conditions, from the oracle alone)
--------------------------------------------------------------------
* No Adam sign ambiguity: at step 1 the update is lr sign(g), so a gradient
  that cancels to within f32 rounding may flip and move a weight by 2 lr.
  Required at every step and for every gene g the batch touches:
  |c_g| >= n_g 2^-22 sum|dO_p| over the batch's paths that hold g (4 x the
  f32 summation bound). An entry that fails is left out of the weight
  comparison; at most 2% of the touched entries may be, and the chosen
  seeds need none on the linear net. The first who step is held to the
  same requirement (no exclusion there).
* ReLU only: a hidden unit with |H64| < 10 M_H may take the other branch in
  f32, which changes dW[g, j] of every gene on that path by a whole term.
  Those entries (about 1% here) are left out under the same 2% cap.
* No undecided path: |o64| >= 10 M_O for every path at every epoch; then
  correct counts and the stop epoch must equal the oracle's exactly.
* Early-stop runs: the oracle's validation count drops by >= 2 paths.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from g2vec_amd.config import G2VecConfig
from g2vec_amd.models.cbow import CbowTrainer
from g2vec_amd.paths import PathSet
from replicate_cases import replica_init

G, P = 200, 400
N_TR = int(0.8 * P)
N_VL = P - N_TR
EPOCHS = 8
LR = 0.005
B1, B2, EPS = 0.9, 0.999, 1e-8

# measured on the CPU mirror (see the table above)
MIRROR_MAX_DW = 6.20e-7         # largest max|W - W64| over all configurations
MIRROR_MAX_DO = 1.97e-6         # largest |o - o64|
MIRROR_MAX_DH = 7.30e-7         # largest |H - H64| (general path, ReLU)
BOUND = 4 * MIRROR_MAX_DW       # mirror and kernels alike
M_O = 4 * MIRROR_MAX_DO
M_H = 4 * MIRROR_MAX_DH
SIGN_REQ = 2.0 ** -22           # 4 x the f32 summation bound n u sum|dO|

# The initial weights differ between the host sampler (CPU) and the device
# kernel, so the oracle's trajectory does too: a seed is chosen per
# configuration and per initialisation such that the fixture conditions
# hold (check_fixture_conditions asserts them on every run). (cpu, cuda)
SEEDS = {
    "default": (0, 12), "b97": (1, 0), "relu": (1, 1), "relu_b97": (1, 0),
    "h128": (2, 2), "kblock20": (0, 12), "es": (12, 12),
}


# ------------------------------------------------------------------ fixture
@functools.lru_cache(maxsize=None)
def fixture():
    """(genes i32, offsets i32, labels f32, X f64 [P,G])."""
    rng = np.random.default_rng(3)
    genes, offs, labels = [], [0], []
    for _ in range(P):
        n = int(rng.integers(1, 15))
        genes += rng.choice(G, size=n, replace=False).tolist()
        offs.append(offs[-1] + n)
        labels.append(float(rng.integers(0, 2)))
    X = np.zeros((P, G), dtype=np.float64)
    for p in range(P):
        X[p, genes[offs[p]:offs[p + 1]]] = 1.0
    return (np.asarray(genes, dtype=np.int32), np.asarray(offs, dtype=np.int32),
            np.asarray(labels, dtype=np.float32), X)


def pathset(device) -> PathSet:
    g, o, l, _X = fixture()
    return PathSet(torch.from_numpy(g).to(device), torch.from_numpy(o).to(device),
                   torch.from_numpy(l).to(device), G)


def split(seed: int):
    gen = torch.Generator()
    gen.manual_seed(seed + 12345)
    perm = torch.randperm(P, generator=gen).numpy()
    return perm[:N_TR], perm[N_TR:]


# ------------------------------------------------------------------- oracle
def _sigmoid(o):
    return 1.0 / (1.0 + np.exp(-o))


def oracle(W0, who0, seed, *, epochs=EPOCHS, batch_size=0, act="none",
           early_stop=False, variant=None):
    """The reference net trained in fp64. variant names a deliberately
    wrong rule (test_wrong_oracles_are_caught): 'inv_b_P', 'no_bias_corr',
    'eps_in_sqrt', 'acc_before', 'dip_weights'."""
    _g, _o, labels, X = fixture()
    y = labels.astype(np.float64)
    tr_idx, vl_idx = split(seed)
    Xtr, ytr, Xvl, yvl = X[tr_idx], y[tr_idx], X[vl_idx], y[vl_idx]
    W, who = W0.astype(np.float64).copy(), who0.astype(np.float64).copy()
    mW, vW, mO, vO = (np.zeros_like(W), np.zeros_like(W),
                      np.zeros_like(who), np.zeros_like(who))
    relu = act == "relu"
    bs = batch_size if batch_size > 0 else N_TR

    def logits(Xs):
        H = Xs @ W
        return (np.maximum(H, 0.0) if relu else H) @ who, H

    def counts():
        o_tr, H_tr = logits(Xtr)
        o_vl, H_vl = logits(Xvl)
        return (int(np.sum((o_tr > 0) == (ytr > 0.5))),
                int(np.sum((o_vl > 0) == (yvl > 0.5))),
                np.concatenate([o_tr, o_vl]),
                min(np.abs(H_tr).min(), np.abs(H_vl).min()))

    t = 0
    out = dict(val=[], tr=[], o=[], W=[], who=[], min_abs_o=np.inf,
               min_ratio=np.inf, min_ratio_who=np.inf, n_kink=0,
               excluded=np.zeros(W.shape, dtype=bool),
               touched=np.zeros(G, dtype=bool))
    stop_epoch = -1
    for e in range(epochs):
        pre = counts() if variant == "acc_before" else None
        for lo in range(0, N_TR, bs):
            Xb, yb = Xtr[lo:lo + bs], ytr[lo:lo + bs]
            inv_b = 1.0 / (P if variant == "inv_b_P" else Xb.shape[0])
            H = Xb @ W
            A = np.maximum(H, 0.0) if relu else H
            dO = (_sigmoid(A @ who) - yb) * inv_b
            g_who = A.T @ dO
            dH = np.outer(dO, who)
            if relu:
                dH = dH * (H > 0)
            g_W = Xb.T @ dH
            # --- fixture condition: no gradient cancels to f32 rounding.
            # dW[g, j] = who_j * sum over the batch's paths holding g of
            # dO_p (times the ReLU mask): n_g terms, f32 summation bound
            # n_g u sum|dO_p|; 4 x that is required of |c_g|
            n_g = Xb.sum(axis=0)
            sum_abs = Xb.T @ np.abs(dO)          # over the paths that hold g
            if relu:
                mask = (H > 0).astype(np.float64)
                c = Xb.T @ (dO[:, None] * mask)                 # [G, h]
                live = (Xb.T @ mask) > 0         # else exactly 0 either way
                ratio = np.where(live, np.abs(c) / np.maximum(
                    (n_g * sum_abs)[:, None], 1e-300), np.inf)
                # a hidden unit on the kink may take the other ReLU branch
                # in f32, which moves dW[g, j] of its path's genes
                kink = (np.abs(H) < 10 * M_H).astype(np.float64)
                out["n_kink"] += int(kink.sum())
                out["excluded"] |= (Xb.T @ kink) > 0
            else:
                c = Xb.T @ dO
                ratio = np.where(n_g > 0, np.abs(c) / np.maximum(
                    n_g * sum_abs, 1e-300), np.inf)[:, None]
            out["touched"] |= n_g > 0
            out["excluded"] |= np.broadcast_to(ratio < SIGN_REQ, W.shape)
            out["min_ratio"] = min(out["min_ratio"], float(ratio.min()))
            if t == 0:
                # the first who step is lr sign(g) too; both summation
                # routes of the trainer: over paths, and W^T c over genes
                r1 = np.abs(g_who) / (Xb.shape[0] * np.abs(
                    A * dO[:, None]).sum(axis=0))
                out["min_ratio_who"] = float(r1.min())
                if not relu:
                    r2 = np.abs(g_who) / (G * np.abs(
                        W * (Xb.T @ dO)[:, None]).sum(axis=0))
                    out["min_ratio_who"] = float(min(r1.min(), r2.min()))
            # --- TF1 Adam, one t per optimizer step
            t += 1
            lr_t = LR * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t)
            if variant == "no_bias_corr":
                lr_t = LR
            for p_, m_, v_, g_ in ((W, mW, vW, g_W), (who, mO, vO, g_who)):
                m_ *= B1
                m_ += (1.0 - B1) * g_
                v_ *= B2
                v_ += (1.0 - B2) * g_ * g_
                if variant == "eps_in_sqrt":
                    p_ -= lr_t * m_ / np.sqrt(v_ + EPS)
                else:
                    p_ -= lr_t * m_ / (np.sqrt(v_) + EPS)
        c_tr, c_vl, o_all, min_h = counts() if pre is None else pre
        out["tr"].append(c_tr)
        out["val"].append(c_vl)
        out["o"].append(o_all)
        out["W"].append(W.copy())
        out["who"].append(who.copy())
        out["min_abs_o"] = min(out["min_abs_o"], float(np.abs(o_all).min()))
        if early_stop and e > 0 and c_vl < out["val"][-2]:
            stop_epoch = e - 1
            break
    out["stop_epoch"] = stop_epoch
    out["epochs_run"] = len(out["val"])
    rep = stop_epoch if stop_epoch >= 0 else out["epochs_run"] - 1
    if variant == "dip_weights" and stop_epoch >= 0:
        out["W_final"], out["who_final"] = out["W"][-1], out["who"][-1]
    else:
        out["W_final"], out["who_final"] = out["W"][rep], out["who"][rep]
    out["reported"] = rep
    return out


def check_fixture_conditions(orc, need_dip=False):
    """Asserted from the oracle alone, so that a bad seed fails loudly
    instead of hiding a difference."""
    n_ex = int(orc["excluded"].sum())
    n_t = int(orc["touched"].sum()) * orc["excluded"].shape[1]
    assert n_ex <= 0.02 * n_t, (n_ex, n_t, orc["min_ratio"], orc["n_kink"])
    assert orc["min_ratio_who"] >= SIGN_REQ, orc["min_ratio_who"]
    assert orc["min_abs_o"] >= 10 * M_O, (orc["min_abs_o"], 10 * M_O)
    if need_dip:
        s = orc["stop_epoch"]
        assert s >= 0, f"the oracle does not stop: {orc['val']}"
        assert orc["val"][s] - orc["val"][s + 1] >= 2, orc["val"]


# ----------------------------------------------------------- configurations
# name -> (G2VecConfig overrides, driver, oracle keywords)
# driver: 'train' = CbowTrainer.train; 'run_epoch' = setup + run_epoch loop
# (exposes who and the train counts of every epoch); 'pipelined' = setup +
# run_epochs_pipelined
CONFIGS = {
    # 1. fast path, full batch, fixed epochs. Through train() an 8-epoch
    # fixed run is one warm epoch plus seven eager bodies whatever
    # use_hipgraph says (the k-block graph of 8 is recorded, never
    # replayed), so full_graph and full_eager run the same kernels; a graph
    # is replayed only by run_epoch_graph (per-epoch hipGraph), the early-
    # stop runners and kblock20, and the first and last assert that it was
    "full_graph": (dict(use_hipgraph=True), "train", {}),
    "full_eager": (dict(use_hipgraph=False), "train", {}),
    "run_epoch_graph": (dict(use_hipgraph=True), "run_epoch", {}),
    "run_epoch_eager": (dict(use_hipgraph=False), "run_epoch", {}),
    # 2. fast path, batches of 97, 97, 97, 29
    "b97": (dict(batch_size=97), "train", dict(batch_size=97)),
    # 3. general path, fp32
    "general_none": (dict(trainer_path="general"), "train", {}),
    "general_relu": (dict(trainer_path="general", activation="relu"), "train",
                     dict(act="relu")),
    "general_b97": (dict(trainer_path="general", batch_size=97), "train",
                    dict(batch_size=97)),
    "general_relu_b97": (dict(trainer_path="general", activation="relu",
                              batch_size=97), "train",
                         dict(act="relu", batch_size=97)),
    "general_run_epoch": (dict(trainer_path="general"), "run_epoch", {}),
    # 4. gene relabelling: W_ih comes back in the original gene order
    "relabel": (dict(gene_relabel="on"), "train", {}),
    "h128": (dict(hidden=128), "train", {}),
    # 5. early stop through the three runners (+ the pipelined runner
    # called directly, which is what train() uses on the device)
    "es_train": (dict(early_stop=True), "train",
                 dict(early_stop=True)),
    "es_pipelined": (dict(early_stop=True), "pipelined",
                     dict(early_stop=True)),
    "es_kgranular": (dict(early_stop=True, earlystop_every=4),
                     "train", dict(early_stop=True)),
    "es_sync_general": (dict(early_stop=True, trainer_path="general"),
                        "train", dict(early_stop=True)),
    # 6. long enough for the k-block graph: 1 warm + 2 blocks of 8 + 3 tail
    "kblock20": (dict(epochs=20), "pipelined", dict(epochs=20)),
}


def seed_class(name) -> str:
    """Configurations that share an oracle run share a seed."""
    okw = CONFIGS[name][2]
    h = CONFIGS[name][0].get("hidden", 64)
    if okw.get("early_stop"):
        return "es"
    if h != 64:
        return "h128"
    if okw.get("epochs", EPOCHS) != EPOCHS:
        return "kblock20"
    parts = [okw["act"]] if "act" in okw else []
    parts += ["b97"] if okw.get("batch_size") else []
    return "_".join(parts) or "default"


def make_cfg(name, device) -> G2VecConfig:
    seed = SEEDS.get(seed_class(name), SEEDS["default"])[
        0 if device.type == "cpu" else 1]
    kw = dict(hidden=64, epochs=EPOCHS, lr=LR, early_stop=False, seed=seed,
              device=device.type, dtype="fp32", gene_relabel="off")
    kw.update(CONFIGS[name][0])
    return G2VecConfig(**kw)


_ORACLES = {}


def oracle_for(name, device):
    cfg = make_cfg(name, device)
    okw = dict(CONFIGS[name][2])
    key = (device.type, cfg.seed, cfg.hidden, tuple(sorted(okw.items())))
    if key not in _ORACLES:
        W0, who0 = replica_init(int(cfg.seed), 0, G, cfg.hidden, device)
        _ORACLES[key] = oracle(W0.cpu().numpy(), who0.cpu().numpy(),
                               int(cfg.seed), **okw)
    return _ORACLES[key]


def run_config(name, device):
    """Drive the trainer; returns dict(W, who|None, val counts, tr counts|
    None, final tr/val counts, stop_epoch, epochs_run, st)."""
    quiet = lambda *a, **k: None   # noqa: E731
    cfg = make_cfg(name, device)
    driver = CONFIGS[name][1]
    ps = pathset(device)
    tr = CbowTrainer(cfg, G, device, log=quiet)
    cnt = lambda a, n: int(round(a * n))   # noqa: E731
    if driver == "train":
        res = tr.train(ps)
        return dict(W=res.W_ih, who=None, stop_epoch=res.stop_epoch,
                    epochs_run=res.epochs_run,
                    val=[cnt(a, N_VL) for a in res.acc_val_history], tr=None,
                    tr_final=cnt(res.acc_tr, N_TR),
                    val_final=cnt(res.acc_val, N_VL), st=None)
    st = tr.setup(ps)
    if driver == "run_epoch":
        accs = [tr.run_epoch(st) for _ in range(cfg.epochs)]
        return dict(W=tr._unrelabel(st.W), who=st.who, stop_epoch=-1,
                    epochs_run=cfg.epochs, val=[cnt(a[1], N_VL) for a in accs],
                    tr=[cnt(a[0], N_TR) for a in accs],
                    tr_final=cnt(accs[-1][0], N_TR),
                    val_final=cnt(accs[-1][1], N_VL), st=st)
    tr_hist = []
    hist, stop, W, who, _a = tr.run_epochs_pipelined(
        st, cfg.epochs, cfg.early_stop,
        on_epoch=lambda e, a_tr, a_val: tr_hist.append(a_tr))
    rep = stop if stop >= 0 else len(hist) - 1
    return dict(W=tr._unrelabel(W), who=who, stop_epoch=stop,
                epochs_run=len(hist), val=[cnt(a, N_VL) for a in hist],
                tr=[cnt(a, N_TR) for a in tr_hist],
                tr_final=cnt(tr_hist[rep], N_TR), val_final=cnt(hist[rep], N_VL),
                st=st)


def deviations(got, orc):
    keep = ~orc["excluded"]
    dW = float(np.abs(got["W"].detach().cpu().numpy().astype(np.float64)
                      - orc["W_final"])[keep].max())
    dwho = None
    if got["who"] is not None:
        dwho = float(np.abs(got["who"].detach().cpu().numpy().astype(np.float64)
                            - orc["who_final"]).max())
    return dW, dwho


def check_config(name, device):
    """One configuration on `device` against the oracle. Returns the
    deviations (dW, dwho) so that callers can report them."""
    cfg = make_cfg(name, device)
    orc = oracle_for(name, device)
    check_fixture_conditions(orc, need_dip=cfg.early_stop)
    got = run_config(name, device)
    dW, dwho = deviations(got, orc)
    n_ex = int(orc["excluded"].sum())
    n_t = int(orc["touched"].sum()) * orc["excluded"].shape[1]
    print(f"trainer-oracle {device.type} {name}: excluded {n_ex} of {n_t} "
          f"touched entries ({100.0 * n_ex / n_t:.2f}%), "
          f"{orc['n_kink']} units on the ReLU kink")
    if cfg.activation != "relu":
        assert n_ex == 0, (name, n_ex)      # the linear seeds need none
    print(f"trainer-oracle {device.type} {name}: max|W-W64|={dW:.3e} "
          f"max|who-who64|={dwho if dwho is None else format(dwho, '.3e')} "
          f"val={got['val']} stop={got['stop_epoch']} "
          f"min|o64|={orc['min_abs_o']:.2e} min_ratio={orc['min_ratio']:.2e}")
    assert got["stop_epoch"] == orc["stop_epoch"]
    assert got["epochs_run"] == orc["epochs_run"]
    assert got["val"] == orc["val"], (got["val"], orc["val"])
    if got["tr"] is not None:
        assert got["tr"] == orc["tr"], (got["tr"], orc["tr"])
    rep = orc["reported"]
    assert got["tr_final"] == orc["tr"][rep]
    assert got["val_final"] == orc["val"][rep]
    assert dW <= BOUND, (name, dW, BOUND)
    if dwho is not None:
        assert dwho <= BOUND, (name, dwho, BOUND)
    if name == "run_epoch_graph" and device.type == "cuda":
        assert got["st"].graph is not None, "per-epoch hipGraph not captured"
    if name == "kblock20" and device.type == "cuda":
        assert getattr(got["st"], "kgraph", None) is not None, \
            "k-block graph not used"
    return dW, dwho


# ------------------------------------------------------ measuring the mirror
def mirror_forward_deviation(name):
    """(max|o32 - o64|, max|H32 - H64|) over the epochs of a run_epoch-
    driven CPU mirror run: o32 / H32 are the f32 forward of the mirror's
    weights after that epoch, o64 / H64 the oracle's. H only on the general
    path (the fast path has no hidden layer)."""
    cpu = torch.device("cpu")
    cfg = make_cfg(name, cpu)
    orc = oracle_for(name, cpu)
    _g, _o, _l, X = fixture()
    tr_idx, vl_idx = split(int(cfg.seed))
    X64 = X[np.concatenate([tr_idx, vl_idx])]
    X32 = torch.from_numpy(X64).float()
    tr = CbowTrainer(cfg, G, cpu, log=lambda *a, **k: None)
    st = tr.setup(pathset(cpu))
    d_o = d_h = 0.0
    for e in range(orc["epochs_run"]):
        tr.run_epoch(st)
        W = tr._unrelabel(st.W)
        if cfg.trainer_path == "general":
            H = X32 @ W
            o32 = (torch.relu(H) if cfg.activation == "relu" else H) @ st.who
            d_h = max(d_h, float(np.abs(H.double().numpy()
                                        - X64 @ orc["W"][e]).max()))
        else:
            o32 = X32 @ torch.mv(W, st.who)
        d_o = max(d_o, float(np.abs(o32.double().numpy()
                                    - orc["o"][e]).max()))
    return d_o, d_h


def measure_mirror():
    cpu = torch.device("cpu")
    rows = []
    threads = torch.get_num_threads()
    torch.set_num_threads(1)         # one summation order: reproducible
    try:
        for name in CONFIGS:
            got = run_config(name, cpu)
            dW, dwho = deviations(got, oracle_for(name, cpu))
            d_o, d_h = mirror_forward_deviation(name)
            rows.append((name, dW, dwho or 0.0, d_o, d_h))
    finally:
        torch.set_num_threads(threads)
    return rows


if __name__ == "__main__":
    rows = measure_mirror()
    print(f"{'configuration':18s} {'|W-W64|':>9s} {'|who-who64|':>11s} "
          f"{'|o-o64|':>9s} {'|H-H64|':>9s}")
    for r in rows:
        print(f"{r[0]:18s} {r[1]:9.2e} {r[2]:11.2e} {r[3]:9.2e} {r[4]:9.2e}")
    w, o, h = (max(r[i] for r in rows) for i in (1, 3, 4))
    print(f"MIRROR_MAX_DW = {w:.2e}  -> BOUND = {4 * w:.2e}")
    print(f"MIRROR_MAX_DO = {o:.2e}  -> M_O = {4 * o:.2e}")
    print(f"MIRROR_MAX_DH = {h:.2e}  -> M_H = {4 * h:.2e}")
