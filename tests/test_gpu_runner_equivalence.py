"""The epoch runners against each other on the device: every way to run
the fast full-batch epoch (train(), the k-granular and k-blocked runners,
the replica trainer, a resumed run) must give the run_epoch loop's history,
stop epoch and weights bit for bit. Runners are compared with each other on
the GPU only — no CPU value enters."""
import dataclasses

import pytest
import torch

import runner_cases as rcase
from g2vec_amd.config import G2VecConfig
from g2vec_amd.models.cbow import CbowTrainer
from g2vec_amd.models.replicas import ReplicaTrainer

pytestmark = pytest.mark.gpu

# The device initialises weights with its own counter-based kernel, so the
# stop epoch is not the CPU fixture's. default_rng(s), s = 0..20, was scanned
# once on an MI355X with the Fixture A recipe (G = 40, P = 120, hidden 64,
# trainer seed 1): DATA_SEED is the first whose run_epoch loop stops at an
# epoch >= 8, STOP_EPOCH that epoch.
DATA_SEED = 10
STOP_EPOCH = 8
G, P = 40, 120


def _dev():
    return torch.device("cuda", 0)


def _case(**cfg_kw):
    kw = dict(hidden=64, epochs=rcase.EPOCHS, seed=1, device="cuda",
              early_stop=True)
    kw.update(cfg_kw)
    return rcase.pathset(DATA_SEED, G, P, _dev()), G2VecConfig(**kw)


def _with_state(trainer):
    """Make trainer.train() leave its state behind: [st] after the run."""
    box, setup = [], trainer.setup

    def keeping(*a, **k):
        box.append(setup(*a, **k))
        return box[-1]
    trainer.setup = keeping
    return box


_REF = {}


def _reference(use_hipgraph):
    """The run_epoch loop with the dip rule applied here, once per mode."""
    if use_hipgraph not in _REF:
        ps, cfg = _case(use_hipgraph=use_hipgraph)
        tr = CbowTrainer(cfg, G, _dev(), log=rcase.quiet)
        st = tr.setup(ps)
        hist, stop, W = rcase.sync_reference(tr, st, cfg.epochs)
        assert (st.graph is not None) == use_hipgraph
        _REF[use_hipgraph] = (hist, stop, W)
    return _REF[use_hipgraph]


@pytest.mark.parametrize("use_hipgraph", (True, False))
def test_early_stop_runners_match_run_epoch_loop(use_hipgraph):
    hist, stop, W = _reference(use_hipgraph)
    print("reference stop epoch", stop, "epochs run", len(hist))
    assert stop == STOP_EPOCH >= 8          # the fixture's precondition
    ps, cfg = _case(use_hipgraph=use_hipgraph)

    tr = CbowTrainer(cfg, G, _dev(), log=rcase.quiet)     # pipelined runner
    box = _with_state(tr)
    res = tr.train(ps)
    assert res.acc_val_history == hist and res.stop_epoch == stop
    assert res.epochs_run == len(hist)
    assert torch.equal(res.W_ih, W)
    assert (box[0].graph is not None) == use_hipgraph
    assert box[0].pipe_bufs[0][0].is_pinned()

    # the dip is epoch 9: it opens a block for k = 2 and k = 8 (restore
    # only) and is the third epoch of one for k = 3 (restore and re-run 2)
    for k in (2, 3, 8):
        tr = CbowTrainer(cfg, G, _dev(), log=rcase.quiet)
        st = tr.setup(ps)
        h, s, Wk, _who, _a = tr.run_epochs_kgranular(st, cfg.epochs, k)
        assert h == hist and s == stop, k
        assert torch.equal(Wk, W), k
        if k == 8:      # KBLOCK: the block graph replays, else eager steps
            assert (getattr(st, "kgraph", None) is not None) == use_hipgraph

    rt = ReplicaTrainer(cfg, G, _dev(), log=rcase.quiet)
    box = _with_state(rt)
    rep0 = rt.train(ps, 2)[0]
    assert rep0.acc_val_history == hist and rep0.stop_epoch == stop
    assert torch.equal(rep0.W_ih, W)
    assert (box[0].graph is not None) == use_hipgraph


class _CountingGraph:
    def __init__(self, graph):
        self.graph, self.replays = graph, 0

    def replay(self):
        self.replays += 1
        self.graph.replay()


def test_fixed_epoch_kblocked_matches_run_epoch_loop():
    """n = 29, graphs on: one 29-epoch block after an eager warm epoch (the
    benchmark's schedule), and the default KBLOCK = 8 (1 warm epoch, 3
    blocks, 4 eager tail epochs)."""
    N = 29
    ps, cfg = _case(early_stop=False, epochs=N)
    ref = CbowTrainer(cfg, G, _dev(), log=rcase.quiet)
    st_ref = ref.setup(ps)
    sync = [ref.run_epoch(st_ref)[1] for _ in range(N)]
    W_29 = st_ref.W.clone()
    sync.append(ref.run_epoch(st_ref)[1])

    tr = CbowTrainer(cfg, G, _dev(), log=rcase.quiet)
    st = tr.setup(ps)
    assert tr.run_epoch(st)[1] == sync[0]
    tr._ensure_kgraph(st, k=tr.pick_kblock(N))
    assert st.kgraph is not None and st.kblock_k == N
    st.kgraph = counting = _CountingGraph(st.kgraph)
    hist, stop, W, _who, _a = tr.run_epochs_pipelined(st, N, False)
    assert counting.replays == 1 and stop == -1
    assert hist == sync[1:]
    assert torch.equal(W, st_ref.W)
    assert (st.epoch_idx, st.t_adam) == (N + 1, N + 1)

    tr = CbowTrainer(cfg, G, _dev(), log=rcase.quiet)
    st = tr.setup(ps)
    hist, stop, W, _who, _a = tr.run_epochs_pipelined(st, N, False)
    assert st.kgraph is not None and st.kblock_k == tr.KBLOCK == 8
    assert stop == -1 and hist == sync[:N]
    assert torch.equal(W, W_29)


def test_resume_on_gpu_is_the_uninterrupted_run(tmp_path):
    """A checkpoint at epoch 5 of 12, written by train(), resumes to the
    history and weights of the uninterrupted run."""
    ps, cfg = _case(epochs=12)
    full = CbowTrainer(cfg, G, _dev(), log=rcase.quiet).train(ps)
    ck = str(tmp_path / "state.pt")
    part = CbowTrainer(
        dataclasses.replace(cfg, epochs=5, train_ckpt=ck, train_ckpt_every=5),
        G, _dev(), log=rcase.quiet).train(ps)
    assert part.acc_val_history == full.acc_val_history[:5]
    lines = []
    resumed = CbowTrainer(dataclasses.replace(cfg, resume_train=ck), G,
                          _dev(), log=lines.append).train(ps)
    assert lines[0] == f"    (resumed training state at epoch 5 from {ck})"
    assert resumed.acc_val_history == full.acc_val_history
    assert (resumed.stop_epoch, resumed.epochs_run, resumed.acc_val,
            resumed.acc_tr) == (full.stop_epoch, full.epochs_run,
                                full.acc_val, full.acc_tr)
    assert torch.equal(resumed.W_ih, full.W_ih)
