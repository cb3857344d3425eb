"""The epoch runners against each other on the CPU: transcript, result,
callback sequence, collective schedule and checkpoint format of every way
to run the fast full-batch epoch. Written against the trainer before its
runners were folded onto one step / stop rule / reporter, so what they pin
is the behaviour, not the layout."""
import dataclasses
import re

import pytest
import torch

import runner_cases as rcase
from g2vec_amd.models.cbow import CbowTrainer
from g2vec_amd.models.replicas import ReplicaTrainer
from g2vec_amd.parallel.dist import DistContext

CPU = torch.device("cpu")
KS = (1, 2, 3, 8)


def _trainer(cfg, G, ctx=None, log=rcase.quiet):
    return CbowTrainer(cfg, G, CPU, ctx, log=log)


def _train(name, log=rcase.quiet, **cfg_kw):
    ps, cfg = rcase.fixture(name, **cfg_kw)
    return _trainer(cfg, ps.n_genes, log=log).train(ps)


# ------------------------------------------- 1. transcript + result, train()
_SEC = re.compile(r"\(\d+\.\d+ sec\)")


def _transcript_run(name, early_stop, k):
    lines = []
    res = _train(name, log=lambda s: lines.append(_SEC.sub("(T sec)", s)),
                 early_stop=early_stop, earlystop_every=k)
    assert len(res.epoch_times_s) == res.epochs_run
    return lines, res


@pytest.mark.parametrize("early_stop", (True, False))
@pytest.mark.parametrize("name", sorted(rcase.FIXTURES))
def test_train_transcript_and_result_identity(name, early_stop):
    ref_lines, ref = _transcript_run(name, early_stop, 1)
    if early_stop:
        # the fixtures' preconditions (runner_cases.FIXTURES has the epochs
        # measured): A dips in a later block for every k, so a replay is
        # needed; B dips inside the first block of every k > 1
        assert ref.stop_epoch >= {"A": 8, "B": 0, "C": 0}[name]
        if name == "B":
            assert ref.stop_epoch + 1 <= 2
    else:
        assert ref.stop_epoch == -1 and ref.epochs_run == rcase.EPOCHS
    key = lambda r: (r.stop_epoch, r.acc_val, r.acc_tr,     # noqa: E731
                     r.epochs_run, r.acc_val_history)
    for k in KS[1:]:
        lines, res = _transcript_run(name, early_stop, k)
        assert lines == ref_lines, k
        assert key(res) == key(ref), k
        assert torch.equal(res.W_ih, ref.W_ih), k


# ------------------------------------------ 2. runner identity below train()
@pytest.mark.parametrize("relabel", ("off", "on"))
def test_runner_identity_below_train(relabel):
    ps, cfg = rcase.fixture("A", early_stop=True, gene_relabel=relabel)
    ref = _trainer(cfg, ps.n_genes).train(ps)
    assert ref.stop_epoch >= 8

    def run(method, *args):
        tr = _trainer(cfg, ps.n_genes)
        st = tr.setup(ps)
        assert (tr.gene_order is not None) == (relabel == "on")
        calls = []
        hist, stop, W, _who, _a = getattr(tr, method)(
            st, cfg.epochs, *args,
            on_epoch=lambda e, a_tr, a_val: calls.append((e, a_tr, a_val)))
        assert hist == ref.acc_val_history
        assert stop == ref.stop_epoch
        assert torch.equal(tr._unrelabel(W), ref.W_ih)
        assert calls[-1][0] == ref.stop_epoch + 1       # ends at the dip
        assert [c[0] for c in calls] == list(range(len(hist)))
        assert [c[2] for c in calls] == hist
        return calls

    calls = run("run_epochs_pipelined", True)
    for k in KS:
        assert run("run_epochs_kgranular", k) == calls, k


# ------------------------------------------- 3. fixed-epoch deferred runner
def test_fixed_epoch_deferred_runner_and_buffer_reuse():
    ps, cfg = rcase.fixture("A", early_stop=False)
    tr1 = _trainer(cfg, ps.n_genes)
    st1 = tr1.setup(ps)
    sync = [tr1.run_epoch(st1)[1] for _ in range(29)]
    tr2 = _trainer(cfg, ps.n_genes)
    st2 = tr2.setup(ps)
    assert tr2.kblock_eligible(st2, 29, False)
    hist, stop, W, _who, _a = tr2.run_epochs_pipelined(st2, 29, False)
    assert stop == -1 and hist == sync
    assert torch.equal(W, st1.W)
    # a second call at another length (no warm epoch, reused run buffers)
    sync += [tr1.run_epoch(st1)[1] for _ in range(5)]
    hist2, stop2, W2, _who, _a = tr2.run_epochs_pipelined(st2, 5, False)
    assert stop2 == -1 and hist + hist2 == sync
    assert torch.equal(W2, st1.W)
    assert st2.epoch_idx == st1.epoch_idx == 34
    assert st2.t_adam == st1.t_adam == 34


# ------------------------------------- 4. collective schedule, one process
class _RecordingCtx(DistContext):
    """Records (method, numel) of every collective before delegating; at
    world=1 the parent returns early, the call still comes through here."""

    def __init__(self):
        super().__init__(0, 1, CPU, False)
        self.calls = []

    def allreduce_(self, t):
        self.calls.append(("allreduce_", t.numel()))
        return super().allreduce_(t)

    def allreduce_max_(self, t):
        self.calls.append(("allreduce_max_", t.numel()))
        return super().allreduce_max_(t)

    def broadcast_(self, t, src=0):
        self.calls.append(("broadcast_", t.numel()))
        return super().broadcast_(t, src)


_G, _H = 40, 64
_SETUP = [("broadcast_", _G * _H), ("broadcast_", _H)]
_EPOCH = [("allreduce_", _G), ("allreduce_", 2)]     # grad c + metric counts
_BODY = [("allreduce_", _G)]                         # deferred-metric body
# Fixture A stops at epoch 10: 12 epochs run (0..11), the dip is epoch 11
SCHEDULES = {
    "train_sync": _SETUP + _EPOCH * 12,
    # speculative: epoch 12 is queued before epoch 11's dip is read
    "pipelined_early_stop": _EPOCH * 13,
    # one warm epoch, 39 deferred bodies, ONE history reduce
    "pipelined_fixed": _EPOCH + _BODY * 39 + [("allreduce_", 2 * 39)],
    # warm epoch, blocks 1-3 4-6 7-9 10-12, dip at 11: replay epoch 10
    "kgranular_3": (_EPOCH + (_BODY * 3 + [("allreduce_", 6)]) * 4
                    + _BODY * 1),
    # warm epoch, blocks 1-8 9-16, dip at 11: replay epochs 9, 10
    "kgranular_8": (_EPOCH + (_BODY * 8 + [("allreduce_", 16)]) * 2
                    + _BODY * 2),
    "kgranular_1": _EPOCH + (_BODY + [("allreduce_", 2)]) * 11,
}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_collective_schedule_single_process(name):
    early = name != "pipelined_fixed"
    ps, cfg = rcase.fixture("A", early_stop=early)
    ctx = _RecordingCtx()
    tr = _trainer(cfg, ps.n_genes, ctx)
    if name == "train_sync":
        assert tr.train(ps).stop_epoch == 10
    else:
        st = tr.setup(ps)
        assert ctx.calls == _SETUP
        del ctx.calls[:]
        if name.startswith("kgranular"):
            out = tr.run_epochs_kgranular(st, cfg.epochs,
                                          int(name.rsplit("_", 1)[1]))
        else:
            out = tr.run_epochs_pipelined(st, cfg.epochs, early)
        assert out[1] == (10 if early else -1)
    assert ctx.calls == SCHEDULES[name]


# ------------------------------------------------------ 5. checkpoint format
BLOB_KEYS = {"W", "who", "mW", "vW", "mO", "vO", "W_keep", "dO_buf",
             "t_adam", "epoch_idx", "fingerprint"}
FINGERPRINT_KEYS = {"n_genes", "hidden", "seed", "lr", "trainer_path",
                    "world", "rank"}


def test_checkpoint_format(tmp_path):
    ps, cfg = rcase.fixture("C", early_stop=False)
    tr = _trainer(cfg, ps.n_genes)
    st = tr.setup(ps)
    for _ in range(3):
        tr.run_epoch(st)
    path = str(tmp_path / "s.pt")
    extra = {"acc_hist": [0.5], "before_val": 0.5, "before_tr": 0.25}
    tr.save_train_state(st, path, extra)
    blob = torch.load(path, map_location="cpu", weights_only=False)
    assert set(blob) == BLOB_KEYS | set(extra)
    assert set(blob["fingerprint"]) == FINGERPRINT_KEYS
    assert blob["fingerprint"] == {
        "n_genes": 30, "hidden": 64, "seed": 1, "lr": cfg.lr,
        "trainer_path": cfg.trainer_path, "world": 1, "rank": 0}
    assert (blob["t_adam"], blob["epoch_idx"]) == (3, 3)
    for name in ("W", "who", "mW", "vW", "mO", "vO", "W_keep", "dO_buf"):
        assert torch.equal(blob[name], vars(st)[name]), name

    # the blob restores a fresh state to the saved one, s_buf included
    st2 = tr.setup(ps)
    back = tr.load_train_state(st2, path)
    assert back["acc_hist"] == [0.5]
    assert (st2.t_adam, st2.epoch_idx) == (3, 3)
    for name in ("W", "who", "mW", "vW", "mO", "vO", "W_keep", "dO_buf",
                 "s_buf"):
        assert torch.equal(vars(st2)[name], vars(st)[name]), name

    bad = {"n_genes": 31, "hidden": 128, "seed": 99, "lr": 0.5,
           "trainer_path": "general"}
    for key, value in bad.items():
        forged = dict(blob, fingerprint=dict(blob["fingerprint"],
                                             **{key: value}))
        p = str(tmp_path / f"bad_{key}.pt")
        torch.save(forged, p)
        want = blob["fingerprint"][key]
        with pytest.raises(ValueError, match=re.escape(
                f"--resume-train checkpoint mismatch: {key} was {value}, "
                f"this run has {want}")):
            tr.load_train_state(st2, p)
    # world / rank are recorded, not compared
    torch.save(dict(blob, fingerprint=dict(blob["fingerprint"], world=2,
                                           rank=1)), path)
    tr.load_train_state(st2, path)


# ------------------------------------------------------ 6. declared state
def test_state_is_declared():
    ps, cfg = rcase.fixture("A", early_stop=True)
    tr = _trainer(cfg, ps.n_genes)
    st = tr.setup(ps)
    declared = {f.name for f in dataclasses.fields(st)}
    tr.run_epoch(st)
    tr.run_epochs_pipelined(st, 4, True)
    tr.run_epochs_pipelined(st, 4, False)       # deferred fixed-epoch runner
    tr.run_epochs_kgranular(st, 6, 3)
    tr._ensure_kgraph(st, k=4)
    assert set(vars(st)) <= declared
    for lazy in ("kbufs", "kgraph", "kblock_k", "run_bufs"):
        assert lazy in declared
    assert st.pipe_bufs is not None and st.pipe_bufs[0][0].numel() == 2

    rt = ReplicaTrainer(cfg, ps.n_genes, CPU, log=rcase.quiet)
    rst = rt.setup(ps, 2)
    rdeclared = {f.name for f in dataclasses.fields(rst)}
    rt.run_epoch(rst)
    assert set(vars(rst)) <= rdeclared
    assert {"R", "W", "W_keep", "graph"} <= rdeclared
