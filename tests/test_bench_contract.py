"""bench.py contract test: the driver depends on the one-JSON-line stdout
protocol and its field set — run the real script as a subprocess on a tiny
config and validate the schema."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

BENCH = os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "bench.py")
TINY = ["--n-genes", "500", "--n-edges", "6000", "--n-extra", "50",
        "--n-modules", "6", "--reps", "2", "--len-path", "12",
        "--steps", "2", "--warmup", "1", "--acc-target-epochs", "2"]


def _run_single(extra, dump_dir):
    """One single-process run of the tiny config -> (result dict, stderr,
    {name: dumped array})."""
    out = subprocess.run(
        [sys.executable, BENCH] + TINY + extra
        + ["--dump-outputs", str(dump_dir)],
        capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.strip()]
    assert len(lines) == 1, f"stdout must be ONE JSON line, got: {lines}"
    dumped = {f[:-len(".npy")]: np.load(os.path.join(dump_dir, f))
              for f in sorted(os.listdir(dump_dir))}
    return json.loads(lines[0]), out.stderr, dumped


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    return _run_single(["--full"], tmp_path_factory.mktemp("dump_full"))


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    return _run_single([], tmp_path_factory.mktemp("dump_plain"))


def test_bench_plain_run_is_lean(plain_run):
    """A plain run keeps the headline fields but runs none of the --full
    extras: no convergence probe, no warmed walk timing — and their
    config entries are absent rather than stale."""
    d, err, _ = plain_run
    assert d["metric"] == "cbow_paths_per_sec" and d["unit"] == "paths/s"
    assert d["higher_is_better"] is True and d["dtype"] == "fp32"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step describe the same timed steps (both rounded:
    # ms_per_step to 1e-3 ms, which is a few % of a tiny-config GPU epoch)
    assert d["value"] == pytest.approx(
        d["config"]["global_batch"] / (d["ms_per_step"] * 1e-3), rel=0.05)
    for key in ("val_acc", "wall_to_val_acc_0.88_s", "conv_runs",
                "conv_seeds", "walks_per_sec"):
        assert key not in d["config"], key
    assert "conv seed" not in err


def test_bench_dump_outputs(plain_run, full_run):
    """--dump-outputs writes what the timed path returned after its last
    step, as float arrays, and the seeded inputs make it reproducible:
    the --full extras run before the timed region on other trainers, so
    a plain and a --full run must dump identical arrays."""
    d, _, got = plain_run
    G, h, steps = 500, d["config"]["hidden"], d["steps"]
    assert set(got) == {"W_ih", "W_ho", "acc_val_history", "acc_train_last"}
    assert got["W_ih"].shape == (G, h) and got["W_ih"].dtype == np.float32
    assert got["W_ho"].shape == (h,) and got["W_ho"].dtype == np.float32
    assert got["acc_val_history"].shape == (steps,)   # one per timed step
    assert got["acc_val_history"].dtype == np.float64
    assert got["acc_train_last"].shape == (1,)
    assert got["acc_train_last"].dtype == np.float64
    for name, a in got.items():
        assert np.isfinite(a).all(), name
    assert got["W_ih"].std() > 0 and np.abs(got["W_ho"]).max() > 0
    assert (got["acc_val_history"] > 0).all()
    assert (got["acc_val_history"] <= 1).all()
    assert 0 < got["acc_train_last"][0] <= 1
    _, _, ref = full_run
    assert set(ref) == set(got)
    for name, a in got.items():
        assert np.array_equal(a, ref[name]), name


@pytest.mark.timeout(600)
def test_bench_json_contract(full_run):
    d, _, _ = full_run

    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in d, key
    assert d["metric"] == "cbow_paths_per_sec"
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["vs_baseline"] == pytest.approx(d["value"] / 16500.0, rel=0.01)
    cfg = d["config"]
    for key in ("model", "global_batch", "seq_len", "parallelism", "val_acc",
                "walks_per_sec"):
        assert key in cfg, key
    assert cfg["parallelism"] == "dp1"
    assert "synthetic" in d["data"]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.timeout(600)
def test_bench_torchrun_dp2_contract(plain_run):
    """The driver's SCALE launch path: torch.distributed.run with 2 ranks
    must still produce ONE valid JSON line from rank 0. The backend is
    pinned to gloo so the two ranks run wherever the suite does: on CPU,
    or sharing the GPUs that are there (RCCL refuses two ranks on one
    device, and this test is about the launch path, not the fabric)."""
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(_free_port()), BENCH, "--gpus", "2"] + TINY,
        env=dict(os.environ, G2VEC_DIST_BACKEND="gloo"),
        capture_output=True, text=True, timeout=500)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines()
             if l.strip().startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected: {lines}"
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0
    # C5 weak scaling: one shared study at num_repetition = reps x world;
    # the global batch must come from the GLOBAL dedup of both ranks'
    # source-sharded walks (reps x world > reps of a single rank's set)
    assert d["config"]["num_repetition_global"] == 4
    d1 = plain_run[0]      # the single-process run of the same arguments
    # same study at 2x the walk budget: strictly more unique paths, and
    # roughly linear growth (dedup saturation would show up here)
    assert d["config"]["global_batch"] > 1.5 * d1["config"]["global_batch"]
