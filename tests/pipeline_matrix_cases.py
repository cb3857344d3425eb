"""Every opt-in feature of pipeline.run at once against each feature alone.

The five features (the scores table, permutation p-values, silhouettes,
nearest-gene queries, replicates) each add files, columns and events and
leave everything else as it was, so a run with all five must reproduce every
single-feature run byte for byte. Runners: test_pipeline_matrix_cpu.py (both
base sets) and test_gpu_pipeline_matrix.py (DEV)."""
from __future__ import annotations

import json

import pytest

from g2vec_amd import pipeline
from g2vec_amd.config import G2VecConfig

HOST = {}
DEV = dict(kmeans_backend="hip", scoring_backend="device",
           score_stat="ranksum")
FEATURES = {"write_scores": dict(write_scores=True),
            "permutations": dict(permutations=20),
            "silhouette": dict(silhouette=True),
            "neighbors": dict(neighbors=5),
            "replicates": dict(replicates=2)}
TRIPLE = ("_biomarkers.txt", "_lgroups.txt", "_vectors.txt")
EXTRA_FILES = ("_neighbors.txt", "_stability.txt",
               "_consensus_biomarkers.txt")


def _cfg(files: dict, tmp_path, device: str, name: str, **kw) -> G2VecConfig:
    return G2VecConfig(expression_file=files["expression"],
                       clinical_file=files["clinical"],
                       network_file=files["network"],
                       result_name=str(tmp_path / name), len_path=15,
                       num_repetition=3, epochs=25, device=device, seed=0,
                       **kw)


def _columns(path) -> dict:
    rows = [ln.split("\t") for ln in path.read_text().splitlines()]
    assert len({len(r) for r in rows}) == 1
    return {name: [r[j] for r in rows[1:]] for j, name in enumerate(rows[0])}


def check_matrix(files: dict, tmp_path, device: str, base: dict):
    ranksum = base.get("score_stat") == "ranksum"
    everything = dict(base)
    for kw in FEATURES.values():
        everything.update(kw)
    log_all = tmp_path / "all.jsonl"
    pipeline.run(_cfg(files, tmp_path, device, "none", **base))
    pipeline.run(_cfg(files, tmp_path, device, "all", log_jsonl=str(log_all),
                      **everything))
    for name, kw in FEATURES.items():
        pipeline.run(_cfg(files, tmp_path, device, name, **base, **kw))

    for name in ("none", *FEATURES):
        for suffix in TRIPLE:
            assert (tmp_path / (name + suffix)).read_bytes() == \
                (tmp_path / ("all" + suffix)).read_bytes(), (name, suffix)

    all_cols = _columns(tmp_path / "all_scores.txt")
    assert list(all_cols) == (
        ["GeneSymbol", "Lgroup", "d_score"]
        + (["z_ranksum", "auc"] if ranksum else ["t_score"])
        + ["gene_score", "biomarker", "silhouette", "nearest_lgroup",
           "p_perm", "q_bh", "p_maxT"])
    assert not (tmp_path / "none_scores.txt").exists()
    with_table = ("write_scores", "permutations", "silhouette")
    for name in FEATURES:
        table = tmp_path / (name + "_scores.txt")
        assert table.exists() == (name in with_table), name
        if name in with_table:
            for col, cells in _columns(table).items():
                assert cells == all_cols[col], (name, col)
    assert {"p_perm", "q_bh", "p_maxT"} <= set(
        _columns(tmp_path / "permutations_scores.txt"))
    assert {"silhouette", "nearest_lgroup"} <= set(
        _columns(tmp_path / "silhouette_scores.txt"))

    wrote = {"neighbors": EXTRA_FILES[:1], "replicates": EXTRA_FILES[1:]}
    for name in ("none", *FEATURES):
        for suffix in EXTRA_FILES:
            path = tmp_path / (name + suffix)
            assert path.exists() == (suffix in wrote.get(name, ())), path
            if path.exists():
                assert path.read_bytes() == \
                    (tmp_path / ("all" + suffix)).read_bytes(), (name, suffix)

    events = [json.loads(ln)["event"] for ln in log_all.open()]
    assert [e for e in events if e != "phase"] == (
        ["counts", "paths", "train"]
        + (["kmeans", "score_stat"] if ranksum else [])
        + ["silhouette", "replicates", "perm", "neighbors", "done"])


def check_failed_run_closes_the_sink(files: dict, tmp_path, monkeypatch):
    """A writer that raises: the error reaches the caller, and the JSONL
    file is closed and ends in a complete record."""
    opened = []

    class Recording(pipeline.JsonlLogger):
        def __init__(self, path=""):
            super().__init__(path)
            opened.append(self._f)

    def full_disk(*a, **k):
        raise OSError("no space left on device")

    monkeypatch.setattr(pipeline, "JsonlLogger", Recording)
    monkeypatch.setattr(pipeline.gio, "write_vectors", full_disk)
    log = tmp_path / "failed.jsonl"
    with pytest.raises(OSError, match="no space left"):
        pipeline.run(_cfg(files, tmp_path, "cpu", "failed",
                          log_jsonl=str(log)))
    assert len(opened) == 1 and opened[0].closed
    text = log.read_text()
    assert text.endswith("\n")
    records = [json.loads(ln) for ln in text.splitlines()]
    assert records[-1] == dict(records[-1], event="phase", name="write")
    assert not any(r["event"] == "done" for r in records)
