"""pipeline.run on the CPU with every opt-in feature at once against each
alone, under the default and the device backends of steps 5-6 (cases:
pipeline_matrix_cases.py), and the JSONL sink of a run that raises."""
import pytest

import pipeline_matrix_cases as mc


@pytest.mark.parametrize("base", [mc.HOST, mc.DEV], ids=["host", "dev"])
def test_all_features_equal_each_alone(tiny_files, tmp_path, base):
    mc.check_matrix(tiny_files, tmp_path, "cpu", base)


def test_failed_run_closes_the_jsonl_sink(tiny_files, tmp_path, monkeypatch):
    mc.check_failed_run_closes_the_sink(tiny_files, tmp_path, monkeypatch)
