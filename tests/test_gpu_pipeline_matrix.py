"""pipeline.run on the GPU with every opt-in feature at once against each
alone, under the HIP k-means, device scoring and rank-sum backends: seven
runs in one process (cases: pipeline_matrix_cases.py; CPU twin:
test_pipeline_matrix_cpu.py)."""
import pytest

import pipeline_matrix_cases as mc

pytestmark = pytest.mark.gpu


def test_all_features_equal_each_alone(tiny_files, tmp_path):
    mc.check_matrix(tiny_files, tmp_path, "cuda", mc.DEV)
