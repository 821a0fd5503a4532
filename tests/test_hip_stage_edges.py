"""The input-stage, ensembling and panoptic edge cases of tests/stage_edge_cases.py on libpascohip.so (csrc/input.hip,
csrc/rows.hip, csrc/panop.hip), held to the independent references of tests/stage_ref.py (the same cases run on the C oracle
in tests/test_stage_edges_cpu.py), and one leg at the row count of the benchmark scene's finest level."""
import pytest
import torch

from tests.stage_edge_cases import CASES, full_size

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_stage_edges_hip(hip, case):
    case(hip, torch.device("cuda", 0))


def test_stage_edges_full_size_hip(hip):
    full_size(hip, torch.device("cuda", 0))
