"""The sparse-structure edge cases of tests/coords_edge_cases.py on the C oracle, held to the independent restatement of
tests/coords_ref.py (no GPU; the same cases run on libpascohip.so in tests/test_hip_coords_edges.py)."""
import pytest
import torch

from tests.coords_edge_cases import CASES


@pytest.mark.parametrize("case", CASES)
def test_coords_edges_oracle(oracle, case):
    case(oracle, torch.device("cpu"))
