"""The sparse-structure edge cases of tests/coords_edge_cases.py on libpascohip.so (csrc/coords.hip, csrc/rows.hip), held to
the independent restatement of tests/coords_ref.py bit for bit (the same cases run on the C oracle in
tests/test_coords_edges_cpu.py)."""
import pytest
import torch

from tests.coords_edge_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES)
def test_coords_edges_hip(hip, case):
    case(hip, torch.device("cuda", 0))
