"""The attention edge cases of tests/attn_edge_cases.py on the C oracle, held to the fp64 reference of tests/attn_ref64.py
with the bound the kernels get (no GPU; the same cases run on libpascohip.so in tests/test_hip_attn_edges.py).  This leg
proves the case table and the reference sound where no GPU is at hand; cases marked gpu_only (at most one in five, and
never the only one of a class) are left to the GPU leg."""
import pytest
import torch

from tests.attn_edge_cases import CASES


@pytest.mark.parametrize("case", [c for c in CASES if not c.gpu_only], ids=lambda c: c.__name__)
def test_attn_edges_oracle(oracle, case):
    case(oracle, torch.device("cpu"))
