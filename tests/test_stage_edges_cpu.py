"""The input-stage, ensembling and panoptic edge cases of tests/stage_edge_cases.py on the C oracle, held to the independent
references of tests/stage_ref.py (no GPU; the same cases run on libpascohip.so in tests/test_hip_stage_edges.py)."""
import pytest
import torch

from tests import stage_ref as ref
from tests.stage_edge_cases import CASES, full_size


@pytest.mark.parametrize("case", CASES)
def test_stage_edges_oracle(oracle, case):
    case(oracle, torch.device("cpu"))


def test_stage_edges_full_size_oracle(oracle):
    full_size(oracle, torch.device("cpu"))


def test_torch_formulation_fits(oracle):
    """K is twice the worst error of the plain fp32 torch formulation over the table: print what it is here,
    in units of 2^-24 scale, and tie the constant to it - a table that grows and moves the figure has to move K with it."""
    if not ref.TORCH_WORST:                                             # run alone: fill the figures
        for case in CASES:
            case.values[0](oracle, torch.device("cpu"))
    for kernel, x in sorted(ref.TORCH_WORST.items()):
        print(f"STAGE_TORCH32 {kernel} {x:.3f}")
    assert ref.K / 2.1 <= max(ref.TORCH_WORST.values()) <= ref.K / 2, (ref.K, ref.TORCH_WORST)
