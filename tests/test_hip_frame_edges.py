"""The frame-preparation edge cases of tests/frame_edge_cases.py on libpascohip.so (csrc/frame.hip), held exactly to the
independent reference of tests/frame_ref.py (which tests/test_frame_edges_cpu.py ties to the host restatements and the
recorded items without a GPU), and one leg at a real frame's size."""
import pytest
import torch

from tests.frame_edge_cases import CASES, full_size

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.data.frame_lib import frame_lib
    return frame_lib()


@pytest.mark.parametrize("case", CASES)
def test_frame_edges_hip(lib, case):
    case(lib, torch.device("cuda", 0))


def test_frame_edges_full_size_hip(lib):
    full_size(lib, torch.device("cuda", 0))
