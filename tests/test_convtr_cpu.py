"""The transposed convolution onto an existing map (`MinkowskiConvolutionTranspose` without `expand_coordinates`, and its
`coordinates=` argument) through the CPU checker backend, against the dense fp64 twin of tests/convtr_cases.py.  The same checks
run on the device in tests/test_hip_convtr.py."""
import pytest
import torch

from tests import convtr_cases as cc

CPU = torch.device("cpu")


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=[f"{a}to{b}" for a, b in cc.SHAPES])
def test_forward_against_the_dense_fp64_twin(shape, bias, oracle_registered):
    cc.check_forward(CPU, *shape, bias)


def test_the_target_is_the_encoders_map(oracle_registered):
    cc.check_map_identity(CPU)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=[f"{a}to{b}" for a, b in cc.SHAPES])
def test_gradients_against_the_dense_fp64_twin(shape, oracle_registered):
    cc.check_gradients(CPU, *shape)


def test_equal_to_the_generative_module_at_the_targets_rows(oracle_registered):
    cc.check_against_generative(CPU)


def test_coordinates_onto_a_pruned_map(oracle_registered):
    cc.check_coordinates_argument(CPU)


def test_grad_modes_and_a_pending_prologue(oracle_registered):
    cc.check_modes_and_prologue(CPU)


def test_refusals(oracle_registered):
    cc.check_refusals(CPU)
