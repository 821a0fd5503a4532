"""The transposed convolution onto an existing map on the MI355X: `MinkowskiConvolutionTranspose` without `expand_coordinates`
lands on the map its input's map was strided from (or on the one `coordinates=` names), through the routes the generative module
runs - the guarded split-precision launch in inference, the exact route for a training-mode kernel, `ConvFunction` backwards -
against the dense fp64 twin of tests/convtr_cases.py.  The CPU side is tests/test_convtr_cpu.py."""
import pytest
import torch

from tests import convtr_cases as cc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("shape", cc.SHAPES, ids=[f"{a}to{b}" for a, b in cc.SHAPES])
def test_forward_against_the_dense_fp64_twin(shape, bias, dev):
    cc.check_forward(dev, *shape, bias)


def test_the_target_is_the_encoders_map(dev):
    cc.check_map_identity(dev)


@pytest.mark.parametrize("shape", cc.SHAPES, ids=[f"{a}to{b}" for a, b in cc.SHAPES])
def test_gradients_against_the_dense_fp64_twin(shape, dev):
    cc.check_gradients(dev, *shape)


def test_equal_to_the_generative_module_at_the_targets_rows(dev):
    cc.check_against_generative(dev)


def test_coordinates_onto_a_pruned_map(dev):
    cc.check_coordinates_argument(dev)


def test_grad_modes_and_a_pending_prologue(dev):
    assert cc.check_modes_and_prologue(dev), "the eval-mode BatchNorm -> ReLU in front was not deferred: the prologue route did not run"


def test_refusals(dev):
    cc.check_refusals(dev)
