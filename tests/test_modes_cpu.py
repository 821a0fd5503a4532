"""The train / eval boundary of `pasco_amd.me` on CPU tensors (the CPU oracle serves the forward launches, pasco_amd/grad/host.py
the backward ones): stale caches and lost gradients where a caller crosses from one mode to the other.  The cases and references
are tests/mode_cases.py; the GPU side is tests/test_hip_modes.py."""
import pytest
import torch

from tests import mode_cases as mc

CPU = torch.device("cpu")


@pytest.fixture()
def split_oracle(oracle_registered):
    """The checker backend taking split-operand descriptors: the modules then run the guarded route as on the device."""
    oracle_registered.checker_split = True
    yield oracle_registered
    oracle_registered.checker_split = False


def _passes(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad)


@pytest.mark.parametrize("inp", mc.INPUTS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_mode_matrix(kind, inp, split_oracle):
    _passes(mc.mode_matrix(kind, inp, CPU, split_oracle))


@pytest.mark.parametrize("kind", mc.KINDS)
def test_mode_matrix_on_the_exact_route(kind, oracle_registered):
    _passes(mc.mode_matrix(kind, "relu", CPU, oracle_registered))


@pytest.mark.parametrize("body_autograd", [False, True], ids=["body_no_grad", "body_frozen_autograd"])
def test_frozen_body_trainable_head(body_autograd, split_oracle):
    _passes(mc.frozen_body(CPU, split_oracle, body_autograd))


@pytest.mark.parametrize("momentum, affine_trains", [(0.1, True), (None, True), (0.1, False)],
                         ids=["momentum_0.1", "momentum_None", "frozen_affine"])
def test_train_validate_cycles(momentum, affine_trains, split_oracle):
    _passes(mc.train_validate_cycles(CPU, momentum, affine_trains))


def test_fused_fold_after_a_training_forward(split_oracle):
    _passes(mc.fused_fold_after_training_forward(CPU))


def test_decoder_resize_entry_is_rebuilt(split_oracle, monkeypatch):
    _passes(mc.decoder_resize_after_training_forward(CPU, monkeypatch))


def test_guarded_forward_under_autograd(split_oracle):
    _passes(mc.guarded_under_autograd(CPU, split_oracle))
