"""The train / eval boundary of `pasco_amd.me` on the MI355X: the cases of tests/mode_cases.py on the device, where channel counts
that are multiples of 8 take the split-precision route and the backward launches are the pg_* kernels.  The CPU side is
tests/test_modes_cpu.py."""
import pytest
import torch

from tests import mode_cases as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


def _passes(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad)


@pytest.mark.parametrize("inp", mc.INPUTS)
@pytest.mark.parametrize("kind", mc.KINDS)
def test_mode_matrix(kind, inp, hip, dev):
    _passes(mc.mode_matrix(kind, inp, dev, hip))


@pytest.mark.parametrize("body_autograd", [False, True], ids=["body_no_grad", "body_frozen_autograd"])
def test_frozen_body_trainable_head(body_autograd, hip, dev):
    _passes(mc.frozen_body(dev, hip, body_autograd))


@pytest.mark.parametrize("momentum, affine_trains", [(0.1, True), (None, True), (0.1, False)],
                         ids=["momentum_0.1", "momentum_None", "frozen_affine"])
def test_train_validate_cycles(momentum, affine_trains, hip, dev):
    _passes(mc.train_validate_cycles(dev, momentum, affine_trains))


def test_running_statistics_version_counters(hip, dev):
    """Whether a training-mode batch norm on device tensors moves the version counters of the running statistics is the
    backend's business; num_batches_tracked, which the caches key on, must move."""
    bn = torch.nn.BatchNorm1d(8).to(dev).train()
    before = (bn.running_mean._version, bn.running_var._version, bn.num_batches_tracked._version)
    bn(torch.randn(64, 8, device=dev))
    after = (bn.running_mean._version, bn.running_var._version, bn.num_batches_tracked._version)
    print(f"version counters (running_mean, running_var, num_batches_tracked): {before} -> {after}")
    assert after[2] > before[2]


def test_fused_fold_after_a_training_forward(hip, dev):
    _passes(mc.fused_fold_after_training_forward(dev))


def test_decoder_resize_entry_is_rebuilt(hip, dev, monkeypatch):
    _passes(mc.decoder_resize_after_training_forward(dev, monkeypatch))


def test_guarded_forward_under_autograd(hip, dev):
    _passes(mc.guarded_under_autograd(dev, hip))


def test_guarded_forward_under_autograd_window_tables(hip, dev):
    _passes(mc.guarded_under_autograd(dev, hip, n=16384, extent=(48, 48, 16), variants=mc.GUARDED[:1]))
