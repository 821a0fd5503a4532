"""Training-mode batch normalisation over rows on the GPU: the pn_* kernels of libpascohip.so (include/pasco_norm.h) through
`pasco_amd.grad.norm.batch_norm_rows`, and the module route `set_me_norm("device")`.  The checks are tests/norm_cases.py (shared
with tests/test_norm_cpu.py), the references tests/norm_ref64.py: the fp64 torch twin, and torch's own fp32 batch_norm on the same
GPU as the yardstick of the error.  The cases of the short table are a few hundred rows; the long ones reach 65 tiles."""
import pytest
import torch
import torch.nn.functional as F

import pasco_amd.me as ME
from pasco_amd import settings
from pasco_amd.grad import host
from pasco_amd.me import modules as M
from tests import norm_cases as nc
from tests.norm_ref64 import NORM_M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def test_binding_mirrors_the_header(dev):
    import os
    import re
    from pasco_amd.grad import normlib
    lib = normlib.norm_lib()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pasco_norm.h")).read()
    const = lambda name: re.search(rf"#define {name} (.+?)\s*(/\*|$)", text, re.M).group(1).strip()
    assert int(const("PN_ABI_VERSION")) == normlib.PN_ABI_VERSION == lib.lib.pn_abi_version()
    assert int(const("PN_TILE_ROWS")) == normlib.PN_TILE_ROWS == host.NORM_TILE_ROWS
    T = normlib.PN_TILE_ROWS
    assert lib.ws_bytes(0, 7) == 0 and lib.ws_bytes(1, 7) == 3 * 7 * 8 and lib.ws_bytes(T + 1, 283) == 2 * 3 * 283 * 8
    with pytest.raises(RuntimeError):
        lib.ws_bytes(5, 0)
    with pytest.raises(RuntimeError, match="pn_apply: apply: act = 9"):
        lib.apply(torch.zeros(2, 3, device=dev), torch.zeros(2, 3, device=dev), None, None, 9, 0.0)


@pytest.mark.parametrize("n,c,act", nc.CASES, ids=[f"{n}x{c}_{a}" for n, c, a in nc.CASES])
def test_case_against_the_fp64_twin(dev, n, c, act):
    nc.check_case(dev, n, c, act)


def test_large_mean(dev):
    nc.check_large_mean(dev)


def test_misaligned_rows(dev):
    nc.check_misaligned(dev)


def test_repeat_gives_the_same_bits(dev):
    nc.check_repeat_bits(dev)


def test_merge_of_the_tile_records_is_the_whole(dev):
    nc.check_split_merge(dev)


def test_no_rows(dev):
    nc.check_empty(dev)


def test_total_count_of_one(dev):
    nc.check_count_one(dev)


def test_relu_at_zero_and_leaky_at_zero(dev):
    nc.check_relu_zero_gets_no_gradient(dev)


def test_leaky_slope_below_zero(dev):
    nc.check_leaky_slope(dev)


def test_without_affine_and_without_running_statistics(dev):
    nc.check_optional_tensors(dev)


def test_cumulative_average(dev):
    nc.check_cumulative_average(dev)


def test_counter_advances_in_place(dev):
    nc.check_counter_in_place(dev)


def test_one_row_raises(dev):
    nc.check_one_row_raises(dev)


def test_non_fp32_raises(dev):
    nc.check_non_fp32_synchronised(dev)


@pytest.mark.parametrize("act", nc.ACT_NAMES)
def test_virtual_ranks(dev, act):
    nc.check_virtual_ranks(dev, act)


@pytest.mark.parametrize("n,c,act", nc.LONG_CASES, ids=[f"{n}x{c}_{a}" for n, c, a in nc.LONG_CASES])
def test_long_case_against_the_fp64_twin(dev, n, c, act):
    """Tile records beyond the first wave and the first pass of the combine; the vector geometry at the net's widths."""
    nc.check_long_case(dev, n, c, act)


@pytest.mark.parametrize("c", nc.MERGE_C)
@pytest.mark.parametrize("r", nc.MERGE_R)
def test_merge_of_unequal_records_equals_the_restatement(dev, r, c):
    nc.check_merge_records(dev, r, c)


@pytest.mark.parametrize("n", nc.LONG_ROWS)
def test_merge_of_many_tile_records_is_the_whole(dev, n):
    nc.check_split_merge_long(dev, n)


def test_virtual_ranks_at_128_channels(dev):
    nc.note_long(dev, max(nc.check_virtual_ranks(dev, "relu", c=128).values()))


def test_misaligned_rows_at_256_channels(dev):
    nc.note_long(dev, max(nc.check_misaligned(dev, c=256).values()))


def test_restatement_has_the_kernels_records(dev):
    """The CPU restatement forms the same records in the same order: fp64 sums of the same fp32 values differ by the order
    inside a tile only."""
    x = nc.inputs(3 * nc.T + 5, 65, "cpu")[0]
    a, b = host.norm_moments(x), nc.ops_of(dev).moments(x.to(dev)).cpu()
    assert torch.equal(a[0], b[0]) and torch.allclose(a[1], b[1], rtol=1e-13, atol=1e-13) and torch.allclose(a[2], b[2], rtol=1e-12)


@pytest.fixture()
def device_norm():
    M.set_me_norm("device")
    yield
    M.set_me_norm("torch")


def test_default_module_forward_is_torchs_op(dev):
    assert settings.current().me_norm == "torch"
    x, _, w, b, rm, rv = nc.inputs(65, 20, dev)
    coords = torch.cat([torch.zeros(65, 1, dtype=torch.int32), torch.arange(65, dtype=torch.int32)[:, None].expand(65, 3)], 1)
    for cls in (ME.MinkowskiBatchNorm, ME.MinkowskiSyncBatchNorm):
        mod = cls(20).to(dev).train()
        with torch.no_grad():
            mod.bn.weight.copy_(w), mod.bn.bias.copy_(b), mod.bn.running_mean.copy_(rm), mod.bn.running_var.copy_(rv)
        out = mod(ME.SparseTensor(x.clone(), coords.contiguous().to(dev)))
        rm2, rv2 = rm.clone(), rv.clone()
        want = F.batch_norm(x, rm2, rv2, w, b, True, 0.1, 1e-5)
        assert torch.equal(out.F, want) and torch.equal(mod.bn.running_mean, rm2) and torch.equal(mod.bn.running_var, rv2)
        assert "BatchNormRows" not in type(out.F.grad_fn).__name__


def test_device_module_route(dev, device_norm):
    """Under set_me_norm("device") a training-mode MinkowskiBatchNorm runs the kernels (and says so in its grad_fn), moves the
    running statistics and the counter like torch's module; eval mode is untouched."""
    x, dy, w, b, rm, rv = nc.inputs(nc.T + 1, 20, dev)
    n = x.shape[0]
    coords = torch.cat([torch.zeros(n, 1, dtype=torch.int32), torch.arange(n, dtype=torch.int32)[:, None].expand(n, 3)], 1).to(dev)
    mod, twin = ME.MinkowskiBatchNorm(20).to(dev).train(), torch.nn.BatchNorm1d(20).to(dev).train()
    with torch.no_grad():
        for m in (mod.bn, twin):
            m.weight.copy_(w), m.bias.copy_(b), m.running_mean.copy_(rm), m.running_var.copy_(rv)
    counter = mod.bn.num_batches_tracked
    out = mod(ME.SparseTensor(x.clone(), coords.contiguous()))
    assert "BatchNormRows" in type(out.F.grad_fn).__name__
    want = twin(x)
    assert mod.bn.num_batches_tracked is counter and int(counter) == 1
    assert torch.allclose(out.F, want, rtol=1e-5, atol=1e-5)
    assert torch.allclose(mod.bn.running_mean, twin.running_mean, rtol=1e-6, atol=1e-6)
    assert torch.allclose(mod.bn.running_var, twin.running_var, rtol=1e-6, atol=1e-6)
    mod.eval()
    with torch.no_grad():
        ev = mod(ME.SparseTensor(x.clone(), coords.contiguous()))
    assert torch.allclose(ev.F, twin.eval()(x), rtol=1e-5, atol=1e-5)


def test_stack_gradients_on_the_device_route(dev, device_norm):
    """tests/grad_cases.py `Stack` (conv -> BatchNorm -> ReLU -> ...) with its BatchNorm on the kernels: every gradient within
    NORM_M of the fp64 twin, relative to the fp32 twin's own error."""
    from tests.grad_cases import stack_ratios
    r = stack_ratios(dev)
    print("[norm] Stack under set_me_norm('device'): " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"  (worst {max(r.values()):.3f})")
    bad = {k: v for k, v in r.items() if not v <= NORM_M}
    assert not bad, f"ratio over NORM_M = {NORM_M}: {bad}"
