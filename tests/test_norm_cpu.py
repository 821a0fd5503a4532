"""Training-mode batch normalisation over rows on CPU tensors: `pasco_amd.grad.norm.batch_norm_rows` on the torch restatement
of include/pasco_norm.h (pasco_amd/grad/host.py) - the same records and the same merge order as the kernels.  The checks are
tests/norm_cases.py, the references tests/norm_ref64.py; the GPU side is tests/test_hip_norm.py."""
import pytest
import torch
import torch.nn.functional as F

import pasco_amd.me as ME
from pasco_amd import settings
from tests import norm_cases as nc

CPU = torch.device("cpu")


@pytest.mark.parametrize("n,c,act", nc.CASES, ids=[f"{n}x{c}_{a}" for n, c, a in nc.CASES])
def test_case_against_the_fp64_twin(n, c, act):
    nc.check_case(CPU, n, c, act)


def test_large_mean():
    nc.check_large_mean(CPU)


def test_repeat_gives_the_same_bits():
    nc.check_repeat_bits(CPU)


def test_merge_of_the_tile_records_is_the_whole():
    nc.check_split_merge(CPU)


def test_no_rows():
    nc.check_empty(CPU)


def test_total_count_of_one():
    nc.check_count_one(CPU)


def test_relu_at_zero_and_leaky_at_zero():
    nc.check_relu_zero_gets_no_gradient(CPU)


def test_leaky_slope_below_zero():
    nc.check_leaky_slope(CPU)


def test_without_affine_and_without_running_statistics():
    nc.check_optional_tensors(CPU)


def test_cumulative_average():
    nc.check_cumulative_average(CPU)


def test_counter_advances_in_place():
    nc.check_counter_in_place(CPU)


def test_one_row_raises():
    nc.check_one_row_raises(CPU)


def test_non_fp32_synchronised_raises():
    nc.check_non_fp32_synchronised(CPU)


@pytest.mark.parametrize("act", nc.ACT_NAMES)
def test_virtual_ranks(act):
    nc.check_virtual_ranks(CPU, act)


@pytest.mark.parametrize("n,c,act", nc.LONG_CASES, ids=[f"{n}x{c}_{a}" for n, c, a in nc.LONG_CASES])
def test_long_case_against_the_fp64_twin(n, c, act):
    """Tile records beyond the first wave and the first pass of the combine; the vector geometry at the net's widths."""
    nc.check_long_case(CPU, n, c, act)


@pytest.mark.parametrize("c", nc.MERGE_C)
@pytest.mark.parametrize("r", nc.MERGE_R)
def test_merge_of_unequal_records_equals_the_restatement(r, c):
    nc.check_merge_records(CPU, r, c)


@pytest.mark.parametrize("n", nc.LONG_ROWS)
def test_merge_of_many_tile_records_is_the_whole(n):
    nc.check_split_merge_long(CPU, n)


def test_virtual_ranks_at_128_channels():
    nc.note_long(CPU, max(nc.check_virtual_ranks(CPU, "relu", c=128).values()))


def test_default_module_forward_is_torchs_op(oracle_registered):
    """The default route is unchanged: a training-mode `MinkowskiBatchNorm` (and a `MinkowskiSyncBatchNorm` outside a process
    group) returns the bits of torch's batch_norm and moves the running statistics as it does."""
    assert settings.current().me_norm == "torch"
    x, _, w, b, rm, rv = nc.inputs(65, 20, CPU)
    coords = torch.cat([torch.zeros(65, 1, dtype=torch.int32), torch.arange(65, dtype=torch.int32)[:, None].expand(65, 3)], 1)
    for cls in (ME.MinkowskiBatchNorm, ME.MinkowskiSyncBatchNorm):
        mod = cls(20).train()
        with torch.no_grad():
            mod.bn.weight.copy_(w), mod.bn.bias.copy_(b), mod.bn.running_mean.copy_(rm), mod.bn.running_var.copy_(rv)
        out = mod(ME.SparseTensor(x.clone(), coords.contiguous()))
        rm2, rv2 = rm.clone(), rv.clone()
        want = F.batch_norm(x, rm2, rv2, w, b, True, 0.1, 1e-5)
        assert torch.equal(out.F, want) and torch.equal(mod.bn.running_mean, rm2) and torch.equal(mod.bn.running_var, rv2)
        assert "BatchNormRows" not in type(out.F.grad_fn).__name__


def test_convert_keeps_the_process_group():
    net = torch.nn.Sequential(ME.MinkowskiBatchNorm(4), torch.nn.Sequential(ME.MinkowskiBatchNorm(8, momentum=None)))
    marker = object()
    out = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(net, marker)
    syncs = [m for m in out.modules() if isinstance(m, ME.MinkowskiSyncBatchNorm)]
    assert len(syncs) == 2 and all(m.process_group is marker for m in syncs)
    assert syncs[1].bn.momentum is None and list(out.state_dict()) == list(net.state_dict())
