"""The pooling / broadcast / channel-wise operators (include/pasco_pool.h) on CPU tensors: the host restatement
(pasco_amd/grad/host.py pool_*) against the fp64 references, and the modules of pasco_amd.me over the CPU oracle's maps.  The
cases, the shared checks and the references are tests/pool_cases.py and tests/pool_ref64.py; the GPU side is
tests/test_hip_pool.py."""
import pytest
import torch

import pasco_amd.me as ME
from pasco_amd.grad import pool_ops
from tests import pool_cases as pc
from tests.pool_ref64 import POOL_STACK_M

CPU = torch.device("cpu")
OPS = pool_ops(torch.zeros(1))


@pytest.mark.parametrize("c", pc.SEG_CHANNELS)
@pytest.mark.parametrize("kind", pc.BATCH_KINDS)
def test_host_seg_reduce_channels_and_batches(kind, c):
    pc.check_seg(OPS, CPU, 2 * pc.R + 3, c, kind)


@pytest.mark.parametrize("n", pc.ROWS)
def test_host_seg_reduce_rows(n):
    for c, kind in ((33, "gap"), (256, "shuffled8")):
        pc.check_seg(OPS, CPU, n, c, kind)


def test_host_seg_reduce_slice_and_max_edges():
    pc.check_seg_slice(OPS, CPU)
    pc.check_seg_max_edges(OPS, CPU)


@pytest.mark.parametrize("c", pc.CHANNELS)
def test_host_broadcast(c):
    for n, kind in ((2 * pc.R + 3, "gap"), (pc.R, "shuffled8"), (1, "one"), (0, "max")):
        pc.check_broadcast(OPS, CPU, n, c, kind, cg=c + 1 if c % 2 else c)
    pc.check_broadcast_batch_outside(OPS, CPU)


@pytest.mark.parametrize("variant", pc.TABLE_VARIANTS)
@pytest.mark.parametrize("kind", ["down", "same"])
def test_host_pool_and_chconv(kind, variant, oracle_registered):
    for c in (3, 32):
        pc.check_pool(OPS, CPU, kind, c, variant)
        pc.check_chconv(OPS, CPU, kind, c, variant, bias=c == 3)


@pytest.mark.parametrize("rows", pc.ROWS)
def test_host_chconv_wgrad_rows(rows, oracle_registered):
    pc.check_chconv_wgrad_rows(OPS, CPU, rows, 33)


def test_modules_against_the_dense_torch_operators(oracle_registered):
    pc.check_dense_twins(CPU, torch.float64)


@pytest.mark.parametrize("name", pc.MODULE_NAMES)
def test_module_modes_and_gradients(name, oracle_registered):
    assert [t[0] for t in pc.module_cases(CPU)] == pc.MODULE_NAMES
    pc.check_module_modes(CPU, name)
    pc.check_module_gradients(CPU, name)


def test_pending_prologue_is_applied(oracle_registered):
    pc.check_prologue(CPU)


def test_state_dict_and_refusals(oracle_registered):
    pc.check_state_dict()
    pc.check_refusals(CPU)


def test_new_names_are_exported():
    for name in ("MinkowskiSumPooling", "MinkowskiGlobalSumPooling", "MinkowskiGlobalMaxPooling", "MinkowskiBroadcast",
                 "MinkowskiBroadcastAddition", "MinkowskiBroadcastConcatenation", "MinkowskiGlobalPooling", "MinkowskiGlobalAvgPooling",
                 "MinkowskiBroadcastMultiplication", "MinkowskiChannelwiseConvolution", "MinkowskiPoolingTranspose", "MinkowskiAvgPooling"):
        assert issubclass(getattr(ME, name), torch.nn.Module), name
    assert ME.MinkowskiGlobalPooling.MODE == pc.AVG                       # upstream's default


def test_pool_stack_gradients_against_the_fp64_twin(oracle_registered):
    ratios = pc.pool_stack_ratios(CPU)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 9 and "dw.kernel" in ratios and "x" in ratios
    for name, r in ratios.items():
        assert r <= POOL_STACK_M, f"{name}: max |g - g64| = {r:.2f} x max |g32 - g64|, bound {POOL_STACK_M}"
