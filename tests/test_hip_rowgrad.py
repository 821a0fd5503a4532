"""The pr_* kernels (include/pasco_rowgrad.h) and the autograd of `SparseTensor.dense()`, `ME.to_sparse()`, the duplicate-dropping
constructor and `MinkowskiMaxPooling` on the MI355X.  The dense <-> rows kernels are copies and are compared bit for bit with torch
index operations; the cases, the shared checks and the references are tests/rowgrad_cases.py and tests/rowgrad_ref.py.  The CPU
side is tests/test_rowgrad_cpu.py."""
import pytest
import torch

from tests import rowgrad_cases as rc
from tests.rowgrad_ref import ROW_STACK_M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.rowlib import rowgrad_lib
    return rowgrad_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("grid", rc.GRIDS, ids=["12x12x6", "5x7x3"])
def test_dense_rows(grid, C, lib, dev):
    rc.check_dense_rows(lib, dev, grid, C)


@pytest.mark.parametrize("C", [1, 65])
@pytest.mark.parametrize("grid", rc.GRIDS, ids=["12x12x6", "5x7x3"])
def test_dense_rows_wraps_and_skips(grid, C, lib, dev):
    rc.check_dense_rows_edges(lib, dev, grid, C)


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("grid", rc.GRIDS, ids=["12x12x6", "5x7x3"])
def test_rows_dense(grid, C, lib, dev):
    rc.check_rows_dense(lib, dev, grid, C)


def test_rows_dense_overwrites_and_no_rows_writes_zeros(lib, dev):
    out = torch.full((2, 3, 5, 7, 3), 7.0, device=dev)
    lib.rows_dense(torch.empty((0, 3), device=dev), torch.empty((0, 4), dtype=torch.int32, device=dev), out.shape, out=out)
    assert bool((out == 0).all())
    out.fill_(7.0)
    sc = rc.site_rows((5, 7, 3), 65, 1, True).to(dev)
    rows = rc.values((65, 3), 2, dev) + 5.0
    lib.rows_dense(rows, sc, out.shape, out=out)
    assert int((out != 0).sum()) == 65 * 3 and not bool((out == 7.0).any())


@pytest.mark.parametrize("C", rc.POOL_CHANNELS)
@pytest.mark.parametrize("kind", ["down", "same"])
def test_maxpool_arg_and_backward(kind, C, lib, dev, hip):
    rc.check_maxpool(lib, hip, dev, kind, C)


def test_dense_gradient_and_inference_route(lib, dev, hip):
    rc.check_dense_autograd(hip, dev)


def test_to_sparse_gradient_and_inference_route(lib, dev):
    rc.check_to_sparse_autograd(dev)


def test_dedup_gradient_and_inference_route(lib, dev, hip):
    rc.check_dedup_autograd(hip, dev)


@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 1)])
def test_maxpool_gradient_and_inference_route(ks, stride, lib, dev, hip):
    rc.check_maxpool_autograd(hip, dev, ks, stride)


def test_bottleneck_stack_gradients_against_the_fp64_twin(lib, dev):
    ratios = rc.row_stack_ratios(dev)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 11 and "dense3d.weight" in ratios and "dense3d.bias" in ratios and "x" in ratios
    for name, r in ratios.items():
        assert r <= ROW_STACK_M, f"{name}: max |g - g64| = {r:.2f} x max |g32 - g64|, bound {ROW_STACK_M}"
