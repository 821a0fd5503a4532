"""Gradients through `SparseTensor.dense()`, `ME.to_sparse()`, the duplicate-dropping constructor and `MinkowskiMaxPooling`
(pasco_amd/me/autograd.py) on CPU tensors: the CPU oracle serves the forward launches, pasco_amd/grad/host.py the backward ones.
The cases, the shared checks and the torch references are tests/rowgrad_cases.py and tests/rowgrad_ref.py; the GPU side is
tests/test_hip_rowgrad.py."""
import importlib

import pytest
import torch

from pasco_amd.grad import host
from tests import rowgrad_cases as rc
from tests import test_bindings_cpu as tb
from tests.rowgrad_ref import ROW_STACK_M

CPU = torch.device("cpu")


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("grid", rc.GRIDS, ids=["12x12x6", "5x7x3"])
def test_host_dense_rows(grid, C):
    rc.check_dense_rows(host, CPU, grid, C)


@pytest.mark.parametrize("grid", rc.GRIDS, ids=["12x12x6", "5x7x3"])
def test_host_dense_rows_wraps_and_skips(grid):
    rc.check_dense_rows_edges(host, CPU, grid, 65)


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("grid", rc.GRIDS, ids=["12x12x6", "5x7x3"])
def test_host_rows_dense(grid, C):
    rc.check_rows_dense(host, CPU, grid, C)


@pytest.mark.parametrize("C", rc.POOL_CHANNELS)
@pytest.mark.parametrize("kind", ["down", "same"])
def test_host_maxpool(kind, C, oracle_registered):
    rc.check_maxpool(host, oracle_registered, CPU, kind, C)


def test_dense_gradient_and_inference_route(oracle_registered):
    rc.check_dense_autograd(oracle_registered, CPU)


def test_to_sparse_gradient_and_inference_route(oracle_registered):
    rc.check_to_sparse_autograd(CPU)


def test_dedup_gradient_and_inference_route(oracle_registered):
    rc.check_dedup_autograd(oracle_registered, CPU)


@pytest.mark.parametrize("ks,stride", [(2, 2), (3, 1)])
def test_maxpool_gradient_and_inference_route(ks, stride, oracle_registered):
    rc.check_maxpool_autograd(oracle_registered, CPU, ks, stride)


def test_bottleneck_stack_gradients_against_the_fp64_twin(oracle_registered):
    ratios = rc.row_stack_ratios(CPU)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 11 and "dense3d.weight" in ratios and "dense3d.bias" in ratios and "x" in ratios
    for name, r in ratios.items():
        assert r <= ROW_STACK_M, f"{name}: max |g - g64| = {r:.2f} x max |g32 - g64|, bound {ROW_STACK_M}"


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _pr_family(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pr", ("pasco_rowgrad.h", "pasco_amd.grad.rowlib", "PR_ABI_VERSION", "RowGradLib",
                                            "rowgrad_lib"))
    return importlib.import_module("pasco_amd.grad.rowlib")


def test_pr_binding_table_matches_its_header(monkeypatch):
    mod = _pr_family(monkeypatch)
    protos, version = tb.prototypes("pr")
    assert len(protos) == 6
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pr_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert tb.ctypes_coarse(t) == a, f"pr_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, tb.C.c_int)) == ret, f"pr_{name}: return type, the header says {ret}"
    assert mod.PR_ABI_VERSION == version == 1


def test_pr_binding_rejects_other_abi_versions_and_keeps_its_error_text(monkeypatch):
    from pasco_amd.build import build_hip
    mod = _pr_family(monkeypatch)
    path = build_hip(verbose=False)
    lib = mod.RowGradLib(path)                               # the version it was written against binds
    # refusals on scalar arguments, before anything touches the HIP runtime: nothing is launched, no pointer is read
    assert lib.lib.pr_maxpool_bwd(None, 1, 1, None, None, 65, 1, None, None) == 1
    assert b"maxpool_bwd: K = 65" in lib.lib.pr_last_error()
    assert lib.lib.pr_abi_version() == 1 and b"maxpool_bwd: K = 65" in lib.lib.pr_last_error()      # the text stays
    assert lib.lib.pr_dense_rows(None, 4, 1, 2, 2, 2, None, 0, 0, 0, 0, 1, None, None) == 0         # n == 0: a no-op
    assert b"maxpool_bwd: K = 65" in lib.lib.pr_last_error()
    assert lib.lib.pr_dense_rows(None, 4, 1, 2, 2, 2, None, 1, 0, 0, 0, 0, None, None) == 1
    assert b"dense_rows: ts = 0" in lib.lib.pr_last_error()
    assert lib.lib.pr_rows_dense(None, -1, 4, None, 1, 2, 2, 2, None, None) == 1 and b"rows_dense: n = -1" in lib.lib.pr_last_error()
    assert lib.lib.pr_maxpool_arg(None, 1, 0, None, 8, 1, None, None, None) == 1 and b"maxpool_arg: c = 0" in lib.lib.pr_last_error()
    with pytest.raises(RuntimeError, match="pr_maxpool_arg: maxpool_arg: c = 0"):
        lib._ok(1, "maxpool_arg")
    monkeypatch.setattr(mod, "PR_ABI_VERSION", mod.PR_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.RowGradLib(path)
