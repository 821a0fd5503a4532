"""The attention backward on CPU tensors (tests/attn_grad_cases.py): the C oracle serves the forward launch, pasco_amd/grad/host.py
the backward, held to the fp64 gradients of tests/attn_grad_ref64.py by  max |g - g64| <= ATTN_GRAD_HOST_M x max |g32 - g64|
(g32 = torch fp32 autograd of the materialised formulation).  Then autograd, the drop-in layer and the binding.  The GPU side is
tests/test_hip_attn_grad.py."""
import importlib

import pytest
import torch

from pasco_amd.grad import host
from tests import attn_grad_cases as ac
from tests import test_bindings_cpu as tb
from tests.attn_grad_ref64 import ATTN_GRAD_HOST_M

CPU = torch.device("cpu")


@pytest.fixture()
def runner(oracle):
    return ac.Runner(CPU, oracle.attn_cross_fwd, host.attn_cross_bwd, ATTN_GRAD_HOST_M, "host")


@pytest.mark.parametrize("pattern", ac.PATTERNS)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "B%d_H%d_Q%d_N%d" % s)
def test_host_gradients_against_fp64(runner, shape, pattern):
    ac.check_precision(runner, shape, pattern)


def test_reference_dead_query_equals_its_removal():
    ac.check_dead_query_equals_its_removal()


def test_host_unattended_keys_get_exact_zero_rows(runner):
    ac.check_unattended_keys(runner)


def test_host_garbage_bits_beyond_q_change_nothing(runner):
    ac.check_garbage_bits(runner)


def test_host_ranges_that_start_fully_masked(runner):
    ac.check_masked_range_start(runner)


def test_host_unwanted_outputs_are_none_and_leave_the_others(runner):
    x = ac.inputs((1, 2, 40, 50), "mask_any")
    full = runner.grads(x)
    for i in range(3):
        need = tuple(j != i for j in range(3))
        part = runner.grads(x, need=need)
        assert part[i] is None
        for j in range(3):
            assert j == i or torch.equal(part[j], full[j])


def test_masked_cross_attention_gradient_and_inference_route(oracle_registered):
    ac.check_autograd_route(oracle_registered, CPU, ATTN_GRAD_HOST_M)


def test_cross_attention_layer_against_the_multihead_attention_twin(oracle_registered):
    ac.check_layer(CPU, ATTN_GRAD_HOST_M, "host")


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _pa_family(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pa", ("pasco_attngrad.h", "pasco_amd.grad.attnlib", "PA_ABI_VERSION", "AttnGradLib",
                                            "attn_grad_lib"))
    return importlib.import_module("pasco_amd.grad.attnlib")


def test_pa_binding_table_matches_its_header(monkeypatch):
    mod = _pa_family(monkeypatch)
    protos, version = tb.prototypes("pa")
    assert len(protos) == 5
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pa_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert tb.ctypes_coarse(t) == a, f"pa_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, tb.C.c_int)) == ret, f"pa_{name}: return type, the header says {ret}"
    assert mod.PA_ABI_VERSION == version == 1


def test_pa_binding_rejects_other_abi_versions_and_refuses_on_the_host(monkeypatch):
    from pasco_amd.build import build_hip
    mod = _pa_family(monkeypatch)
    path = build_hip(verbose=False)
    lib = mod.AttnGradLib(path)                              # the version it was written against binds
    # refusals on scalar arguments, before anything touches the HIP runtime: nothing is launched, no pointer is read
    none10 = (None,) * 10
    assert lib.lib.pa_attn_cross_bwd(*none10, 10, 1, 1, 10, 64, None, 0, None) == 1
    assert b"head dim 64 not served" in lib.lib.pa_last_error()
    assert lib.lib.pa_abi_version() == 1 and b"head dim 64 not served" in lib.lib.pa_last_error()      # the text stays
    assert lib.lib.pa_attn_cross_bwd(*none10, 10, 1, 1, 129, 48, None, 0, None) == 1 and b"129 queries" in lib.lib.pa_last_error()
    assert lib.lib.pa_attn_cross_bwd(*none10, 0, 1, 1, 10, 48, None, 0, None) == 1 and b"shape" in lib.lib.pa_last_error()
    assert lib.lib.pa_attn_cross_bwd(*none10, 10, 1, 1, 10, 48, None, 1 << 40, None) == 1 and b"workspace" in lib.lib.pa_last_error()
    assert lib.workspace_bytes(10, 1, 1, 10, 64) == 0 and lib.workspace_bytes(10, 1, 1, 10) > 0
    # the workspace is what the launch arithmetic of attn_grad_cases.bwd_geometry says: statistics, partial (m, l), partial dQ
    for shape in ac.SHAPES:
        B, H, Q, N = shape
        ge, rows = ac.bwd_geometry(*shape), (Q + 15) // 16 * 16
        a256 = lambda v: (v + 255) // 256 * 256
        want = 2 * a256(B * H * rows * 4) + a256(B * H * ge["splits"] * rows * 8) + a256(B * H * ge["splits"] * rows * 48 * 4)
        assert lib.workspace_bytes(N, B, H, Q) == want, shape
    monkeypatch.setattr(mod, "PA_ABI_VERSION", mod.PA_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.AttnGradLib(path)
