"""The autograd layer of the convolution family (pasco_amd/me/autograd.py) on CPU tensors: the CPU oracle serves the forward
launches, pasco_amd/grad/host.py the backward ones.  References are fp64 torch twins written from the formulas
(tests/grad_ref64.py); the GPU side is tests/test_hip_grad.py."""
import importlib

import pytest
import torch

import pasco_amd.me as ME
from pasco_amd.grad import host
from tests import test_bindings_cpu as tb
from tests.conv_ref64 import gather_sum64, violations
from tests.grad_cases import (KINDS, SLAB_ROWS, WGRAD_CAPPED, WGRAD_CASES, box_coords, make_map, make_module, operands, stack_ratios,
                              table_out_of_range, wgrad_geometry)
from tests.grad_ref64 import C_WGRAD, STACK_M, conv_twin, invert_loop, invert_torch, sum_cap, wgrad64

CPU = torch.device("cpu")


def _run(kind, cin=16, cout=24, seed=0):
    m = make_map(kind, CPU, seed)
    torch.manual_seed(seed)
    mod = make_module(kind, cin, cout).train()
    feats, dy = operands(m["n_in"], cin, m["n_out"], cout, CPU)
    feats.requires_grad_(True)
    x = ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])
    return m, mod, feats, dy, mod(x)


@pytest.mark.parametrize("kind", KINDS)
def test_conv_output_has_grad_fn_and_todays_values(kind, oracle_registered):
    m, mod, feats, _, out = _run(kind)
    assert out.F.grad_fn is not None
    assert out.F.shape == (m["n_out"], 24)
    want = oracle_registered.conv_fwd(feats.detach(), mod.kernel.detach(), m["nbr"], m["n_out"],
                                      bias=mod.bias.detach().reshape(-1).contiguous())
    assert torch.equal(out.F.detach(), want)
    out.F.square().sum().backward()
    assert mod.kernel.grad is not None and mod.kernel.grad.shape == mod.kernel.shape
    assert mod.bias.grad is not None and mod.bias.grad.shape == mod.bias.shape
    assert feats.grad is not None and feats.grad.shape == feats.shape


@pytest.mark.parametrize("kind", KINDS)
def test_conv_gradients_against_the_fp64_twin(kind, oracle_registered):
    m, mod, feats, dy, out = _run(kind)
    out.F.backward(dy)
    x64 = feats.detach().double().requires_grad_(True)
    w64 = mod.kernel.detach().double().requires_grad_(True)
    b64 = mod.bias.detach().double().requires_grad_(True)
    conv_twin(x64, w64, m["nbr"], b64).backward(dy.double())
    # weight gradient: element-wise against its magnitude
    ref, A = wgrad64(feats.detach(), dy, m["nbr"])
    assert torch.allclose(ref, w64.grad, rtol=1e-12, atol=1e-12)           # the two references agree
    err = (mod.kernel.grad.double() - w64.grad).abs()
    assert bool((err <= C_WGRAD * A + 1e-30).all()), float((err / (A + 1e-300)).max())
    # bias gradient
    err = (mod.bias.grad.double() - b64.grad).abs()
    assert bool((err <= sum_cap(m["n_out"]) * dy.double().abs().sum(0) + 1e-30).all())
    # input gradient: the forward operation over the inverse table
    inv = invert_torch(m["nbr"], m["n_in"])
    w_t = mod.kernel.detach().transpose(1, 2).contiguous()
    acc, mag = gather_sum64(dy, w_t, inv, torch.arange(m["n_in"]))
    assert torch.allclose(acc, x64.grad, rtol=1e-12, atol=1e-12)
    assert not bool(violations(feats.grad, acc, mag, acc.abs()).any())


def test_k1_convolution_gradients(oracle_registered):
    m = make_map("same", CPU)
    torch.manual_seed(1)
    mod = ME.MinkowskiConvolution(16, 20, kernel_size=1, bias=True, dimension=3).train()
    feats, dy = operands(m["n_in"], 16, m["n_in"], 20, CPU)
    feats.requires_grad_(True)
    out = mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"]))
    assert out.F.grad_fn is not None
    out.F.backward(dy)
    x64, w64, b64 = (t.detach().double().requires_grad_(True) for t in (feats, mod.kernel, mod.bias))
    conv_twin(x64, w64, None, b64).backward(dy.double())
    for got, want in ((feats.grad, x64.grad), (mod.kernel.grad, w64.grad), (mod.bias.grad, b64.grad)):
        assert got.shape == want.shape
        assert float((got.double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_only_what_requires_grad_gets_one(oracle_registered):
    m = make_map("same", CPU)
    mod = make_module("same", 8, 8).train()
    mod.kernel.requires_grad_(False)
    feats = torch.randn(m["n_in"], 8)
    out = mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"]))
    out.F.sum().backward()                      # only the bias asks
    assert mod.kernel.grad is None and feats.grad is None
    assert torch.allclose(mod.bias.grad, torch.full((1, 8), float(m["n_out"])))
    mod.bias.requires_grad_(False)
    out = mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"]))
    assert out.F.grad_fn is None                # nothing requires grad: the present route
    with torch.no_grad():
        mod.kernel.requires_grad_(True)
        assert mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])).F.grad_fn is None


def test_nbr_invert_against_the_loop(oracle_registered):
    for kind in KINDS:
        m = make_map(kind, CPU)
        want = invert_loop(m["nbr"], m["n_in"])
        assert torch.equal(host.nbr_invert(m["nbr"], m["n_in"]), want)
        assert torch.equal(invert_torch(m["nbr"], m["n_in"]), want)
        assert torch.equal(m["mgr"].kernel_map_inverse(m["nbr"], m["n_in"]), want)
        assert m["mgr"].kernel_map_inverse(m["nbr"], m["n_in"]) is m["mgr"].kernel_map_inverse(m["nbr"], m["n_in"])   # cached
    nbr = make_map("same", CPU)["nbr"].clone()
    nbr[5] = -1                                  # one offset entirely absent
    inv = host.nbr_invert(nbr, nbr.shape[1])
    assert torch.equal(inv, invert_loop(nbr, nbr.shape[1])) and bool((inv[5] == -1).all())
    empty = host.nbr_invert(torch.empty((27, 0), dtype=torch.int32), 7)
    assert empty.shape == (27, 7) and bool((empty == -1).all())
    assert host.nbr_invert(torch.empty((27, 0), dtype=torch.int32), 0).shape == (27, 0)


def test_host_wgrad_edges():
    nbr = torch.full((8, 5), -1, dtype=torch.int32)
    x, dy = torch.randn(4, 3), torch.randn(5, 2)
    assert torch.equal(host.conv_wgrad(x, dy, nbr), torch.zeros(8, 3, 2))
    assert torch.equal(host.conv_wgrad(x, torch.empty(0, 2), torch.empty((8, 0), dtype=torch.int32)), torch.zeros(8, 3, 2))
    nbr[3, 1], nbr[3, 4] = 2, 0
    want = torch.zeros(8, 3, 2)
    want[3] = torch.outer(x[2], dy[1]) + torch.outer(x[0], dy[4])
    assert torch.allclose(host.conv_wgrad(x, dy, nbr), want, atol=1e-6)
    assert torch.equal(host.colsum(torch.empty(0, 4)), torch.zeros(4))


def test_host_wgrad_entries_outside_the_input_are_absent(oracle_registered):
    m = make_map("same", CPU)
    bad = table_out_of_range(m["nbr"], m["n_in"])
    assert int((bad >= m["n_in"]).sum()) > 100 and int((bad == -7).sum()) > 100
    x, dy = operands(m["n_in"], 12, m["n_out"], 9, CPU)
    ref, A = wgrad64(x, dy, bad)
    absent = torch.where((bad >= 0) & (bad < m["n_in"]), bad, torch.full_like(bad, -1))
    assert torch.equal(wgrad64(x, dy, absent)[0], ref)
    got = host.conv_wgrad(x, dy, bad)
    assert bool(((got.double() - ref).abs() <= sum_cap(m["n_out"]) * A + 1e-30).all())


def test_wgrad_geometry_restates_the_library_queries():
    """tests/grad_cases.py `wgrad_geometry` chooses the shapes of the device tests: its slab arithmetic against the library's own
    host-side queries (nothing is launched), over the case tables."""
    from pasco_amd.grad.lib import GradLib
    from pasco_amd.build import build_hip
    lib = GradLib(build_hip(verbose=False))
    assert lib.wgrad_slab_rows(27, 32, 32, 1) == SLAB_ROWS
    natural = box_coords(0).shape[0]
    for name, kind, cin, cout, rows_of in WGRAD_CASES + [WGRAD_CAPPED[:4] + (lambda R: WGRAD_CAPPED[4],)]:
        K = 27 if kind == "same" else 8
        rows = natural if rows_of is None else rows_of(SLAB_ROWS)
        g = wgrad_geometry(K, cin, cout, rows)
        assert g["slab_rows"] == lib.wgrad_slab_rows(K, cin, cout, rows), name
        assert lib.wgrad_workspace_bytes(K, cin, cout, rows) == (0 if g["slabs"] == 1 else g["slabs"] * K * cin * cout * 4), name


def _pruning(feats, m, mask):
    x = ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])
    return ME.MinkowskiPruning()(x, mask)


def test_pruning_gradient_and_inference_route(oracle_registered):
    m = make_map("same", CPU)
    feats = torch.randn(m["n_in"], 5)
    mask = torch.arange(m["n_in"]) % 3 != 0
    today = oracle_registered.gather_rows(feats, m["mgr"].prune(m["in_key"], mask)[1])
    assert torch.equal(today, feats[mask])
    for f, ctx in ((feats, torch.enable_grad()), (feats.clone().requires_grad_(True), torch.no_grad())):
        with ctx:
            out = _pruning(f, m, mask)
        assert out.F.grad_fn is None and torch.equal(out.F, today)
    f = feats.clone().requires_grad_(True)
    out = _pruning(f, m, mask)
    assert out.F.grad_fn is not None and torch.equal(out.F.detach(), today)
    g = torch.randn(out.F.shape)
    out.F.backward(g)
    twin = feats.clone().requires_grad_(True)
    twin[mask].backward(g)
    assert torch.equal(f.grad, twin.grad)


def test_union_add_gradient_and_inference_route(oracle_registered):
    m = make_map("same", CPU)
    mgr, key = m["mgr"], m["in_key"]
    mask_a, mask_b = torch.arange(m["n_in"]) % 3 != 0, torch.arange(m["n_in"]) % 2 == 0
    ka, keep_a = mgr.prune(key, mask_a)
    kb, keep_b = mgr.prune(key, mask_b)
    fa, fb = torch.randn(keep_a.shape[0], 6), torch.randn(keep_b.shape[0], 6)

    def add(a, b):
        return ME.SparseTensor(a, coordinate_map_key=ka, coordinate_manager=mgr) + \
            ME.SparseTensor(b, coordinate_map_key=kb, coordinate_manager=mgr)

    today = add(fa, fb)
    assert today.F.grad_fn is None
    with torch.no_grad():
        quiet = add(fa.clone().requires_grad_(True), fb)
    assert quiet.F.grad_fn is None and torch.equal(quiet.F, today.F)
    # the union rows of b, from the coordinates
    lookup = {tuple(c): i for i, c in enumerate(today.C.tolist())}
    b2o = torch.tensor([lookup[tuple(c)] for c in mgr.get_coordinates(kb).tolist()])
    na, n_out = fa.shape[0], today.F.shape[0]
    assert n_out > na
    for ra, rb in ((True, True), (True, False), (False, True)):
        a, b = fa.clone().requires_grad_(ra), fb.clone().requires_grad_(rb)
        out = add(a, b)
        assert out.F.grad_fn is not None and torch.equal(out.F.detach(), today.F)
        g = torch.randn(n_out, 6)
        out.F.backward(g)
        ta, tb_ = fa.clone().requires_grad_(ra), fb.clone().requires_grad_(rb)
        torch.cat([ta, torch.zeros(n_out - na, 6)]).index_add(0, b2o, tb_).backward(g)
        assert (a.grad is None) == (not ra) and (b.grad is None) == (not rb)
        if ra:
            assert torch.equal(a.grad, ta.grad)
        if rb:
            assert torch.equal(b.grad, tb_.grad)


def test_stack_gradients_against_the_fp64_twin(oracle_registered):
    ratios = stack_ratios(CPU)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 11
    for name, r in ratios.items():
        assert r <= STACK_M, f"{name}: max |g - g64| = {r:.2f} x max |g32 - g64|, bound {STACK_M}"


def _pg_family(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pg", ("pasco_grad.h", "pasco_amd.grad.lib", "PG_ABI_VERSION", "GradLib", "grad_lib"))
    return importlib.import_module("pasco_amd.grad.lib")


def test_pg_binding_table_matches_its_header(monkeypatch):
    mod = _pg_family(monkeypatch)
    protos, version = tb.prototypes("pg")
    assert len(protos) == 8
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pg_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert tb.ctypes_coarse(t) == a, f"pg_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, tb.C.c_int)) == ret, f"pg_{name}: return type, the header says {ret}"
    assert mod.PG_ABI_VERSION == version == 1


def test_pg_binding_rejects_other_abi_versions(monkeypatch):
    from pasco_amd.build import build_hip
    mod = _pg_family(monkeypatch)
    path = build_hip(verbose=False)
    lib = mod.GradLib(path)                                  # the version it was written against binds
    # host-side queries and refusals: nothing is launched
    assert lib.wgrad_slab_rows(27, 32, 32, 100) == 256 and lib.wgrad_workspace_bytes(27, 32, 32, 256) == 0
    assert lib.wgrad_workspace_bytes(27, 32, 32, 257) == 2 * 27 * 32 * 32 * 4
    big = lib.wgrad_slab_rows(27, 256, 256, 600_000)
    assert big > 256 and -(-600_000 // big) * 27 * 256 * 256 * 4 <= 64 << 20 < -(-600_000 // (big // 2)) * 27 * 256 * 256 * 4
    assert lib.wgrad_slab_rows(65, 32, 32, 100) == -1 and lib.wgrad_slab_rows(27, 0, 32, 100) == -1
    assert lib.lib.pg_nbr_invert(None, 65, 1, 1, None, None) == 1 and b"K = 65" in lib.lib.pg_last_error()
    monkeypatch.setattr(mod, "PG_ABI_VERSION", mod.PG_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.GradLib(path)
