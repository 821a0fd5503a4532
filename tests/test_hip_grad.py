"""The pg_* kernels (include/pasco_grad.h) and the autograd layer on the MI355X, against fp64 references written from the formulas
(tests/grad_ref64.py) on the maps of tests/grad_cases.py.  The CPU side is tests/test_grad_cpu.py."""
import pytest
import torch

import pasco_amd.me as ME
from tests.conv_ref64 import gather_sum64, violations, worst_ratio
from tests.grad_cases import (COLSUM_ROWS, DGRAD_CASES, KINDS, WGRAD_CAPPED, WGRAD_CASES, WGRAD_MISALIGNED, make_map, make_module,
                              misaligned, operands, stack_ratios, table_out_of_range, table_with_rows, wgrad_geometry)
from tests.grad_ref64 import C_WGRAD, STACK_M, invert_torch, sum_cap, wgrad64

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.lib import grad_lib
    return grad_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


# ---- pg_nbr_invert ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_nbr_invert(kind, lib, dev):
    m = make_map(kind, dev)
    assert torch.equal(lib.nbr_invert(m["nbr"], m["n_in"]), invert_torch(m["nbr"], m["n_in"]))
    assert torch.equal(m["mgr"].kernel_map_inverse(m["nbr"], m["n_in"]), invert_torch(m["nbr"], m["n_in"]))


def test_nbr_invert_edges(lib, dev):
    nbr = make_map("same", dev)["nbr"].clone()
    nbr[5] = -1                                   # one offset entirely absent
    inv = lib.nbr_invert(nbr, nbr.shape[1])
    assert torch.equal(inv, invert_torch(nbr, nbr.shape[1])) and bool((inv[5] == -1).all())
    empty = lib.nbr_invert(torch.empty((27, 0), dtype=torch.int32, device=dev), 7)
    assert empty.shape == (27, 7) and bool((empty == -1).all())
    assert lib.nbr_invert(torch.full((8, 4), -1, dtype=torch.int32, device=dev), 0).shape == (8, 0)      # n_in == 0: a no-op


# ---- pg_conv_wgrad ------------------------------------------------------------------------------------------------------
def _check_wgrad(lib, x, dy, nbr, what):
    got = lib.conv_wgrad(x, dy, nbr)
    ref, A = wgrad64(x, dy, nbr)
    err = (got.double() - ref).abs()
    ok = A > 0
    worst = float((err[ok] / A[ok]).max()) if bool(ok.any()) else 0.0
    print(f"wgrad {what}: n_out = {nbr.shape[1]}, worst err / A = {worst:.3e}")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= sum_cap(nbr.shape[1]) * A + 1e-30).all()), f"{what}: worst err / A = {worst:.3e} above the a-priori cap"
    assert bool((err <= C_WGRAD * A + 1e-30).all()), f"{what}: worst err / A = {worst:.3e}, C_WGRAD = {C_WGRAD:.3e}"
    return got


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_wgrad_against_fp64(case, lib, dev):
    name, kind, cin, cout, rows_of = case
    K = 27 if kind == "same" else 8
    R = lib.wgrad_slab_rows(K, cin, cout, 1)
    rows = None if rows_of is None else rows_of(R)
    nbr, n_in = table_with_rows(kind, rows, dev)
    assert rows is None or nbr.shape[1] == rows
    assert lib.wgrad_slab_rows(K, cin, cout, nbr.shape[1]) == R          # the slab length the kernel uses at this shape
    x, dy = operands(n_in, cin, nbr.shape[1], cout, dev)
    _check_wgrad(lib, x, dy, nbr, name)


def test_conv_wgrad_slab_length_doubled_by_the_workspace_cap(lib, dev):
    name, kind, cin, cout, rows = WGRAD_CAPPED
    R = lib.wgrad_slab_rows(27, cin, cout, 1)
    assert lib.wgrad_slab_rows(27, cin, cout, rows) == 2 * R == wgrad_geometry(27, cin, cout, rows)["slab_rows"]
    assert lib.wgrad_workspace_bytes(27, cin, cout, rows) == 5 * 27 * cin * cout * 4
    nbr, n_in = table_with_rows(kind, rows, dev)
    assert nbr.shape[1] == rows
    x, dy = operands(n_in, cin, rows, cout, dev)
    first = _check_wgrad(lib, x, dy, nbr, name)
    again = lib.conv_wgrad(x, dy, nbr, out=torch.full_like(first, 3.0))
    assert torch.equal(first, again)                # overwritten, and the same bits


@pytest.mark.parametrize("which", WGRAD_MISALIGNED)
def test_conv_wgrad_base_pointer_not_16_byte_aligned(which, lib, dev):
    R = lib.wgrad_slab_rows(27, 32, 32, 1)
    nbr, n_in = table_with_rows("same", R, dev)
    x, dy = operands(n_in, 32, R, 32, dev)
    aligned = lib.conv_wgrad(x, dy, nbr)
    xm, dym = (misaligned(x), dy) if which == "x" else (x, misaligned(dy))
    got = _check_wgrad(lib, xm, dym, nbr, f"{which} misaligned")
    assert torch.equal(got, aligned)                # the same values in the same order, whichever loads fetched them


def test_conv_wgrad_entries_outside_the_input_are_absent(lib, dev):
    nbr, n_in = table_with_rows("same", None, dev)
    bad = table_out_of_range(nbr, n_in)
    absent = torch.where((bad >= 0) & (bad < n_in), bad, torch.full_like(bad, -1))
    assert int((bad >= n_in).sum()) > 100 and int((bad == -7).sum()) > 100
    for cin, cout in ((32, 32), (129, 130)):        # vector and scalar loads
        x, dy = operands(n_in, cin, nbr.shape[1], cout, dev)
        got = _check_wgrad(lib, x, dy, bad, f"out-of-range entries {cin}x{cout}")
        assert torch.equal(got, lib.conv_wgrad(x, dy, absent))


def test_conv_wgrad_constant_is_below_the_a_priori_cap(lib):
    R = lib.wgrad_slab_rows(27, 64, 64, 1)
    assert C_WGRAD < sum_cap(2 * R + 3)           # the row count of the three-slab case the constant was calibrated on


def test_conv_wgrad_absent_offset_and_no_rows(lib, dev):
    nbr, n_in = table_with_rows("same", None, dev)
    nbr = nbr.clone()
    nbr[11] = -1
    x, dy = operands(n_in, 32, nbr.shape[1], 32, dev)
    got = _check_wgrad(lib, x, dy, nbr, "absent offset")
    assert bool((got[11] == 0).all()) and bool((got[13] != 0).any())
    out = torch.full((27, 32, 32), 7.0, device=dev)
    lib.conv_wgrad(x, torch.empty((0, 32), device=dev), torch.empty((27, 0), dtype=torch.int32, device=dev), out=out)
    assert bool((out == 0).all())                 # overwritten with exact zeros


def test_conv_wgrad_overwrites_and_repeats_bit_for_bit(lib, dev):
    R = lib.wgrad_slab_rows(27, 32, 32, 1)
    for rows in (R, 2 * R + 3):                   # one slab, three slabs
        nbr, n_in = table_with_rows("same", rows, dev)
        assert -(-rows // lib.wgrad_slab_rows(27, 32, 32, rows)) == (1 if rows == R else 3)
        x, dy = operands(n_in, 32, rows, 32, dev)
        first = lib.conv_wgrad(x, dy, nbr)
        again = lib.conv_wgrad(x, dy, nbr, out=torch.full_like(first, 3.0))
        assert torch.equal(first, again)


# ---- input gradient: the forward kernels over the inverse table -------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_input_gradient_through_conv_function(kind, lib, dev):
    m = make_map(kind, dev)
    torch.manual_seed(2)
    mod = make_module(kind, 32, 64).to(dev).train()
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(m["n_in"], 32, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(m["n_out"], 64, generator=g).to(dev)
    out = mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"]))
    assert out.F.grad_fn is not None
    out.F.backward(dy)
    inv = invert_torch(m["nbr"], m["n_in"])       # built in torch, not by pg_nbr_invert
    w_t = mod.kernel.detach().transpose(1, 2).contiguous()
    acc, mag = gather_sum64(dy, w_t, inv, torch.arange(m["n_in"], device=dev))
    bad = violations(feats.grad, acc, mag, acc.abs())
    print(f"input gradient {kind}: worst err / A = {worst_ratio(feats.grad, acc, mag, acc.abs()):.3e}")
    assert not bool(bad.any()), int(bad.sum())


@pytest.mark.parametrize("case", DGRAD_CASES, ids=[f"{c[0]}to{c[1]}_{c[2]}" for c in DGRAD_CASES])
def test_input_gradient_shapes(case, lib, dev):
    cin, cout, kind = case
    m = make_map(kind, dev)
    torch.manual_seed(2)
    mod = make_module(kind, cin, cout).to(dev).train()
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(m["n_in"], cin, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(m["n_out"], cout, generator=g).to(dev)
    out = mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"]))
    assert out.F.grad_fn is not None
    out.F.backward(dy)
    inv = invert_torch(m["nbr"], m["n_in"])
    w_t = mod.kernel.detach().transpose(1, 2).contiguous()
    acc, mag = gather_sum64(dy, w_t, inv, torch.arange(m["n_in"], device=dev))
    bad = violations(feats.grad, acc, mag, acc.abs())
    print(f"input gradient {cin} -> {cout} {kind}: worst err / A = {worst_ratio(feats.grad, acc, mag, acc.abs()):.3e}")
    assert feats.grad.shape == feats.shape and not bool(bad.any()), int(bad.sum())


# ---- pg_colsum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 4099, COLSUM_ROWS, COLSUM_ROWS + 1])
@pytest.mark.parametrize("c", [1, 20, 256, 65])
def test_colsum(n, c, lib, dev):
    dy = operands(0, 1, n, c, dev, seed=n + c)[1]
    got = lib.colsum(dy)
    ref = dy.double().sum(0)
    bound = sum_cap(n) * dy.double().abs().sum(0) + 1e-30
    assert got.shape == (c,)
    assert bool(((got.double() - ref).abs() <= bound).all())
    assert torch.equal(got, lib.colsum(dy, out=torch.full_like(got, 5.0)))
    assert bool((lib.colsum(torch.empty((0, c), device=dev)) == 0).all())


# ---- the stack and the modules ----------------------------------------------------------------------------------------------
def test_stack_gradients_against_the_fp64_twin(lib, dev):
    ratios = stack_ratios(dev)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 11
    for name, r in ratios.items():
        assert r <= STACK_M, f"{name}: max |g - g64| = {r:.2f} x max |g32 - g64|, bound {STACK_M}"


@pytest.mark.parametrize("kind", KINDS)
def test_module_gradients_have_the_parameter_shapes_and_accumulate(kind, lib, dev):
    m = make_map(kind, dev)
    torch.manual_seed(4)
    mod = make_module(kind, 16, 20).to(dev).train()
    feats = operands(m["n_in"], 16, 0, 1, dev)[0]

    def step():
        out = mod(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"]))
        out.F.square().sum().backward()

    step()
    assert mod.kernel.grad.shape == mod.kernel.shape and mod.bias.grad.shape == mod.bias.shape
    k1, b1 = mod.kernel.grad.clone(), mod.bias.grad.clone()
    step()                                         # torch accumulates into .grad; the kernels overwrite their own output
    assert torch.equal(mod.kernel.grad, k1 + k1) and torch.equal(mod.bias.grad, b1 + b1)
