"""Test helper: the shared checks of the transposed convolution onto an existing map (`MinkowskiConvolutionTranspose` without
`expand_coordinates`, and `forward(x, coordinates=...)`) for tests/test_convtr_cpu.py and tests/test_hip_convtr.py.

The reference is a dense fp64 twin: the input rows laid into a [B, cin, X/2, Y/2, Z/2] grid, `conv_transpose3d` at stride 2 with
the module's kernel (a child at parent + o_k * ts_out uses kernel[k], k = (oz * 2 + oy) * 2 + ox), read at the target's rows; its
gradients come from torch's autograd in fp64.  The magnitudes the bounds scale with come from the same twin on the absolute
values.  Bounds: those of tests/conv_ref64.py (C_ROUTE * A + EPI_ROUNDING * E: forward and input gradient, every route of the
forward kernels) and tests/grad_ref64.py (C_WGRAD and the a-priori cap of a sum: weight and bias gradient) - what
tests/test_hip_grad.py holds the generative module to."""
import pytest
import torch
import torch.nn.functional as F

import pasco_amd.me as ME
from pasco_amd.me.core import CoordinateManager
from tests.conv_ref64 import bound
from tests.grad_cases import box_coords
from tests.grad_ref64 import C_WGRAD, sum_cap

SHAPES = [(4, 8), (16, 16), (64, 32)]            # (16, 16): the guarded split route on the device
DIMS = (2, 16, 16, 8)                            # B, X, Y, Z: the box of tests/grad_cases.py (12 x 12 x 6) fits


def maps(device, seed=0):
    """-> (mgr, key0 at tensor stride 1, key1 = stride(key0, 2))."""
    mgr = CoordinateManager(D=3, device=device)
    key0, _ = mgr.insert_and_map(box_coords(seed).to(device), 1)
    return mgr, key0, mgr.stride(key0, 2)


def make_up(cin, cout, bias, device, seed=4, **kw):
    torch.manual_seed(seed)
    return ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=2, stride=2, bias=bias, dimension=3, **kw).to(device)


def feats_on(mgr, key, c, device, seed=6, grad=False):
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(mgr.size(key), c, generator=g)
    f[f.shape[0] // 2] *= 100.0
    return f.to(device).requires_grad_(grad)


def twin(x, in_coords, ts_in, kernel, bias, out_coords, dy=None):
    """fp64: -> (out [n_out, cout], (dx, dw, db) for the upstream gradient `dy`, or None)."""
    x = x.detach().double().cpu().requires_grad_(True)
    k = kernel.detach().double().cpu().requires_grad_(True)
    b = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    cin, cout = k.shape[1], k.shape[2]
    B, X, Y, Z = DIMS
    ic, oc = in_coords.long().cpu(), out_coords.long().cpu()
    ts_out = ts_in // 2
    dense = torch.zeros((B, X // 2, Y // 2, Z // 2, cin), dtype=torch.float64)
    dense = dense.index_put((ic[:, 0], ic[:, 1] // ts_in, ic[:, 2] // ts_in, ic[:, 3] // ts_in), x)
    w = k.reshape(2, 2, 2, cin, cout).permute(3, 4, 2, 1, 0)                       # [cin, cout, ox, oy, oz]
    full = F.conv_transpose3d(dense.permute(0, 4, 1, 2, 3), w, stride=2).permute(0, 2, 3, 4, 1)
    out = full[oc[:, 0], oc[:, 1] // ts_out, oc[:, 2] // ts_out, oc[:, 3] // ts_out]
    if b is not None:
        out = out + b.reshape(1, -1)
    if dy is None:
        return out.detach(), None
    grads = torch.autograd.grad(out, [x, k] + ([b] if b is not None else []), grad_outputs=dy.detach().double().cpu())
    return out.detach(), (grads[0], grads[1], grads[2] if b is not None else None)


def within(got, want, bnd, what):
    err = (got.detach().double().cpu() - want).abs()
    ratio = float((err / bnd.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{what}: worst err / bound = {ratio:.3f}")
    assert got.shape == want.shape and bool((err <= bnd).all()), f"{what}: worst err / bound = {ratio:.3f}"


def check_forward(device, cin, cout, bias):
    mgr, key0, key1 = maps(device)
    up = make_up(cin, cout, bias, device).eval()
    x = feats_on(mgr, key1, cin, device)
    with torch.no_grad():
        y = up(ME.SparseTensor(x, coordinate_map_key=key1, coordinate_manager=mgr))
    assert y.coordinate_map_key is key0 and y.tensor_stride == [1, 1, 1] and y.F.shape == (mgr.size(key0), cout)
    c1, c0 = mgr.get_coordinates(key1), mgr.get_coordinates(key0)
    want, _ = twin(x, c1, 2, up.kernel, up.bias, c0)
    mag, _ = twin(x.abs(), c1, 2, up.kernel.abs(), None if up.bias is None else up.bias.abs(), c0)
    within(y.F, want, bound(mag, mag), f"forward {cin} -> {cout} bias={bias}")
    return mgr, key0, key1, up, x, y


def check_map_identity(device):
    """The target's key IS the encoder's key, `cat` with the skip succeeds, and the same after a `stride_chain`."""
    mgr, key0, key1 = maps(device)
    up = make_up(8, 4, False, device).eval()
    skip = ME.SparseTensor(feats_on(mgr, key0, 3, device), coordinate_map_key=key0, coordinate_manager=mgr)
    with torch.no_grad():
        y = up(ME.SparseTensor(feats_on(mgr, key1, 8, device), coordinate_map_key=key1, coordinate_manager=mgr))
        assert y.coordinate_map_key is skip.coordinate_map_key and mgr.transposed_target(key1, 2) is key0
        n_maps = len(mgr._maps)
        both = ME.cat(y, skip)
        assert both.F.shape == (mgr.size(key0), 7) and both.coordinate_map_key == key0
        four = ME.SparseTensor(feats_on(mgr, key0, 4, device, seed=8), coordinate_map_key=key0, coordinate_manager=mgr)
        added = y + four                                         # the two-map + sees one map: a row-wise sum, no union
        assert added.coordinate_map_key == key0 and torch.equal(added.F, y.F + four.F)
        assert len(mgr._maps) == n_maps, "no map is registered by the transposed convolution or the concatenation"
    mgr2 = CoordinateManager(D=3, device=device)
    k0, _ = mgr2.insert_and_map(box_coords(1).to(device), 1)
    k1, k2 = mgr2.stride_chain(k0, 2)
    up2 = make_up(8, 8, False, device).eval()
    with torch.no_grad():
        a = up2(ME.SparseTensor(feats_on(mgr2, k2, 8, device), coordinate_map_key=k2, coordinate_manager=mgr2))
        assert a.coordinate_map_key is k1 and a.tensor_stride == [2, 2, 2]
        b = up2(a)
        assert b.coordinate_map_key is k0
        ME.cat(b, ME.SparseTensor(feats_on(mgr2, k0, 2, device), coordinate_map_key=k0, coordinate_manager=mgr2))
    want, _ = twin(a.F, mgr2.get_coordinates(k1), 2, up2.kernel, None, mgr2.get_coordinates(k0))
    mag, _ = twin(a.F.abs(), mgr2.get_coordinates(k1), 2, up2.kernel.abs(), None, mgr2.get_coordinates(k0))
    within(b.F, want, bound(mag, mag), "second level of a stride_chain")


def check_gradients(device, cin, cout):
    mgr, key0, key1 = maps(device)
    up = make_up(cin, cout, True, device).train()
    x = feats_on(mgr, key1, cin, device, grad=True)
    y = up(ME.SparseTensor(x, coordinate_map_key=key1, coordinate_manager=mgr))
    assert y.F.grad_fn is not None and y.coordinate_map_key is key0
    dy = feats_on(mgr, key0, cout, device, seed=9)
    y.F.backward(dy)
    c1, c0 = mgr.get_coordinates(key1), mgr.get_coordinates(key0)
    _, (dx, dw, db) = twin(x, c1, 2, up.kernel, up.bias, c0, dy)
    _, (mx, mw, mb) = twin(x.abs(), c1, 2, up.kernel.abs(), up.bias.abs(), c0, dy.abs())
    n_out = mgr.size(key0)
    within(x.grad, dx, bound(mx, mx), f"dX {cin} -> {cout}")
    within(up.kernel.grad, dw, min(C_WGRAD, sum_cap(n_out)) * mw + 1e-30, f"dW {cin} -> {cout}")
    within(up.bias.grad, db, sum_cap(n_out) * mb + 1e-30, f"db {cin} -> {cout}")
    first = (x.grad.clone(), up.kernel.grad.clone(), up.bias.grad.clone())
    x.grad = up.kernel.grad = up.bias.grad = None
    up(ME.SparseTensor(x, coordinate_map_key=key1, coordinate_manager=mgr)).F.backward(dy)
    assert torch.equal(first[0], x.grad) and torch.equal(first[1], up.kernel.grad) and torch.equal(first[2], up.bias.grad)


def check_against_generative(device, cin=16, cout=16):
    """The same weights in `MinkowskiGenerativeConvolutionTranspose`, its rows gathered at the target's coordinates."""
    mgr, key0, key1, up, x, y = check_forward(device, cin, cout, True)
    gen = ME.MinkowskiGenerativeConvolutionTranspose(cin, cout, kernel_size=2, stride=2, bias=True, dimension=3).to(device).eval()
    gen.load_state_dict(up.state_dict())
    with torch.no_grad():
        z = gen(ME.SparseTensor(x, coordinate_map_key=key1, coordinate_manager=mgr))
    assert z.F.shape[0] == 8 * mgr.size(key1) and z.coordinate_map_key != key0
    row = {tuple(c): i for i, c in enumerate(z.C.cpu().tolist())}
    pick = torch.tensor([row[tuple(c)] for c in mgr.get_coordinates(key0).cpu().tolist()], dtype=torch.int64)
    c1, c0 = mgr.get_coordinates(key1), mgr.get_coordinates(key0)
    mag, _ = twin(x.abs(), c1, 2, up.kernel.abs(), up.bias.abs(), c0)
    # the same table call and the same launches: the single bound the generative module itself is held to
    within(y.F, z.F.cpu()[pick].double(), bound(mag, mag), "against the generative module")


def check_coordinates_argument(device):
    """Onto a pruned map, from a pruned input: children without a parent give `bias`, parents without a child drop out."""
    mgr, key0, key1 = maps(device)
    cin, cout = 16, 8
    up = make_up(cin, cout, True, device).eval()
    prune = ME.MinkowskiPruning()
    n0, n1 = mgr.size(key0), mgr.size(key1)
    full_in = ME.SparseTensor(feats_on(mgr, key1, cin, device), coordinate_map_key=key1, coordinate_manager=mgr)
    skip = ME.SparseTensor(feats_on(mgr, key0, 2, device), coordinate_map_key=key0, coordinate_manager=mgr)
    with torch.no_grad():
        x = prune(full_in, (torch.arange(n1, device=device) % 3) != 0)
        target = prune(skip, (torch.arange(n0, device=device) % 5) != 1)
        with pytest.raises(ValueError, match="coordinates=.*expand_coordinates=True"):
            up(x)                                                # a pruned map has no recorded parent
        y = up(x, coordinates=target.coordinate_map_key)
        y2 = up(x, coordinates=target)
    assert y.coordinate_map_key is target.coordinate_map_key and torch.equal(y.F, y2.F)
    ME.cat(y, target)
    want, _ = twin(x.F, x.C, 2, up.kernel, up.bias, target.C)
    mag, _ = twin(x.F.abs(), x.C, 2, up.kernel.abs(), up.bias.abs(), target.C)
    within(y.F, want, bound(mag, mag), "coordinates= onto a pruned map")
    have = {tuple(c) for c in x.C.cpu().tolist()}
    orphan = torch.tensor([(c[0], c[1] // 2 * 2, c[2] // 2 * 2, c[3] // 2 * 2) not in have for c in target.C.cpu().tolist()])
    assert 0 < int(orphan.sum()) < orphan.numel()
    assert torch.equal(y.F.cpu()[orphan], up.bias.detach().cpu().expand(int(orphan.sum()), cout)), "a child without a parent is the bias"
    kept = {(c[0], c[1] // 2 * 2, c[2] // 2 * 2, c[3] // 2 * 2) for c in target.C.cpu().tolist()}
    assert have - kept, "the case has parents without a child in the target"


def check_modes_and_prologue(device):
    mgr, key0, key1 = maps(device)
    cin, cout = 16, 16
    up = make_up(cin, cout, True, device).eval()
    x = feats_on(mgr, key1, cin, device, grad=True)
    sp = lambda f: ME.SparseTensor(f, coordinate_map_key=key1, coordinate_manager=mgr)
    a = up(sp(x)).F
    assert a.grad_fn is not None
    with torch.no_grad():
        b = up(sp(x.detach())).F
    with torch.inference_mode():
        c = up(sp(x.detach())).F
    assert torch.equal(a.detach(), b) and torch.equal(b, c), "the three grad modes give the same forward bits"
    # a pending eval-mode BatchNorm -> ReLU is applied to the operand first
    bn, relu = ME.MinkowskiBatchNorm(cin).to(device).eval(), ME.MinkowskiReLU()
    with torch.no_grad():
        bn.bn.running_mean.copy_(torch.linspace(-1, 1, cin))
        bn.bn.running_var.copy_(torch.linspace(0.5, 2, cin))
        bn.bn.weight.copy_(torch.linspace(0.5, 1.5, cin))
        bn.bn.bias.copy_(torch.linspace(-0.3, 0.3, cin))
        h = relu(bn(sp(x.detach())))
        pending = h._pending is not None
        y = up(h)
    scale, shift = (t.double().cpu() for t in bn.folded())
    xd = x.detach().double().cpu()
    operand, operand_mag = torch.relu(xd * scale + shift), xd.abs() * scale.abs() + shift.abs()
    c1, c0 = mgr.get_coordinates(key1), mgr.get_coordinates(key0)
    want, _ = twin(operand, c1, 2, up.kernel, up.bias, c0)
    mag, _ = twin(operand_mag, c1, 2, up.kernel.abs(), up.bias.abs(), c0)
    within(y.F, want, bound(mag, mag), f"behind a deferred BatchNorm -> ReLU (pending: {pending})")
    assert y.coordinate_map_key is key0
    return pending


def check_refusals(device):
    mgr, key0, key1 = maps(device)
    up = make_up(4, 4, False, device).eval()
    x = ME.SparseTensor(feats_on(mgr, key1, 4, device), coordinate_map_key=key1, coordinate_manager=mgr)
    with torch.no_grad():
        # no recorded parent: a map made by insert
        lone = ME.SparseTensor(feats_on(mgr, key1, 4, device), mgr.get_coordinates(key1).clone(), tensor_stride=2)
        with pytest.raises(ValueError, match=r"made by insert, prune, union or expand.*coordinates=.*expand_coordinates=True"):
            up(lone)
        with pytest.raises(ValueError, match="made by insert"):
            up(ME.SparseTensor(feats_on(mgr, key0, 4, device), coordinate_map_key=key0, coordinate_manager=mgr))   # stride 1: nothing below
        # a recorded parent at another stride than in / stride: the message names the parent's stride, not how the map was made
        key4 = mgr.stride(key0, 4)
        with pytest.raises(ValueError, match=r"strided from a map of tensor stride \[1, 1, 1\].*lands on tensor stride \[2, 2, 2\].*coordinates="):
            up(ME.SparseTensor(feats_on(mgr, key4, 4, device), coordinate_map_key=key4, coordinate_manager=mgr))
        # coordinates=: the wrong stride, a foreign manager (key and tensor), a coordinate tensor
        with pytest.raises(ValueError, match=r"tensor stride \[2, 2, 2\].*lands on \[1, 1, 1\]"):
            up(x, coordinates=key1)
        other, okey0, _ = maps(device, seed=2)
        with pytest.raises(ValueError, match="no coordinate map of the input's manager"):
            up(x, coordinates=okey0)
        with pytest.raises(ValueError, match="another coordinate manager"):
            up(x, coordinates=ME.SparseTensor(feats_on(other, okey0, 1, device), coordinate_map_key=okey0, coordinate_manager=other))
        with pytest.raises(ValueError, match="a coordinate tensor is not served"):
            up(x, coordinates=mgr.get_coordinates(key0))
        # kernel != stride stays refused, and says so
        k3 = ME.MinkowskiConvolutionTranspose(4, 4, kernel_size=3, stride=2, dimension=3).to(device)
        with pytest.raises(ValueError, match="kernel != stride is not served"):
            k3(x)
        # the generative module generates its own map; the plain convolution keeps its refusal
        gen = ME.MinkowskiGenerativeConvolutionTranspose(4, 4, kernel_size=2, stride=2, dimension=3).to(device)
        with pytest.raises(ValueError, match="generates its own output map"):
            gen(x, coordinates=key0)
        with pytest.raises(AssertionError, match="explicit output coordinates"):
            ME.MinkowskiConvolution(4, 4, kernel_size=3, dimension=3).to(device)(x, coordinates=key1)
        with pytest.raises(AssertionError, match="explicit output coordinates"):
            ME.MinkowskiConvolution(4, 4, kernel_size=1, dimension=3).to(device)(x, coordinates=key1)
