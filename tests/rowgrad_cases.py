"""Test helper: the cases of the dense <-> rows and max-pooling gradient tests (tests/test_rowgrad_cpu.py on the host restatement
and the CPU oracle, tests/test_hip_rowgrad.py on the pr_* kernels) and the checks the two files share.  `ops` is whatever serves
`dense_rows / rows_dense / maxpool_arg / maxpool_bwd`: `pasco_amd.grad.host` or the `RowGradLib` binding."""
import itertools

import numpy as np
import torch
import torch.nn as nn

import pasco_amd.me as ME
from tests.grad_cases import box_coords, make_map
from tests.grad_ref64 import invert_torch
from tests.rowgrad_ref import (dense_rows_ref, dense_twin, maxpool_arg_loop, maxpool_bwd_ref, maxpool_out_ref, row_stack_twin,
                               rows_dense_ref, to_sparse_twin)

GRIDS = ((12, 12, 6), (5, 7, 3))
BATCH = 2
ROWS = (0, 1, 63, 64, 65, 131)             # around the 64-row tile; 131 = two tiles and a tail
CHANNELS = (1, 3, 63, 64, 65, 96)          # around the 64-channel tile
STRIDES = (1, 2, 8)
MINS = ((0, 0, 0), (-8, 0, 8))
POOL_CHANNELS = (1, 20, 64)
EPS = 2.0 ** -24


def site_rows(grid, n, seed, permute):
    """n distinct sites of the [BATCH, *grid] grid as int32 [n, 4], in to_sparse (lexicographic) order or randomly permuted."""
    rng = np.random.default_rng(seed)
    total = BATCH * grid[0] * grid[1] * grid[2]
    flat = np.sort(rng.choice(total, size=n, replace=False))
    if permute:
        flat = flat[rng.permutation(n)]
    b, x, y, z = np.unravel_index(flat, (BATCH,) + tuple(grid))
    return torch.from_numpy(np.stack([b, x, y, z], axis=1).astype(np.int32)).reshape(n, 4)


def coords_of(sites, min3, ts):
    """Coordinates whose site is `sites`: site * ts + min, plus i % ts on every axis so that the division has to floor."""
    c = sites.clone()
    off = (torch.arange(sites.shape[0], dtype=torch.int32) % ts)[:, None]
    c[:, 1:] = sites[:, 1:] * ts + torch.tensor(min3, dtype=torch.int32) + off
    return c


def values(shape, seed, device):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(device)


# ---- pr_dense_rows / pr_rows_dense ------------------------------------------------------------------------------------------
def check_dense_rows(ops, device, grid, C):
    dense = values((BATCH, C) + tuple(grid), 7 * C, device)
    for n, ts, min3, permute in itertools.product(ROWS, STRIDES, MINS, (False, True)):
        coords = coords_of(site_rows(grid, n, n + ts, permute), min3, ts).to(device)
        got = ops.dense_rows(dense, coords, min3, ts)
        assert got.shape == (n, C)
        assert torch.equal(got, dense_rows_ref(dense, coords, min3, ts)), (grid, C, n, ts, min3, permute)
        assert torch.equal(got, ops.dense_rows(dense, coords, min3, ts))


def check_dense_rows_edges(ops, device, grid, C, ts=2, min3=(-8, 0, 8)):
    """Rows that wrap, two rows on one site, rows beyond -dim, at or above dim, and batch indices outside."""
    X, Y, Z = grid
    site = [                     # (b, x, y, z) in site units, before the wrap
        (0, 1, 2, 1),            # 0  plain
        (1, -1, 2, 1),           # 1  wraps to x = X - 1
        (1, X - 1, 2, 1),        # 2  the same site directly: rows 1 and 2 both receive it
        (0, -X, -Y, -Z),         # 3  wraps to (0, 0, 0) on every axis
        (0, -X - 1, 2, 1),       # 4  beyond -dim: zero row
        (0, 1, Y, 1),            # 5  at dim: zero row
        (0, 1, 2, Z + 3),        # 6  above dim: zero row
        (-1, 1, 2, 1),           # 7  batch index below: zero row
        (BATCH, 1, 2, 1),        # 8  batch index above: zero row
        (1, 0, -1, -1),          # 9  wraps on two axes
    ]
    sites = torch.tensor(site * 8, dtype=torch.int32)                     # 80 rows: more than one tile
    coords = coords_of(sites, min3, ts).to(device)
    dense = values((BATCH, C) + tuple(grid), 3, device)
    got = ops.dense_rows(dense, coords, min3, ts)
    assert torch.equal(got, dense_rows_ref(dense, coords, min3, ts))
    assert torch.equal(got[1], dense[1, :, X - 1, 2, 1]) and torch.equal(got[1], got[2])
    assert torch.equal(got[3], dense[0, :, 0, 0, 0]) and torch.equal(got[9], dense[1, :, 0, Y - 1, Z - 1])
    for r in (4, 5, 6, 7, 8):
        assert bool((got[r::10] == 0).all()), r
    assert bool((got[0::10] != 0).any())


def check_rows_dense(ops, device, grid, C):
    shape5 = (BATCH, C) + tuple(grid)
    for n, permute in itertools.product(ROWS, (False, True)):
        sc = site_rows(grid, n, 3 * n + 1, permute).to(device)
        rows = values((n, C), n + C, device)
        rows = torch.where(rows == 0, torch.ones_like(rows), rows)
        got = ops.rows_dense(rows, sc, shape5)
        assert tuple(got.shape) == shape5
        assert torch.equal(got, rows_dense_ref(rows, sc, shape5)), (grid, C, n, permute)
        assert int((got != 0).sum()) == n * C                                  # every untouched element exactly 0
        assert torch.equal(got, ops.rows_dense(rows, sc, shape5))
    # rows with an index out of range are skipped
    sc = site_rows(grid, 70, 5, True)
    bad = {3: (0, -1, 0, 0), 17: (0, 0, grid[1], 0), 40: (BATCH, 0, 0, 0), 64: (-1, 1, 1, 1), 69: (1, 0, 0, grid[2])}
    for r, c in bad.items():
        sc[r] = torch.tensor(c, dtype=torch.int32)
    sc = sc.to(device)
    rows = values((70, C), 9, device) + 5.0
    got = ops.rows_dense(rows, sc, shape5)
    assert torch.equal(got, rows_dense_ref(rows, sc, shape5))
    assert int((got != 0).sum()) == (70 - len(bad)) * C


# ---- max pooling ------------------------------------------------------------------------------------------------------------
def pool_case(kind, C, device, seed=0):
    """-> (x, nbr, n_in): the kernel 2 / stride 2 ("down") or kernel 3 / stride 1 ("same") table of tests/grad_cases.make_map with
    one window emptied by hand; x holds small integers (repeated maxima inside a window) and zeros of both signs."""
    m = make_map(kind, device, seed)
    nbr = m["nbr"].clone()
    nbr[:, 3] = -1                                   # an empty window
    g = torch.Generator().manual_seed(seed + C)
    x = torch.randint(-2, 3, (m["n_in"], C), generator=g).float()
    x = torch.where((x == 0) & (torch.rand(x.shape, generator=g) < 0.5), -torch.zeros_like(x), x)
    rows = nbr[:, 5][nbr[:, 5] >= 0].long().cpu()    # window 5, channel 0: zeros of alternating sign, -0 first
    x[rows, 0] = torch.tensor([-0.0, 0.0] * len(rows))[:len(rows)]
    return x.to(device), nbr, m["n_in"]


def check_maxpool(ops, be, device, kind, C):
    x, nbr, n_in = pool_case(kind, C, device)
    K, n_out = nbr.shape
    out = be.maxpool_fwd(x, nbr)
    assert torch.equal(out, maxpool_out_ref(x, nbr))
    arg = ops.maxpool_arg(x, nbr, out)
    assert arg.dtype == torch.int32 and torch.equal(arg, maxpool_arg_loop(x, nbr, out))
    assert bool((arg[3] == -1).all()) and bool((arg[torch.arange(n_out, device=device) != 3] >= 0).all())
    first = nbr[:, 5][nbr[:, 5] >= 0][0]             # +0 and -0 tie: the first present offset of the all-zero window
    assert float(out[5, 0]) == 0 and int(arg[5, 0]) == int(first)
    dy = values((n_out, C), 17 + C, device)
    inv = invert_torch(nbr, n_in)
    dx = ops.maxpool_bwd(dy, arg, inv, n_in)
    assert torch.equal(dx, ops.maxpool_bwd(dy, arg, inv, n_in))
    ref32, _ = maxpool_bwd_ref(dy, arg, n_in, torch.float32)
    ref64, mag = maxpool_bwd_ref(dy, arg, n_in, torch.float64)
    if kind == "down":                               # kernel == stride: one term, a copy
        assert torch.equal(dx, ref32)
    err = (dx.double() - ref64).abs()
    assert bool((err <= (K - 1) * EPS * mag).all()), float((err / (mag + 1e-300)).max())
    nonempty = (nbr >= 0).any(dim=0)
    total = dy.double()[nonempty]
    assert abs(float(dx.double().sum() - total.sum())) <= (K - 1) * EPS * float(total.abs().sum())
    # a NaN maximum compares equal to nothing: no row receives its gradient
    xn = x.clone()
    xn[nbr[:, 0][nbr[:, 0] >= 0].long(), 0] = float("nan")
    out_n = be.maxpool_fwd(xn, nbr)
    arg_n = ops.maxpool_arg(xn, nbr, out_n)
    assert bool(torch.isnan(out_n[0, 0])) and int(arg_n[0, 0]) == -1
    assert torch.equal(arg_n, maxpool_arg_loop(xn, nbr, out_n))


# ---- the autograd layer -------------------------------------------------------------------------------------------------------
def _sparse(feats, m):
    return ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])


def check_dense_autograd(be, device):
    m = make_map("same", device)
    mgr, key = m["mgr"], m["in_key"]
    coords = mgr.get_coordinates(key)
    feats = values((m["n_in"], 5), 1, device)
    shape5, min3 = (2, 5, 16, 10, 6), (4, 0, 0)          # x: indices -4 .. -1 wrap to 12 .. 15; y: 10 and 11 are cut off
    args = dict(shape=torch.Size(shape5), min_coordinate=torch.IntTensor(min3))
    today = be.to_dense(feats, coords, min3, 1, (2, 16, 10, 6))
    for f, ctx in ((feats, torch.enable_grad()), (feats.clone().requires_grad_(True), torch.no_grad())):
        with ctx:
            d = _sparse(f, m).dense(**args)[0]
        assert d.grad_fn is None and torch.equal(d, today)
    f = feats.clone().requires_grad_(True)
    d = _sparse(f, m).dense(**args)[0]
    assert d.grad_fn is not None and torch.equal(d.detach(), today)
    g = values(shape5, 2, device)
    d.backward(g)
    twin = feats.clone().requires_grad_(True)
    dense_twin(twin, coords, min3, 1, shape5).backward(g)
    assert torch.equal(f.grad, twin.grad)
    assert bool((f.grad == 0).all(dim=1).any()) and bool((f.grad != 0).any())   # skipped rows are there and get zero rows
    # X = 7: the wrapped rows land on sites that other rows hold.  Which row the forward keeps is not stated, so only the
    # gradients are compared: every row of a shared site receives it
    shape5 = (2, 5, 7, 12, 6)
    f = feats.clone().requires_grad_(True)
    g = values(shape5, 3, device)
    _sparse(f, m).dense(shape=torch.Size(shape5), min_coordinate=torch.IntTensor(min3))[0].backward(g)
    twin = feats.clone().requires_grad_(True)
    dense_twin(twin, coords, min3, 1, shape5).backward(g)
    assert torch.equal(f.grad, twin.grad)
    x_idx = coords[:, 1].long() - 4
    a = int(torch.nonzero(x_idx == -1)[0])
    same = torch.nonzero((coords[:, 0] == coords[a, 0]) & (x_idx == 6) & (coords[:, 2:] == coords[a, 2:]).all(dim=1))
    if same.numel():
        assert torch.equal(f.grad[a], f.grad[int(same[0])])


def check_to_sparse_autograd(device):
    x = values((2, 6, 5, 7, 3), 4, device)
    x = x * (values((2, 1, 5, 7, 3), 5, device) > 0.3)          # most sites are empty
    today = ME.to_sparse(x)
    assert today.F.grad_fn is None and 0 < today.F.shape[0] < 2 * 5 * 7 * 3
    with torch.no_grad():
        quiet = ME.to_sparse(x.clone().requires_grad_(True))
    assert quiet.F.grad_fn is None and torch.equal(quiet.F, today.F) and torch.equal(quiet.C, today.C)
    xr = x.clone().requires_grad_(True)
    sp = ME.to_sparse(xr)
    assert sp.F.grad_fn is not None and torch.equal(sp.F.detach(), today.F) and torch.equal(sp.C, today.C)
    assert not sp.C.requires_grad
    g = values(tuple(sp.F.shape), 6, device)
    sp.F.backward(g)
    twin = x.clone().requires_grad_(True)
    to_sparse_twin(twin, today.C).backward(g)
    assert torch.equal(xr.grad, twin.grad)
    assert int((xr.grad != 0).sum()) == int((g != 0).sum())


def check_dedup_autograd(be, device):
    coords = box_coords(2).to(device)
    coords = torch.cat([coords, coords[::3], coords[:5]])         # duplicates of rows seen before
    feats = values((coords.shape[0], 4), 8, device)
    today = ME.SparseTensor(feats, coords)
    uniq = today.unique_index
    assert uniq is not None and today.F.grad_fn is None and torch.equal(today.F, feats[uniq.long()])
    with torch.no_grad():
        quiet = ME.SparseTensor(feats.clone().requires_grad_(True), coords)
    assert quiet.F.grad_fn is None and torch.equal(quiet.F, today.F)
    f = feats.clone().requires_grad_(True)
    st = ME.SparseTensor(f, coords)
    assert st.F.grad_fn is not None and torch.equal(st.F.detach(), today.F)
    g = values(tuple(st.F.shape), 9, device)
    st.F.backward(g)
    twin = feats.clone().requires_grad_(True)
    twin[uniq.long()].backward(g)
    assert torch.equal(f.grad, twin.grad)
    assert bool((f.grad[-5:] == 0).all())                         # dropped duplicates get zero gradient
    # no duplicates: the features pass through as they are
    f2 = feats[:10].clone().requires_grad_(True)
    assert ME.SparseTensor(f2, coords[:10]).F is f2


def check_maxpool_autograd(be, device, ks, stride):
    m = make_map("same", device)
    pool = ME.MinkowskiMaxPooling(ks, stride, dimension=3)
    feats = values((m["n_in"], 20), 10, device)
    out_key = m["mgr"].stride(m["in_key"], stride)
    nbr = m["mgr"].kernel_map(m["in_key"], out_key, ks)
    today = be.maxpool_fwd(feats, nbr)
    for f, ctx in ((feats, torch.enable_grad()), (feats.clone().requires_grad_(True), torch.no_grad())):
        with ctx:
            out = pool(_sparse(f, m))
        assert out.F.grad_fn is None and torch.equal(out.F, today)
    f = feats.clone().requires_grad_(True)
    out = pool(_sparse(f, m))
    assert out.F.grad_fn is not None and torch.equal(out.F.detach(), today)
    g = values(tuple(out.F.shape), 11, device)
    out.F.backward(g)
    arg = maxpool_arg_loop(feats, nbr, today)
    K = nbr.shape[0]
    ref64, mag = maxpool_bwd_ref(g, arg, m["n_in"], torch.float64)
    if ks == stride:
        assert torch.equal(f.grad, maxpool_bwd_ref(g, arg, m["n_in"], torch.float32)[0])
    assert bool(((f.grad.double() - ref64).abs() <= (K - 1) * EPS * mag).all())


# ---- a bottleneck-shaped stack ----------------------------------------------------------------------------------------------
STACK_MIN = (-8, 0, 8)


class RowStack(nn.Module):
    """conv 3^3 (3 -> 16) -> BatchNorm (training) -> ReLU -> conv k2 / s2 (16 -> 32) -> dense(shape, min_coordinate) ->
    nn.Conv3d(32, 32, 3, padding=1) + ReLU -> ME.to_sparse -> ME.SparseTensor(F, C * 2 + min, tensor_stride=2, the first manager)
    -> generative transpose (32 -> 16) -> pruning to the box -> two-map + with the first convolution's output -> k = 1 head;
    and a MinkowskiMaxPooling(2, 2) branch off the first convolution's output (the second output)."""

    def __init__(self):
        super().__init__()
        self.c1 = ME.MinkowskiConvolution(3, 16, kernel_size=3, bias=True, dimension=3)
        self.bn = ME.MinkowskiBatchNorm(16)
        self.relu = ME.MinkowskiReLU()
        self.c2 = ME.MinkowskiConvolution(16, 32, kernel_size=2, stride=2, dimension=3)
        self.dense3d = nn.Conv3d(32, 32, 3, padding=1)
        self.up = ME.MinkowskiGenerativeConvolutionTranspose(32, 16, kernel_size=2, stride=2, dimension=3)
        self.prune = ME.MinkowskiPruning()
        self.head = ME.MinkowskiConvolution(16, 20, kernel_size=1, bias=True, dimension=3)
        self.pool = ME.MinkowskiMaxPooling(2, 2, dimension=3)

    def forward(self, x, maps=None):
        mgr, k0 = x.coordinate_manager, x.coordinate_map_key
        y1 = self.c1(x)
        deepest = self.c2(self.relu(self.bn(y1)))
        k1 = deepest.coordinate_map_key
        shape5 = (2, 32, 6, 6, 3)                                 # the 12 x 12 x 6 box at tensor stride 2
        min_c = torch.IntTensor(STACK_MIN)
        d, _, _ = deepest.dense(shape=torch.Size(shape5), min_coordinate=min_c)
        d = torch.relu(self.dense3d(d))
        sp = ME.to_sparse(d)
        c = sp.C.clone()
        c[:, 1:] = c[:, 1:] * 2 + min_c.to(c.device)
        low = ME.SparseTensor(sp.F, c, tensor_stride=2, coordinate_manager=mgr)
        k2 = low.coordinate_map_key
        h = self.up(low)
        k3 = h.coordinate_map_key
        mask = mgr.find(k0, h.C) >= 0                             # the children inside the input's box
        hp = self.prune(h, mask)
        u = hp + y1
        out = self.head(u)
        pooled = self.pool(y1)
        if maps is not None:                                      # what the torch twin needs: the tables the modules used
            lookup = {tuple(c): i for i, c in enumerate(u.C.cpu().tolist())}
            b2o = torch.tensor([lookup[tuple(c)] for c in y1.C.cpu().tolist()], dtype=torch.int64, device=x.device)
            assert torch.equal(u.C[:hp.F.shape[0]], hp.C) and low.unique_index is None
            maps.update(nbr1=mgr.kernel_map(k0, k0, 3), nbr2=mgr.kernel_map(k0, k1, 2), coords2=mgr.get_coordinates(k1),
                        min3=STACK_MIN, shape5=shape5, sites=sp.C, nbr4=mgr.kernel_map(k2, k3, 2, transposed=True),
                        keep=mgr.prune(k3, mask)[1], b2o=b2o, n_union=u.F.shape[0],
                        nbr_pool=mgr.kernel_map(k0, mgr.stride(k0, 2), 2))
        return out, pooled


def row_stack_gradients(device):
    """-> {name: (g, g32, g64)}: the gradient of every parameter of `RowStack` (the Conv3d's included) and of the input features
    ("x") from the modules, from the fp32 torch twin and from the fp64 torch twin, on the same maps."""
    torch.manual_seed(3)
    net = RowStack().to(device).train()
    coords = box_coords(5)
    coords[:, 1:] += torch.tensor(STACK_MIN, dtype=torch.int32)
    coords = coords.to(device)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(coords.shape[0], 3, generator=g).to(device).requires_grad_(True)
    x = ME.SparseTensor(feats, coords)
    maps = {}
    out, pooled = net(x, maps)
    assert out.F.grad_fn is not None and pooled.F.grad_fn is not None
    tgt = torch.randn(out.F.shape, generator=g).to(device)
    ((out.F - tgt).square().mean() + pooled.F.square().mean()).backward()
    params = dict(net.named_parameters())
    g32 = row_stack_twin(params, maps, feats, tgt, torch.float32)
    g64 = row_stack_twin(params, maps, feats, tgt, torch.float64)
    got = {k: v.grad for k, v in params.items()}
    got["x"] = feats.grad
    return {k: (got[k], g32[k], g64[k]) for k in g64}


def row_stack_ratios(device):
    """name -> max |g - g64| / max |g32 - g64|."""
    out = {}
    for k, (g, g32, g64) in row_stack_gradients(device).items():
        assert g is not None, f"{k} has no gradient"
        assert g.shape == g64.shape
        out[k] = float((g.double() - g64).abs().max()) / float((g32.double() - g64).abs().max())
    return out
