"""Test helper: the maps, inputs and the case table of the gradient tests (tests/test_grad_cpu.py, tests/test_hip_grad.py).

Maps: random occupancy (~40 %) in a 12 x 12 x 6 box, batch 2, built through a real CoordinateManager; `reps` copies of the box
side by side along x where a test needs more rows than one box gives."""
import numpy as np
import torch
import torch.nn as nn

import pasco_amd.me as ME
from pasco_amd.me.core import CoordinateManager

KINDS = ("same", "down", "gen")
BOX = (12, 12, 6)

# pg_conv_wgrad: (name, kind, cin, cout, rows) - rows: an int, None = the natural map, or a function of the slab length R
WGRAD_CASES = [
    ("3x20_one_row", "same", 3, 20, lambda R: 1),
    ("32x32_R-1", "same", 32, 32, lambda R: R - 1),
    ("32x32_R", "same", 32, 32, lambda R: R),
    ("32x32_R+1", "same", 32, 32, lambda R: R + 1),
    ("64x64_2R+3", "same", 64, 64, lambda R: 2 * R + 3),
    ("33x65_257", "same", 33, 65, lambda R: 257),
    ("32x64_strided", "down", 32, 64, None),
    ("64x32_generative", "gen", 64, 32, None),
    ("128x256_65", "same", 128, 256, lambda R: 65),
]


def box_coords(seed: int, reps: int = 1) -> torch.Tensor:
    rng = np.random.default_rng(seed)
    out = []
    for r in range(reps):
        occ = rng.random((2,) + BOX) < 0.4
        c = np.argwhere(occ).astype(np.int32)
        c[:, 1] += 16 * r                    # a gap of 4 between the copies: an even offset keeps the strided cells apart
        out.append(c)
    c = np.concatenate(out)
    return torch.from_numpy(c[rng.permutation(len(c))].copy())


def make_map(kind: str, device, seed: int = 0, reps: int = 1):
    """-> dict(mgr, in_key, out_key, nbr int32 [K, n_out], n_in, n_out, module kwargs)."""
    mgr = CoordinateManager(D=3, device=device)
    key, _ = mgr.insert_and_map(box_coords(seed, reps).to(device), 1)
    if kind == "same":
        in_key = out_key = key
        nbr = mgr.kernel_map(key, key, 3)
    elif kind == "down":
        in_key, out_key = key, mgr.stride(key, 2)
        nbr = mgr.kernel_map(in_key, out_key, 2)
    else:
        in_key = mgr.stride(key, 2)
        out_key = mgr.expand(in_key, 2)
        nbr = mgr.kernel_map(in_key, out_key, 2, transposed=True)
    return dict(mgr=mgr, in_key=in_key, out_key=out_key, nbr=nbr, n_in=mgr.size(in_key), n_out=mgr.size(out_key))


def make_module(kind: str, cin: int, cout: int, bias: bool = True):
    if kind == "same":
        return ME.MinkowskiConvolution(cin, cout, kernel_size=3, bias=bias, dimension=3)
    if kind == "down":
        return ME.MinkowskiConvolution(cin, cout, kernel_size=2, stride=2, bias=bias, dimension=3)
    return ME.MinkowskiGenerativeConvolutionTranspose(cin, cout, kernel_size=2, stride=2, bias=bias, dimension=3)


def table_with_rows(kind: str, rows, device, seed: int = 0):
    """A neighbour table of `kind` with exactly `rows` output rows (None: the natural map of one box): the box is tiled until the
    map has enough rows, then the table is cut.  -> (nbr, n_in)."""
    reps = 1
    while True:
        m = make_map(kind, device, seed, reps)
        if rows is None or m["n_out"] >= rows:
            break
        reps += 1
    nbr = m["nbr"] if rows is None else m["nbr"][:, :rows].contiguous()
    return nbr, m["n_in"]


def operands(n_in: int, cin: int, n_out: int, cout: int, device, seed: int = 1):
    """x [n_in, cin], dy [n_out, cout]: normal values, one row of large ones (1e4) and one column of tiny ones (1e-6) each."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_in, cin, generator=g)
    dy = torch.randn(n_out, cout, generator=g)
    for t in (x, dy):
        if t.shape[0]:
            t[t.shape[0] // 2] *= 1e4
            t[:, t.shape[1] // 2] *= 1e-6
    return x.to(device), dy.to(device)


class Stack(nn.Module):
    """conv 3^3 (3 -> 32) -> BatchNorm (training) -> ReLU -> conv k2 / s2 (32 -> 64) -> conv 3^3 (64 -> 64) -> generative
    transpose (64 -> 32) -> pruning with a fixed mask -> two-map + with the first layer's output -> k = 1 conv (32 -> 20)."""

    def __init__(self):
        super().__init__()
        self.c1 = ME.MinkowskiConvolution(3, 32, kernel_size=3, bias=True, dimension=3)
        self.bn = ME.MinkowskiBatchNorm(32)
        self.relu = ME.MinkowskiReLU()
        self.c2 = ME.MinkowskiConvolution(32, 64, kernel_size=2, stride=2, dimension=3)
        self.c3 = ME.MinkowskiConvolution(64, 64, kernel_size=3, bias=True, dimension=3)
        self.up = ME.MinkowskiGenerativeConvolutionTranspose(64, 32, kernel_size=2, stride=2, dimension=3)
        self.prune = ME.MinkowskiPruning()
        self.head = ME.MinkowskiConvolution(32, 20, kernel_size=1, bias=True, dimension=3)

    def forward(self, x, maps=None):
        mgr, k0 = x.coordinate_manager, x.coordinate_map_key
        y1 = self.c1(x)
        h = self.c2(self.relu(self.bn(y1)))
        k1 = h.coordinate_map_key
        h = self.up(self.c3(h))
        k2 = h.coordinate_map_key
        mask = (torch.arange(h.F.shape[0], device=h.device) % 3) != 1
        hp = self.prune(h, mask)
        u = hp + y1
        out = self.head(u)
        if maps is not None:                  # what the torch twin needs: the tables the modules used
            lookup = {tuple(c): i for i, c in enumerate(u.C.cpu().tolist())}
            b2o = torch.tensor([lookup[tuple(c)] for c in y1.C.cpu().tolist()], dtype=torch.int64, device=x.device)
            assert torch.equal(u.C[:hp.F.shape[0]], hp.C)
            maps.update(nbr1=mgr.kernel_map(k0, k0, 3), nbr2=mgr.kernel_map(k0, k1, 2), nbr3=mgr.kernel_map(k1, k1, 3),
                        nbr4=mgr.kernel_map(k1, k2, 2, transposed=True), keep=mgr.prune(k2, mask)[1], b2o=b2o,
                        n_union=u.F.shape[0])
        return out


def stack_gradients(device):
    """-> {name: (g, g32, g64)}: the gradient of every parameter of `Stack` (and of the input features, "x") from the modules,
    from the fp32 torch twin and from the fp64 torch twin, on the same maps."""
    from tests.grad_ref64 import stack_twin
    torch.manual_seed(3)
    net = Stack().to(device).train()
    coords = box_coords(5).to(device)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(coords.shape[0], 3, generator=g).to(device).requires_grad_(True)
    x = ME.SparseTensor(feats, coords)
    maps = {}
    out = net(x, maps)
    tgt = torch.randn(out.F.shape, generator=g).to(device)
    (out.F - tgt).square().mean().backward()
    params = dict(net.named_parameters())
    assert x.inverse_mapping is None or x.unique_index is None      # the box has no duplicates: rows are the input rows
    g32 = stack_twin(params, maps, feats, tgt, torch.float32)
    g64 = stack_twin(params, maps, feats, tgt, torch.float64)
    got = {k: v.grad for k, v in params.items()}
    got["x"] = feats.grad
    return {k: (got[k], g32[k], g64[k]) for k in g64}


def stack_ratios(device):
    """name -> max |g - g64| / max |g32 - g64|."""
    out = {}
    for k, (g, g32, g64) in stack_gradients(device).items():
        assert g is not None, f"{k} has no gradient"
        out[k] = float((g.double() - g64).abs().max()) / float((g32.double() - g64).abs().max())
    return out
