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
    # launch classes (wgrad_geometry below), rows as small as the class allows
    ("128x32_two_ci_tiles", "same", 128, 32, None),
    ("96x40_two_ci_tiles", "same", 96, 40, None),
    ("40x200_four_co_tiles", "same", 40, 200, None),
    ("256x256_R+1_wide_2x2", "same", 256, 256, lambda R: R + 1),
    ("129x130_wide_2x2_scalar", "same", 129, 130, None),
    ("65x96_wide_partial", "same", 65, 96, None),
    ("32x32_33_two_chunks", "same", 32, 32, lambda R: 33),
    ("32x32_64_two_chunks", "same", 32, 32, lambda R: 64),
]
# the workspace cap doubles the slab length: 10 slabs of 256 rows would need 10 * 27 * 256 * 256 * 4 = 70.8 MB > 64 MiB, so 5 of 512
WGRAD_CAPPED = ("256x256_2305_capped", "same", 256, 256, 2305)
# (32, 32) at R rows with one operand at a base address that is 4- but not 16-byte aligned: scalar loads although cin % 4 == 0
WGRAD_MISALIGNED = ("x", "dy")

SLAB_ROWS, WGRAD_CAP, CHUNK = 256, 64 << 20, 32      # PG_SLAB_ROWS, PG_WGRAD_WORKSPACE_CAP; rows per LDS stage of k_wgrad
COLSUM_ROWS = 1024                                   # PG_COLSUM_ROWS


# !! `wgrad_geometry` restates the launch arithmetic of pg_conv_wgrad (pasco_amd/csrc/grad.hip).  It is used to CHOOSE shapes and to
# !! assert, at import, that the tables above reach every launch class - never to form an expected value: the expected values come
# !! from tests/grad_ref64.py alone.  If the kernel's tiling changes, the assertions below say which class the tables lost.
def wgrad_geometry(K, cin, cout, rows):
    wide = cin > 64 and cout > 64
    bc = 128 if wide else 64
    ci_tiles, co_tiles = -(-cin // bc), -(-cout // bc)
    slab = SLAB_ROWS
    while slab < rows and -(-rows // slab) * K * cin * cout * 4 > WGRAD_CAP:
        slab *= 2
    slabs = max(1, -(-rows // slab))
    half = bc // 2                                   # a wave's share of the tile, per side
    dead = sum(1 for ci0 in range(0, ci_tiles * bc, bc) for co0 in range(0, co_tiles * bc, bc) for wm in (0, 1) for wn in (0, 1)
               if ci0 + wm * half >= cin or co0 + wn * half >= cout)
    return dict(wide=wide, ci_tiles=ci_tiles, co_tiles=co_tiles, slab_rows=slab, slabs=slabs,
                chunks_last=-(-(rows - (slabs - 1) * slab) // CHUNK), dead_waves=dead, waves=4 * ci_tiles * co_tiles,
                scalar_x=cin % 4 != 0, scalar_y=cout % 4 != 0, partial_ci=cin % bc != 0, partial_co=cout % bc != 0)


def _check_wgrad_table():
    natural = None
    ge = {}
    for name, kind, cin, cout, rows_of in WGRAD_CASES + [WGRAD_CAPPED[:4] + (lambda R: WGRAD_CAPPED[4],)]:
        if rows_of is None and kind == "same":
            natural = box_coords(0).shape[0] if natural is None else natural      # a stride-1 map has one output row per input row
        rows = rows_of(SLAB_ROWS) if rows_of is not None else natural if kind == "same" else 100
        ge[name] = wgrad_geometry(27 if kind == "same" else 8, cin, cout, rows)
    v = list(ge.values())
    assert any(not x["wide"] and x["ci_tiles"] == 2 for x in v), "narrow, two input-channel tiles"
    assert any(not x["wide"] and x["ci_tiles"] >= 2 and x["partial_ci"] for x in v), "narrow, a partial second input-channel tile"
    assert any(not x["wide"] and x["co_tiles"] == 4 for x in v), "narrow, four output-channel tiles"
    assert any(x["wide"] and (x["ci_tiles"], x["co_tiles"]) == (2, 2) and x["dead_waves"] == 0 for x in v), "wide, 2 x 2 full tiles"
    assert any(x["wide"] and (x["ci_tiles"], x["co_tiles"]) == (2, 2) and x["scalar_x"] and x["scalar_y"] and x["dead_waves"] > 0
               for x in v), "wide, 2 x 2 tiles, the second ones nearly empty, both operands by scalar loads"
    assert any(x["wide"] and (x["ci_tiles"], x["co_tiles"]) == (1, 1) and x["partial_ci"] and x["partial_co"] for x in v), \
        "wide, one partial tile"
    assert any(x["slabs"] == 1 and x["chunks_last"] == 1 for x in v), "one chunk"
    assert sum(1 for x in v if x["slabs"] == 1 and x["chunks_last"] == 2) >= 2, "exactly two chunks (a partial and a full second one)"
    assert any(x["slabs"] > 1 and x["chunks_last"] == 1 for x in v), "a last slab of one chunk"
    assert any(x["slabs"] > 1 and x["slab_rows"] == SLAB_ROWS for x in v), "several slabs of the base length"
    assert any(x["dead_waves"] == 3 and x["waves"] == 4 for x in v) and any(x["dead_waves"] == 0 for x in v), "dead and no dead waves"
    c = ge[WGRAD_CAPPED[0]]
    assert (c["slab_rows"], c["slabs"]) == (2 * SLAB_ROWS, 5) and -(-WGRAD_CAPPED[4] // SLAB_ROWS) * 27 * 256 * 256 * 4 > WGRAD_CAP, \
        "the cap doubles the slab length"
    g = wgrad_geometry(27, 32, 32, SLAB_ROWS)
    assert not g["scalar_x"] and not g["scalar_y"], "the misaligned cases: channel counts that are multiples of 4"


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


_check_wgrad_table()


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


def misaligned(t: torch.Tensor) -> torch.Tensor:
    """The same values at a base address 4 bytes past a 16-byte boundary (a contiguous view one element into a flat buffer)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert flat.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def table_out_of_range(nbr: torch.Tensor, n_in: int, seed: int = 4) -> torch.Tensor:
    """A copy of the table with ~3 % of its entries rewritten to values >= n_in (n_in itself, n_in + 5, 2^31 - 1) and ~3 % to -7:
    include/pasco_grad.h sums over the o with 0 <= nbr[k][o] < n_in, so all of them are absent."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(nbr.shape, generator=g).to(nbr.device)
    out = nbr.clone()
    out[u < 0.01] = n_in
    out[(u >= 0.01) & (u < 0.02)] = n_in + 5
    out[(u >= 0.02) & (u < 0.03)] = 2 ** 31 - 1
    out[(u >= 0.03) & (u < 0.06)] = -7
    return out


# the input gradient through ConvFunction: (forward cin, cout, kind) - the backward runs the forward kernel at cout -> cin
DGRAD_CASES = [(3, 32, "same"), (20, 7, "same"), (256, 256, "same"), (128, 64, "down"), (64, 128, "gen")]


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
