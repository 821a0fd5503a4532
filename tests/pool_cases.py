"""Test helper: the cases of the pooling / broadcast / channel-wise tests (tests/test_pool_cpu.py on the host restatement and the
CPU oracle, tests/test_hip_pool.py on the pp_* kernels), the checks the two files share and the launch arithmetic of
pasco_amd/csrc/pool.hip restated.  `ops` is whatever serves `seg_reduce / seg_max_bwd / broadcast / broadcast_mul_bwd / pool /
pool_bwd / chconv_fwd / chconv_wgrad`: `pasco_amd.grad.pool_ops(cpu tensor)` or the `PoolLib` binding.

Bounds (a priori, include/pasco_pool.h's orders): an output element that is the sum of T addends a_j, added one after the other in
fp32, is off its fp64 value by at most (T - 1) u sum |a_j| to first order, u = 2^-24; the tests allow (T + 2) u sum |a_j|, plus one
u for every further rounding of an addend (the product of the channel-wise convolution and of the broadcast product's gradient,
the division of an average, and two for the average's backward: 1 / cnt and the product with it).  Copies and selections are
compared bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import pasco_amd.me as ME
from pasco_amd.grad import host
from pasco_amd.me.core import CoordinateManager
from tests import pool_ref64 as ref
from tests.grad_cases import misaligned, table_with_rows

SEG_ROWS, MAX_BATCH, MAX_KVOL = 256, 64, 64          # PP_SEG_ROWS, PP_MAX_BATCH, PP_MAX_KVOL
R = SEG_ROWS
CHANNELS = (1, 3, 32, 33, 65, 256)
SEG_CHANNELS = CHANNELS + (260,)                     # 260: the wide kernel with a second, nearly empty column block
ROWS = (0, 1, R - 1, R, R + 1, 2 * R + 3)
BATCH_KINDS = ("one", "gap", "shuffled8", "max")
BOX = (12, 12, 6)
SUM, AVG, MAX = host.POOL_SUM, host.POOL_AVG, host.POOL_MAX
ADD, MUL, CAT, COPY = host.POOL_BC_ADD, host.POOL_BC_MUL, host.POOL_BC_CAT, host.POOL_BC_COPY


# !! `seg_geometry` / `row_geometry` restate the launch arithmetic of pasco_amd/csrc/pool.hip.  They are used to CHOOSE shapes and
# !! to assert, at import, that the tables reach every launch class - never to form an expected value.
def seg_geometry(n, c, aligned=True, ld=None):
    """pp_seg_reduce (sum / avg), pp_broadcast_mul_bwd, pp_chconv_wgrad: one wave per (partial, column block)."""
    ld = c if ld is None else ld
    wide = c > 64 and c % 4 == 0 and ld % 4 == 0 and aligned
    per_block = 64 * (4 if wide else 1)
    blocks = -(-c // per_block)
    return dict(wide=wide, partials=-(-n // R), tail=n % R, col_blocks=blocks, idle_lanes=blocks * per_block > c)


def row_geometry(c, aligned=True):
    """The row kernels: V = 4 channels per thread where every row starts on a 16-byte boundary, else 1."""
    return dict(wide=c % 4 == 0 and aligned)


def _check_tables():
    seg = [seg_geometry(n, c) for n in ROWS for c in SEG_CHANNELS] + [seg_geometry(R, 33, aligned=False), seg_geometry(R, 256, aligned=False),
                                                                      seg_geometry(R + 1, 96, ld=96 + 33)]
    assert {g["partials"] for g in seg} >= {0, 1, 2, 3}, "no row, one partial, a second one, three"
    assert any(g["partials"] == 1 and g["tail"] == 0 for g in seg) and any(g["partials"] == 2 and g["tail"] == 1 for g in seg)
    assert any(g["partials"] == 1 and g["tail"] == R - 1 for g in seg), "a partial one row short"
    assert any(g["wide"] and g["col_blocks"] == 1 and not g["idle_lanes"] for g in seg), "wide, one full column block"
    assert any(g["wide"] and g["col_blocks"] == 2 and g["idle_lanes"] for g in seg), "wide, a second column block with idle lanes"
    assert any(not g["wide"] and g["col_blocks"] == 2 for g in seg) and any(not g["wide"] and g["col_blocks"] == 1 and g["idle_lanes"] for g in seg)
    assert sum(1 for g in seg if not g["wide"] and g["col_blocks"] > 1) >= 2, "scalar because narrow / odd / misaligned / odd stride"
    row = [row_geometry(c) for c in CHANNELS] + [row_geometry(33, False), row_geometry(32, False)]
    assert any(g["wide"] for g in row) and any(not g["wide"] for g in row)


_check_tables()


def values(shape, seed, device, dtype=torch.float32):
    """Normal values with one row of large ones (1e4) and one column of tiny ones (1e-6), as tests/grad_cases.operands."""
    t = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if t.dim() == 2 and t.shape[0]:
        t[t.shape[0] // 2] *= 1e4
        t[:, t.shape[1] // 2] *= 1e-6
    return t.to(dtype).to(device)


def batch_coords(kind, n, device, seed=0):
    """-> (coords int32 [n, 4], B): the batch column by `kind`; the rows of one batch index are NOT contiguous."""
    g = torch.Generator().manual_seed(seed + n)
    if kind == "one":
        b, B = torch.zeros(n, dtype=torch.int64), 1
    elif kind == "gap":                       # B = 3, batch index 1 has no row
        b, B = torch.randint(0, 2, (n,), generator=g) * 2, 3
    elif kind == "shuffled8":
        b, B = torch.randint(0, 8, (n,), generator=g), 8
    else:
        b, B = torch.randint(0, MAX_BATCH, (n,), generator=g), MAX_BATCH
    if n:
        b[-1] = B - 1                         # the largest batch index is there
    c = torch.randint(-50, 50, (n, 4), generator=g)
    c[:, 0] = b
    return c.to(torch.int32).to(device), B


def _place(t, misalign):
    return misaligned(t) if misalign and t.is_cuda else t


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _assert_within(got, want, mag, T, extra, what):
    ok, worst = ref.within(got, want, mag, T, extra)
    assert ok, f"{what}: the error is {worst:.2f} x the bound"


# ---- per-batch reductions ----------------------------------------------------------------------------------------------------
def check_seg(ops, device, n, c, kind, misalign=False):
    x = _place(values((n, c), 3 * n + c, device), misalign)
    coords, B = batch_coords(kind, n, device)
    want, mag, T, count = ref.seg_sum_ref(x, coords, B)
    for mode in (SUM, AVG):
        out, cnt, arg = ops.seg_reduce(x, coords, B, mode)
        assert arg is None and out.shape == (B, c) and torch.equal(cnt.double(), count), (n, c, kind)
        d = count.clamp(min=1)[:, None] if mode == AVG else 1.0
        _assert_within(out, want / d, mag / d, T, int(mode == AVG), f"seg_reduce mode {mode} n={n} c={c} {kind}")
        assert bool((out[count == 0] == 0).all())
        assert _bits(out, ops.seg_reduce(x, coords, B, mode)[0])
    out, cnt, arg = ops.seg_reduce(x, coords, B, MAX)
    m, a = ref.seg_max_loop(x, coords, B)
    assert torch.equal(arg, a) and _bits(out, m) and torch.equal(cnt.double(), count), (n, c, kind)
    if n:
        assert torch.equal(out[count > 0], torch.stack([x[coords[:, 0] == b].amax(dim=0) for b in range(B) if count[b] > 0]))
    dy = values((B, c), 5, device)
    dx = ops.seg_max_bwd(dy, arg, n)
    want_dx = torch.zeros((n, c), dtype=dy.dtype, device=device)
    ok = arg >= 0
    want_dx[arg.long()[ok], torch.arange(c, device=device)[None, :].expand(B, c)[ok]] = dy[ok]
    assert _bits(dx, want_dx)


def check_seg_slice(ops, device):
    """The reduction of a column slice of a wider matrix (the backward of the concatenation): row stride 129, an odd multiple."""
    n, c, off = R + 1, 96, 33
    full = values((n, off + c), 9, device)
    coords, B = batch_coords("gap", n, device)
    want, mag, T, _ = ref.seg_sum_ref(full[:, off:], coords, B)
    out = ops.seg_reduce(full[:, off:], coords, B, SUM)[0]
    _assert_within(out, want, mag, T, 0, "seg_reduce on a slice")
    assert _bits(out, ops.seg_reduce(full[:, off:].contiguous(), coords, B, SUM)[0])


def check_seg_max_edges(ops, device):
    """Ties (the first row in row order wins), +0 against -0, a NaN column, an empty segment."""
    n, c = R + 7, 5
    x = torch.randint(-2, 3, (n, c), generator=torch.Generator().manual_seed(1)).float()
    coords, B = batch_coords("gap", n, "cpu")
    x[:, 1] = 0.0
    x[0::2, 1] = -0.0                                     # -0 first in every segment
    x[3, 2] = float("nan")
    x[:, 3] = 7.0                                         # all equal: the first row of each segment
    x, coords = x.to(device), coords.to(device)
    out, cnt, arg = ops.seg_reduce(x, coords, B, MAX)
    m, a = ref.seg_max_loop(x, coords, B)
    assert torch.equal(arg, a) and _bits(torch.nan_to_num(out, nan=123.0), torch.nan_to_num(m, nan=123.0))
    b3 = int(coords[3, 0])
    assert bool(torch.isnan(out[b3, 2])) and int(arg[b3, 2]) == -1
    assert bool((arg[1] == -1).all()) and bool((out[1] == 0).all()) and float(cnt[1]) == 0
    for b in (0, 2):
        first = int(torch.nonzero(coords[:, 0] == b)[0])
        assert int(arg[b, 3]) == first and int(arg[b, 1]) == first
        assert bool(torch.signbit(out[b, 1])) == bool(torch.signbit(x[first, 1]))
    dy = values((B, c), 2, device) + 3.0
    dx = ops.seg_max_bwd(dy, arg, n)
    assert bool((dx[:, 2][coords[:, 0] == b3] == 0).all()), "a NaN maximum passes no gradient"
    assert int((dx != 0).sum()) == int((arg >= 0).sum())


# ---- broadcast ---------------------------------------------------------------------------------------------------------------
def check_broadcast(ops, device, n, c, kind, misalign=False, cg=None):
    cg = c if cg is None else cg
    coords, B = batch_coords(kind, n, device)
    x = _place(values((n, c), n + c, device), misalign)
    g = _place(values((B, c), 7, device), misalign)
    gc = _place(values((B, cg), 8, device), misalign)
    b = coords[:, 0].long()
    assert _bits(ops.broadcast(x, g, coords, ADD), x + g[b])
    assert _bits(ops.broadcast(x, g, coords, MUL), x * g[b])
    assert _bits(ops.broadcast(x, gc, coords, CAT), torch.cat([x, gc[b]], dim=1))
    assert _bits(ops.broadcast(None, gc, coords, COPY), gc[b].reshape(n, cg))
    cnt = torch.arange(1, B + 1, device=device, dtype=torch.float32) * 3
    assert _bits(ops.broadcast(None, gc, coords, COPY, cnt), (gc / cnt[:, None])[b].reshape(n, cg))
    dy = _place(values((n, c), n + 11, device), misalign)
    dx, dg = ops.broadcast_mul_bwd(dy, x, g, coords)
    assert _bits(dx, dy * g[b])
    want, mag, T, _ = ref.seg_sum_ref(dy, coords, B, x)
    _assert_within(dg, want, mag, T, 1, f"broadcast_mul_bwd n={n} c={c} {kind}")
    again = ops.broadcast_mul_bwd(dy, x, g, coords)
    assert _bits(dx, again[0]) and _bits(dg, again[1])
    only_x, none = ops.broadcast_mul_bwd(dy, x, g, coords, True, False)
    assert none is None and _bits(only_x, dx)
    none, only_g = ops.broadcast_mul_bwd(dy, x, g, coords, False, True)
    assert none is None and _bits(only_g, dg)


def check_broadcast_batch_outside(ops, device):
    """Through the entry only: a batch index >= B or < 0 gives a zero row (and no term of dg)."""
    n, c, B = 70, 8, 3
    coords, _ = batch_coords("gap", n, device)
    coords[5, 0], coords[64, 0] = 3, -1
    x, g, dy = values((n, c), 1, device) + 5, values((B, c), 2, device) + 5, values((n, c), 3, device)
    inside = ((coords[:, 0] >= 0) & (coords[:, 0] < B))[:, None]
    b = coords[:, 0].long().clamp(0, B - 1)
    for mode, want in ((ADD, x + g[b]), (MUL, x * g[b]), (CAT, torch.cat([x, g[b]], 1)), (COPY, g[b])):
        got = ops.broadcast(None if mode == COPY else x, g, coords, mode)
        assert _bits(got, torch.where(inside, want, torch.zeros_like(want))) and bool((got[5] == 0).all()) and bool((got[64] == 0).all())
    dx, dg = ops.broadcast_mul_bwd(dy, x, g, coords)
    assert _bits(dx, torch.where(inside, dy * g[b], torch.zeros_like(dy)))
    keep = inside[:, 0]
    want, mag, T, _ = ref.seg_sum_ref(dy[keep], coords[keep], B, x[keep])
    _assert_within(dg, want, mag, T, 1, "broadcast_mul_bwd with rows outside")
    out, cnt, _ = ops.seg_reduce(x, coords, B, SUM)
    want, mag, T, count = ref.seg_sum_ref(x[keep], coords[keep], B)
    _assert_within(out, want, mag, T, 0, "seg_reduce with rows outside")
    assert torch.equal(cnt.double(), count)


# ---- tables ------------------------------------------------------------------------------------------------------------------
def pool_coords(seed=0):
    """~30 % of a 12 x 12 x 6 box, two batch elements, in a shuffled row order."""
    rng = np.random.default_rng(100 + seed)
    c = np.argwhere(rng.random((2,) + BOX) < 0.3).astype(np.int32)
    return torch.from_numpy(c[rng.permutation(len(c))].copy())


_MAPS = {}


def pool_map(kind, device, seed=0):
    """-> dict(mgr, in_key, out_key, nbr, n_in, n_out, ks, stride): "down" = kernel 2 / stride 2 (K = 8), "same" = 3^3 (K = 27)."""
    key = (kind, str(device), seed)
    if key not in _MAPS:
        mgr = CoordinateManager(D=3, device=device)
        k0, _ = mgr.insert_and_map(pool_coords(seed).to(device), 1)
        ks, stride = (2, 2) if kind == "down" else (3, 1)
        out_key = mgr.stride(k0, stride)
        nbr = mgr.kernel_map(k0, out_key, ks)
        _MAPS[key] = dict(mgr=mgr, in_key=k0, out_key=out_key, nbr=nbr, n_in=mgr.size(k0), n_out=mgr.size(out_key), ks=ks, stride=stride)
    return _MAPS[key]


TABLE_VARIANTS = ("plain", "offset_absent", "out_of_range", "empty_row")


def table_variant(nbr, n_in, variant):
    t = nbr.clone()
    if variant == "offset_absent":
        t[t.shape[0] // 2] = -1                            # one offset absent everywhere
    elif variant == "out_of_range":
        u = torch.rand(t.shape, generator=torch.Generator().manual_seed(4)).to(t.device)
        t[u < 0.03] = n_in
        t[(u >= 0.03) & (u < 0.05)] = 2 ** 31 - 1
        t[(u >= 0.05) & (u < 0.09)] = -7
    elif variant == "empty_row":
        t[:, 3] = -1                                       # an output row with no present neighbour
    return t


def check_pool(ops, device, kind, c, variant="plain", misalign=False):
    from pasco_amd.grad import nbr_invert
    m = pool_map(kind, device)
    n_in, n_out = m["n_in"], m["n_out"]
    nbr = table_variant(m["nbr"], n_in, variant)
    x = _place(values((n_in, c), c + 1, device), misalign)
    dy = _place(values((n_out, c), c + 2, device), misalign)
    clean = torch.where(ref.present(nbr, n_in), nbr, torch.full_like(nbr, -1))
    inv = nbr_invert(clean, n_in)
    for mode in (SUM, AVG):
        out, cnt = ops.pool(x, nbr, mode)
        want, mag, T, count = ref.pool_ref(x, nbr, mode == AVG)
        assert torch.equal(cnt.double(), count)
        _assert_within(out, want, mag, T, int(mode == AVG), f"pool mode {mode} {kind} c={c} {variant}")
        assert _bits(out, ops.pool(x, nbr, mode)[0])
        dx = ops.pool_bwd(dy, cnt, inv, n_in, mode)
        want, mag, T = ref.pool_bwd_ref(dy, nbr, n_in, mode == AVG)
        _assert_within(dx, want, mag, T, 2 * int(mode == AVG), f"pool_bwd mode {mode} {kind} c={c} {variant}")
        assert _bits(dx, ops.pool_bwd(dy, cnt, inv, n_in, mode))
        if variant == "empty_row":
            assert float(cnt[3]) == 0 and bool((out[3] == 0).all())
    if kind == "down" and variant == "plain":               # kernel == stride: one term per input row, the sum's backward is a copy
        assert int((inv >= 0).sum(dim=0).max()) == 1
        parent = inv.max(dim=0).values.long()
        assert _bits(ops.pool_bwd(dy, None, inv, n_in, SUM), dy[parent])


def check_chconv(ops, device, kind, c, variant="plain", bias=True, misalign=False):
    from pasco_amd.grad import nbr_invert
    m = pool_map(kind, device)
    n_in, n_out, K = m["n_in"], m["n_out"], m["nbr"].shape[0]
    nbr = table_variant(m["nbr"], n_in, variant)
    x = _place(values((n_in, c), c + 3, device), misalign)
    w = _place(values((K, c), c + 4, device), misalign)
    bb = _place(values((1, c), c + 5, device).reshape(-1), misalign) if bias else None
    out = ops.chconv_fwd(x, nbr, w, bb)
    want, mag, T = ref.chconv_ref(x, nbr, w, bb)
    _assert_within(out, want, mag, T, 1, f"chconv_fwd {kind} c={c} {variant}")
    assert _bits(out, ops.chconv_fwd(x, nbr, w, bb))
    if variant == "empty_row":
        assert _bits(out[3], bb if bias else torch.zeros(c, device=device))
    dy = _place(values((n_out, c), c + 6, device), misalign)
    dw = ops.chconv_wgrad(x, dy, nbr)
    want, mag, T = ref.chconv_wgrad_ref(x, dy, nbr)
    _assert_within(dw, want, mag, T, 1, f"chconv_wgrad {kind} c={c} {variant}")
    assert _bits(dw, ops.chconv_wgrad(x, dy, nbr))
    # the input gradient: the same entry over the inverse table with the same weights, against the adjoint by scatter
    clean = torch.where(ref.present(nbr, n_in), nbr, torch.full_like(nbr, -1))
    inv = nbr_invert(clean, n_in)
    dx = ops.chconv_fwd(dy, inv, w, None)
    want = torch.zeros((n_in, c), dtype=torch.float64, device=device)
    mag = torch.zeros_like(want)
    for k in range(K):
        o = torch.nonzero(clean[k] >= 0).reshape(-1)
        t = dy.double()[o] * w.double()[k]
        want.index_put_((clean[k, o].long(),), t, accumulate=True)
        mag.index_put_((clean[k, o].long(),), t.abs(), accumulate=True)
    _assert_within(dx, want, mag, (inv >= 0).double().sum(dim=0)[:, None], 1, f"chconv input gradient {kind} c={c} {variant}")


def check_chconv_wgrad_rows(ops, device, rows, c):
    """pp_chconv_wgrad at a given number of output rows (the partials of PP_SEG_ROWS rows and their tail)."""
    nbr, n_in = table_with_rows("same", rows, device)
    x, dy = values((n_in, c), rows + 1, device), values((rows, c), rows + 2, device)
    dw = ops.chconv_wgrad(x, dy, nbr)
    want, mag, T = ref.chconv_wgrad_ref(x, dy, nbr)
    assert dw.shape == (27, c)
    _assert_within(dw, want, mag, T, 1, f"chconv_wgrad rows={rows} c={c}")
    if rows == 0:
        assert bool((dw == 0).all())


# ---- against the dense torch operators ----------------------------------------------------------------------------------------
def _sparse(feats, m):
    return ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])


def check_dense_twins(device, dtype):
    """The modules against avg_pool3d / conv3d(groups=C) / masked means on the zero-filled grid: exact agreement is not promised
    (the dense operators add in another order), so fp64 on the CPU compares at 1e-12 of the magnitude and fp32 on the device at the
    a-priori bound with T = the kernel volume (+ the bias)."""
    dims = (2,) + BOX
    c = 6
    for kind in ("down", "same"):
        m = pool_map(kind, device)
        coords, out_coords = m["mgr"].get_coordinates(m["in_key"]), m["mgr"].get_coordinates(m["out_key"])
        feats = values((m["n_in"], c), 21, device, dtype)
        K = m["nbr"].shape[0]
        f64, mag = feats.double(), ref.dense_pool(feats.double().abs(), coords, out_coords, dims, m["ks"], m["stride"], False)

        def close(got, want, mag, extra, what):
            if dtype == torch.float64:
                assert bool(((got - want).abs() <= 1e-12 * mag + 1e-300).all()), what
            else:
                _assert_within(got, want, mag, K, extra, what)

        x = _sparse(feats, m)
        with torch.no_grad():
            s = ME.MinkowskiSumPooling(m["ks"], m["stride"], dimension=3)(x)
            a = ME.MinkowskiAvgPooling(m["ks"], m["stride"], dimension=3)(x)
            conv = ME.MinkowskiChannelwiseConvolution(c, m["ks"], m["stride"], bias=True, dimension=3).to(device=device, dtype=dtype)
            y = conv(x)
        assert s.coordinate_map_key == m["out_key"] and torch.equal(s.C, out_coords)
        close(s.F, ref.dense_pool(f64, coords, out_coords, dims, m["ks"], m["stride"], False), mag, 0, f"sum pooling {kind}")
        cnt = ref.dense_pool(torch.ones_like(f64[:, :1]), coords, out_coords, dims, m["ks"], m["stride"], False)
        close(a.F, ref.dense_pool(f64, coords, out_coords, dims, m["ks"], m["stride"], True), mag / cnt, 1, f"avg pooling {kind}")
        kd, bd = conv.kernel.detach().double(), conv.bias.detach().double()
        wmag = ref.dense_chconv(f64.abs(), coords, out_coords, dims, kd.abs(), bd.abs(), m["ks"], m["stride"])
        close(y.F, ref.dense_chconv(f64, coords, out_coords, dims, kd, bd, m["ks"], m["stride"]), wmag, 2, f"channel-wise convolution {kind}")
    with torch.no_grad():
        g = ME.MinkowskiGlobalAvgPooling()(x)
    want = ref.dense_global_avg(f64, coords, dims)
    n_b = torch.bincount(coords[:, 0].long(), minlength=2).double()[:, None]
    gmag = ref.dense_global_avg(f64.abs(), coords, dims)
    if dtype == torch.float64:
        assert bool(((g.F - want).abs() <= 1e-12 * gmag).all())
    else:
        _assert_within(g.F, want, gmag, n_b, 1, "global average")
    assert g.C.tolist() == [[0, 0, 0, 0], [1, 0, 0, 0]] and g.tensor_stride == [0, 0, 0]


# ---- the modules -------------------------------------------------------------------------------------------------------------
def module_cases(device, c=6):
    """(name, build(), run(module, feats) -> features of the result, parameters?) over the "same" and "down" maps."""
    m3, m2 = pool_map("same", device), pool_map("down", device)

    def glob(m, feats):
        return ME.MinkowskiGlobalAvgPooling()(_sparse(feats * 0.5 + 0.25, m))

    def bc(cls):
        return lambda mod, feats: cls()(_sparse(feats, m3), glob(m3, feats)).F

    def on(m):
        return lambda mod, feats: mod(_sparse(feats, m)).F

    def up(mod, feats):
        low = ME.MinkowskiSumPooling(2, 2, dimension=3)(_sparse(feats, m2))
        return mod(low).F

    return [
        ("global_sum", ME.MinkowskiGlobalSumPooling, on(m3)), ("global_avg", ME.MinkowskiGlobalPooling, on(m3)),
        ("global_max", ME.MinkowskiGlobalMaxPooling, on(m3)),
        ("bc_copy", ME.MinkowskiBroadcast, bc(ME.MinkowskiBroadcast)), ("bc_add", ME.MinkowskiBroadcastAddition, bc(ME.MinkowskiBroadcastAddition)),
        ("bc_mul", ME.MinkowskiBroadcastMultiplication, bc(ME.MinkowskiBroadcastMultiplication)),
        ("bc_cat", ME.MinkowskiBroadcastConcatenation, bc(ME.MinkowskiBroadcastConcatenation)),
        ("sum_down", lambda: ME.MinkowskiSumPooling(2, 2, dimension=3), on(m2)), ("avg_down", lambda: ME.MinkowskiAvgPooling(2, 2, dimension=3), on(m2)),
        ("sum_same", lambda: ME.MinkowskiSumPooling(3, 1, dimension=3), on(m3)), ("avg_same", lambda: ME.MinkowskiAvgPooling(3, 1, dimension=3), on(m3)),
        ("transpose", lambda: ME.MinkowskiPoolingTranspose(2, 2, expand_coordinates=True, dimension=3), up),
        ("chconv_same", lambda: ME.MinkowskiChannelwiseConvolution(c, 3, bias=True, dimension=3), on(m3)),
        ("chconv_down", lambda: ME.MinkowskiChannelwiseConvolution(c, 2, 2, bias=False, dimension=3), on(m2)),
    ]


MODULE_NAMES = ["global_sum", "global_avg", "global_max", "bc_copy", "bc_add", "bc_mul", "bc_cat", "sum_down", "avg_down", "sum_same",
                "avg_same", "transpose", "chconv_same", "chconv_down"]


def check_module_modes(device, name, c=6):
    """The forward values are the same bits under no_grad, inference_mode and on the autograd route, which alone has a grad_fn;
    the backward reaches the input and the parameters."""
    _, build, run = next(t for t in module_cases(device, c) if t[0] == name)
    torch.manual_seed(5)
    mod = build().to(device)
    n = pool_map("same", device)["n_in"]
    feats = values((n, c), 31, device)
    with torch.no_grad():
        quiet = run(mod, feats.clone().requires_grad_(True))
    with torch.inference_mode():
        inf = run(mod, feats)
    assert quiet.grad_fn is None and _bits(quiet, inf)
    f = feats.clone().requires_grad_(True)
    out = run(mod, f)
    assert out.grad_fn is not None and _bits(out.detach(), quiet)
    out.backward(values(tuple(out.shape), 32, device))
    assert f.grad is not None and f.grad.shape == f.shape and bool(torch.isfinite(f.grad).all())
    for p in mod.parameters():
        assert p.grad is not None and bool((p.grad != 0).any())
    with pytest.raises(RuntimeError):                        # once differentiable
        f2 = feats.clone().requires_grad_(True)
        o2 = run(mod, f2)
        (g1,) = torch.autograd.grad(o2.sum(), f2, create_graph=True)
        g1.sum().backward()


def check_module_gradients(device, name, c=4):
    """fp64 on the CPU: the module's autograd (pasco_amd.me.autograd over the host restatement) against torch's own autograd
    through the host restatement's differentiable torch operations, for the input and every parameter."""
    _, build, run = next(t for t in module_cases(device, c) if t[0] == name)
    torch.manual_seed(6)
    mod = build().to(device).double()
    n = pool_map("same", device)["n_in"]
    feats = values((n, c), 33, device, torch.float64)
    f = feats.clone().requires_grad_(True)
    out = run(mod, f)
    dy = values(tuple(out.shape), 34, device, torch.float64)
    out.backward(dy)
    got = [f.grad] + [p.grad.clone() for p in mod.parameters()]
    for p in mod.parameters():
        p.grad = None
    f2 = feats.clone().requires_grad_(True)
    if name.startswith("chconv"):                            # the module detaches its parameters off the autograd route
        nbr = pool_map(name.split("_")[1], device)["nbr"]
        out2 = host.pool_chconv_fwd(f2, nbr, mod.kernel, None if mod.bias is None else mod.bias.reshape(-1))
    else:
        with host_autograd():
            out2 = run(mod, f2)
    assert torch.equal(out2.detach(), out.detach())
    out2.backward(dy)
    want = [f2.grad] + [p.grad for p in mod.parameters()]
    for g, w in zip(got, want):
        assert g.shape == w.shape
        scale = float(w.abs().max()) + 1e-300
        assert float((g - w).abs().max()) <= 1e-12 * scale, (name, float((g - w).abs().max()) / scale)


class host_autograd:
    """Inside the block the modules of pasco_amd.me take the route without their autograd Functions although an input requires
    grad (`wants_grad` answers False), so on CPU tensors torch differentiates the host restatement's own operations."""

    def __enter__(self):
        from pasco_amd.me import modules
        self.modules, self.was = modules, modules.wants_grad
        modules.wants_grad = lambda *t: False

    def __exit__(self, *exc):
        self.modules.wants_grad = self.was


def check_prologue(device):
    """A pending BatchNorm -> ReLU prologue on the input is applied before the operator reads the rows."""
    m = pool_map("same", device)
    c = 6
    feats = values((m["n_in"], c), 41, device)
    bn, relu = ME.MinkowskiBatchNorm(c).to(device).eval(), ME.MinkowskiReLU()
    with torch.no_grad():
        bn.bn.running_mean.normal_(), bn.bn.running_var.uniform_(0.5, 2.0), bn.bn.weight.normal_(), bn.bn.bias.normal_()
        for build in (ME.MinkowskiGlobalAvgPooling, lambda: ME.MinkowskiSumPooling(3, 1, dimension=3),
                      lambda: ME.MinkowskiChannelwiseConvolution(c, 3, dimension=3).to(device),
                      lambda: ME.MinkowskiAvgPooling(2, 2, dimension=3)):
            mod = build()
            pend = relu(bn(_sparse(feats, m)))
            assert pend._pending is not None, "the eval-mode BatchNorm -> ReLU is deferred"
            got = mod(pend).F
            plain = torch.relu(F.batch_norm(feats, bn.bn.running_mean, bn.bn.running_var, bn.bn.weight, bn.bn.bias, False, 0.0, bn.bn.eps))
            want = mod(_sparse(pend.F, m)).F
            assert _bits(got, want) and bool(torch.allclose(pend.F, plain, rtol=1e-5, atol=1e-6))


def check_state_dict():
    for ks, bias in ((3, True), (2, False)):
        mod = ME.MinkowskiChannelwiseConvolution(10, ks, stride=1 if ks == 3 else 2, bias=bias, dimension=3)
        sd = mod.state_dict()
        assert list(sd) == (["kernel", "bias"] if bias else ["kernel"])
        assert tuple(sd["kernel"].shape) == (ks ** 3, 10) and (not bias or tuple(sd["bias"].shape) == (1, 10))
        fresh = ME.MinkowskiChannelwiseConvolution(10, ks, stride=1 if ks == 3 else 2, bias=bias, dimension=3)
        fresh.load_state_dict({k: v.clone() + 1 for k, v in sd.items()}, strict=True)
        assert torch.equal(fresh.kernel, mod.kernel + 1)
    for cls in (ME.MinkowskiGlobalPooling, ME.MinkowskiBroadcastMultiplication, ME.MinkowskiBroadcastAddition):
        assert len(cls().state_dict()) == 0


def check_refusals(device):
    with pytest.raises(ValueError, match="PP_MAX_KVOL"):
        ME.MinkowskiAvgPooling(5, 1, dimension=3)                              # 125 offsets
    with pytest.raises(ValueError, match="PP_MAX_KVOL"):
        ME.MinkowskiChannelwiseConvolution(4, 7, dimension=3)
    with pytest.raises(ValueError, match="kernel == stride"):
        ME.MinkowskiSumPooling(3, 2, dimension=3)
    with pytest.raises(ValueError, match="must be odd"):
        ME.MinkowskiChannelwiseConvolution(4, 2, dimension=3)
    with pytest.raises(ValueError, match="dimension=3"):
        ME.MinkowskiAvgPooling(2, 2, dimension=2)
    with pytest.raises(ValueError, match="kernel generators"):
        ME.MinkowskiSumPooling(2, 2, kernel_generator=object(), dimension=3)
    with pytest.raises(ValueError, match="expand_coordinates=True"):
        ME.MinkowskiPoolingTranspose(2, 2, dimension=3)
    with pytest.raises(ValueError, match="kernel 2 / stride 2"):
        ME.MinkowskiPoolingTranspose(3, 1, expand_coordinates=True, dimension=3)
    m = pool_map("same", device)
    x = _sparse(values((m["n_in"], 4), 1, device), m)
    with pytest.raises(AssertionError, match="explicit output coordinates"):
        ME.MinkowskiGlobalPooling()(x, coordinates=x.C)
    # a global tensor with fewer rows than the input has batch indices; channel counts that do not match
    one = ME.SparseTensor(values((1, 4), 2, device), torch.zeros((1, 4), dtype=torch.int32, device=device))
    with pytest.raises(ValueError, match="batch index 1"):
        ME.MinkowskiBroadcastMultiplication()(x, one)
    g5 = ME.MinkowskiGlobalPooling()(_sparse(values((m["n_in"], 5), 3, device), m))
    with pytest.raises(ValueError, match="4 channels against 5"):
        ME.MinkowskiBroadcastAddition()(x, g5)
    with pytest.raises(ValueError, match="the kernel has 8"):
        ME.MinkowskiChannelwiseConvolution(8, 3, dimension=3).to(device)(x)
    # more batch indices than PP_MAX_BATCH
    n = MAX_BATCH + 1
    coords = torch.zeros((n, 4), dtype=torch.int32)
    coords[:, 0] = torch.arange(n)
    many = ME.SparseTensor(values((n, 4), 4, device), coords.to(device))
    with pytest.raises(ValueError, match="PP_MAX_BATCH"):
        ME.MinkowskiGlobalAvgPooling()(many)
    if device.type == "cuda":
        with pytest.raises(TypeError, match="fp32"):
            ME.MinkowskiGlobalAvgPooling()(_sparse(values((m["n_in"], 4), 1, device).double(), m))
        with pytest.raises(TypeError, match="fp32"):
            ME.MinkowskiSumPooling(3, 1, dimension=3)(_sparse(values((m["n_in"], 4), 1, device).half(), m))


# ---- the stack -----------------------------------------------------------------------------------------------------------------
STACK_C = 8


class PoolStack(nn.Module):
    """A squeeze-and-excitation block (global avg -> linear -> ReLU -> linear -> sigmoid -> broadcast multiplication), then a
    depthwise-separable block (channel-wise 3^3 -> k = 1 convolution -> sum and avg pooling down, added -> pooling transpose up
    -> broadcast addition and concatenation of the result's global average)."""

    def __init__(self, c=STACK_C):
        super().__init__()
        self.gap = ME.MinkowskiGlobalAvgPooling()
        self.fc1, self.fc2 = ME.MinkowskiLinear(c, c // 2), ME.MinkowskiLinear(c // 2, c)
        self.relu, self.sigmoid = ME.MinkowskiReLU(), ME.MinkowskiSigmoid()
        self.mul = ME.MinkowskiBroadcastMultiplication()
        self.dw = ME.MinkowskiChannelwiseConvolution(c, kernel_size=3, bias=True, dimension=3)
        self.pw = ME.MinkowskiConvolution(c, 2 * c, kernel_size=1, bias=True, dimension=3)
        self.down_sum = ME.MinkowskiSumPooling(2, 2, dimension=3)
        self.down_avg = ME.MinkowskiAvgPooling(2, 2, dimension=3)
        self.up = ME.MinkowskiPoolingTranspose(2, 2, expand_coordinates=True, dimension=3)
        self.add, self.cat = ME.MinkowskiBroadcastAddition(), ME.MinkowskiBroadcastConcatenation()

    def forward(self, x):
        s = self.mul(x, self.sigmoid(self.fc2(self.relu(self.fc1(self.gap(x))))))
        y = self.pw(self.dw(s))
        u = self.up(self.down_sum(y) + self.down_avg(y))
        g = self.gap(u)
        return self.cat(self.add(u, g), g)


def pool_stack_gradients(device):
    """-> {name: (g, g32, g64)} for every parameter of `PoolStack` and the input features ("x")."""
    torch.manual_seed(3)
    net = PoolStack().to(device).train()
    coords = pool_coords(5).to(device)
    gen = torch.Generator().manual_seed(11)
    # a mean of 1 per channel: the squeeze's hidden units are not all on the dead side of the ReLU
    feats = (torch.randn(coords.shape[0], STACK_C, generator=gen) + 1.0).to(device).requires_grad_(True)
    out = net(ME.SparseTensor(feats, coords))
    assert out.F.grad_fn is not None and out.F.shape[1] == 4 * STACK_C
    dims = (2,) + BOX
    tgt = torch.randn((2, 4 * STACK_C) + BOX, generator=gen).to(device)
    (out.F - ref.at_sites(tgt, out.C)).square().mean().backward()
    params = dict(net.named_parameters())
    g32 = ref.pool_stack_twin(params, feats, coords, tgt, dims, torch.float32)
    g64 = ref.pool_stack_twin(params, feats, coords, tgt, dims, torch.float64)
    got = {k: v.grad for k, v in params.items()}
    got["x"] = feats.grad
    return {k: (got[k], g32[k], g64[k]) for k in g64}


def pool_stack_ratios(device):
    """name -> max |g - g64| / max |g32 - g64|."""
    out = {}
    for k, (g, g32, g64) in pool_stack_gradients(device).items():
        assert g is not None, f"{k} has no gradient"
        assert g.shape == g64.shape, (k, g.shape, g64.shape)
        assert float((g.double() - g64).abs().max()) <= 1e-3 * float(g64.abs().max()), f"{k}: not the twin's gradient"
        out[k] = float((g.double() - g64).abs().max()) / float((g32.double() - g64).abs().max())
    return out
