"""Test helper: the cases of the point <-> voxel tests (tests/test_field_cpu.py on the host restatement and the CPU checker,
tests/test_hip_field.py on the pq_* kernels) and the checks the two files share.  `ops` is whatever serves `group / seg_rows /
seg_max_bwd / gather_w / interp_map / interp_fwd`: `pasco_amd.grad.field_ops(cpu tensor)` or the `FieldLib` binding.

Bounds (a priori, include/pasco_field.h's orders; u = 2^-24): a segment sum of m terms, each product rounded once, then added
one after the other in fp32, is within m u sum |w_j x_j| of its fp64 value; the average adds one rounding for the division:
(m + 1) u sum |w_j x_j| / cnt.  An interpolation weight is within 8 u of its fp64 value, relative (one rounding each for the
division, the subtraction and the 1 - ., for three axes' worth folded into the product, plus two for the product of three); an
interpolated row within 16 u sum_k |w_k x_k| (weights 8 u, one rounding per product, seven per sum).  Copies, selections and
tables are compared exactly."""
import torch
import torch.nn as nn
import torch.nn.functional as F

import pasco_amd.me as ME
from pasco_amd.grad import host
from pasco_amd.me.core import CoordinateManager, SparseTensor
from tests import field_ref64 as ref
from tests.grad_cases import misaligned
from tests.pool_cases import values

SEG_ROWS = 64                                  # PQ_SEG_ROWS
S = SEG_ROWS
U = ref.U
SUM, AVG, MAX = host.FIELD_SUM, host.FIELD_AVG, host.FIELD_MAX
GROUP_N = (0, 1, 63, 64, 65, 4099, 20481)             # 20481: eleven sort tiles, a second trip of the count scan
GROUP_PATTERNS = ("unique", "one", "half_absent", "descending", "mostly_empty", "nseg1")
SEG_LENGTHS = (1, S - 1, S, S + 1, 2 * S + 3, 0)              # the last: an empty segment
SEG_CHANNELS = (1, 4, 33, 256, 260)
Q = ME.SparseTensorQuantizationMode
QUANT_MODES = (Q.UNWEIGHTED_AVERAGE, Q.UNWEIGHTED_SUM, Q.MAX_POOL, Q.RANDOM_SUBSAMPLE)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


def _place(t, misalign):
    return misaligned(t) if misalign and t.is_cuda else t


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- grouping ------------------------------------------------------------------------------------------------------------------
def group_keys(pattern, n, seed=0):
    """-> (keys int32 [n] on the CPU, n_seg)."""
    g = _gen(seed + n)
    if pattern == "unique":
        return torch.randperm(n, generator=g).to(torch.int32), max(n, 1)
    if pattern == "one":
        return torch.full((n,), 1, dtype=torch.int32), 3
    if pattern == "half_absent":                       # every second key absent: -1 and values >= n_seg in turn
        k = torch.randint(0, 5, (n,), generator=g)
        k[1::4], k[3::4] = -1, 5 + 7
        return k.to(torch.int32), 5
    if pattern == "descending":
        return torch.arange(n - 1, -1, -1, dtype=torch.int32), max(n, 1)
    if pattern == "mostly_empty":                      # three digit passes, most segments without a member
        return torch.randint(0, 100000, (n,), generator=g).to(torch.int32), 100000
    assert pattern == "nseg1"
    k = torch.zeros(n, dtype=torch.int64)
    k[2::5] = 1
    return k.to(torch.int32), 1


def check_group(ops, device, pattern, n):
    keys, n_seg = group_keys(pattern, n)
    offsets, perm = ops.group(keys.to(device), n_seg)
    want_off, want_perm = ref.group_ref(keys, n_seg)
    assert offsets.dtype == torch.int32 and perm.dtype == torch.int32 and offsets.shape == (n_seg + 1,) and perm.shape == (n,)
    assert torch.equal(offsets.cpu().long(), want_off), (pattern, n)
    assert torch.equal(perm.cpu().long()[:want_perm.numel()], want_perm), (pattern, n)
    again = ops.group(keys.to(device), n_seg)
    assert torch.equal(again[0], offsets) and torch.equal(again[1][:want_perm.numel()], perm[:want_perm.numel()])


# ---- segment sums --------------------------------------------------------------------------------------------------------------
def seg_case(device, seed=0):
    """Segments of every length of SEG_LENGTHS, their members scattered over the list, and a few absent entries."""
    lens = list(SEG_LENGTHS)
    keys = torch.cat([torch.full((m,), s, dtype=torch.int64) for s, m in enumerate(lens)] + [torch.full((5,), -1, dtype=torch.int64)])
    keys = keys[torch.randperm(keys.numel(), generator=_gen(seed))].to(torch.int32)
    return keys, len(lens), ref.members_of(keys, len(lens))


def _assert_within(got, want, bound, what):
    err = (got.detach().cpu().double() - want).abs()
    ok = bool((err <= bound).all())
    assert ok, f"{what}: the error is {float((err / bound.clamp(min=1e-300)).max()):.2f} x the bound"


def check_seg_sums(ops, device, c, misalign=False):
    keys, n_seg, members = seg_case(device)
    n = keys.numel()
    offsets, perm = ops.group(keys.to(device), n_seg)
    x = _place(values((n, c), 7 + c, device), misalign)
    w = torch.randn(n, generator=_gen(11)).to(device)
    lens = torch.tensor([len(m) for m in members], dtype=torch.float64)
    for weights in (None, w):
        want, mag, cnt = ref.seg_sum_ref(x, members, weights)
        for mode in (SUM, AVG):
            out, count, arg = ops.seg_rows(x, offsets, perm, mode, w=weights)
            assert arg is None and out.shape == (n_seg, c) and torch.equal(count.cpu().double(), cnt)
            d = cnt.clamp(min=1)[:, None] if mode == AVG else 1.0
            bound = (lens[:, None] + (1 if mode == AVG else 0)) * U * mag / d
            _assert_within(out, want / d, bound, f"seg_rows mode {mode} c={c} weights={weights is not None}")
            assert bool((out[-1] == 0).all()) and float(count[-1]) == 0            # the empty segment
            assert _bits(out, ops.seg_rows(x, offsets, perm, mode, w=weights)[0])
    # src_mod: list entry j reads row j % 7 (the shape of the interpolation's backward)
    xs = _place(values((7, c), 3, device), misalign)
    members7 = members
    want, mag, cnt = ref.seg_sum_ref(xs, members7, w, src_mod=7)
    out = ops.seg_rows(xs, offsets, perm, SUM, w=w, src_mod=7)[0]
    _assert_within(out, want, lens[:, None] * U * mag, f"seg_rows src_mod c={c}")


def check_seg_max(ops, device, c=5):
    """Values and arg bit for bit: ties (the first in list order), +0 against -0, a NaN, -inf only, an empty segment."""
    keys, n_seg, members = seg_case(device, seed=3)
    n = keys.numel()
    offsets, perm = ops.group(keys.to(device), n_seg)
    x = values((n, c), 21, device).cpu()
    x = (x * 4).round() / 4                                        # many ties
    first = [m[0] for m in members if m]
    x[first[1], 0] = float("nan")                                  # a NaN in segment 1, channel 0
    x[members[2], 1] = float("-inf")                               # nothing but -inf
    zeros = members[3][:4]
    x[members[3], 2] = -1.0
    x[zeros[0], 2], x[zeros[1], 2], x[zeros[2], 2] = -0.0, 0.0, -0.0   # -0 comes first: its bits are the result
    x = x.to(device)
    out, cnt, arg = ops.seg_rows(x, offsets, perm, MAX)
    m, a = ref.seg_max_loop(x, members)
    assert torch.equal(arg.cpu(), a) and _bits(out.cpu(), m), "max / arg differ from the literal loop"
    assert bool(torch.isnan(out[1, 0])) and int(arg[1, 0]) == -1 and int(arg[-1, 0]) == -1 and float(out[-1, 0]) == 0.0
    assert float(out[2, 1]) == float("-inf") and int(arg[2, 1]) == members[2][0]
    assert int(arg[3, 2]) == zeros[0] and torch.signbit(out[3, 2].cpu())
    assert torch.equal(cnt.cpu().double(), torch.tensor([len(v) for v in members], dtype=torch.float64))
    dy = values((n_seg, c), 5, device)
    dx = ops.seg_max_bwd(dy, arg, n)
    want = torch.zeros((n, c), dtype=dy.dtype)
    ok = a >= 0
    want[a.long()[ok], torch.arange(c)[None, :].expand(n_seg, c)[ok]] = dy.cpu()[ok]
    assert _bits(dx.cpu(), want)
    assert _bits(out, ops.seg_rows(x, offsets, perm, MAX)[0]) and torch.equal(arg, ops.seg_rows(x, offsets, perm, MAX)[2])


def check_gather_w(ops, device, c, misalign=False):
    n_src, n = 37, 2 * S + 3
    x = _place(values((n_src, c), 13 + c, device), misalign)
    d = torch.randint(1, 9, (n_src,), generator=_gen(2)).float()
    d[5], d[6] = 0.0, 3.0
    idx = torch.randint(0, n_src, (n,), generator=_gen(4)).to(torch.int32)
    idx[0], idx[1], idx[2], idx[3] = 5, -1, n_src, 6
    out = ops.gather_w(x, idx.to(device), d.to(device))
    xc = x.cpu()
    ic = idx.long().clamp(0, n_src - 1)
    want = xc[ic] * (1.0 / torch.where(d[ic] == 0, torch.ones_like(d[ic]), d[ic]))[:, None]
    want[(idx < 0) | (idx >= n_src) | (d[ic] == 0)] = 0.0
    assert _bits(out.cpu(), want), f"gather_w c={c}"
    assert bool((out[:3] == 0).all())


# ---- interpolation -------------------------------------------------------------------------------------------------------------
def voxel_map(device, ts, batch, one=False):
    """A 3 x 3 x 3 block of voxels around the origin (negative coordinates included) with one voxel missing, in batch index
    `batch`; or a map of one voxel.  -> (manager, key, coordinates int32 [n, 4] in row order)."""
    if one:
        c = torch.tensor([[batch, 0, 0, 0]], dtype=torch.int32)
    else:
        r = torch.arange(-1, 2) * ts
        g = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3)
        g = g[torch.randperm(27, generator=_gen(ts))]
        g = g[~((g[:, 0] == ts) & (g[:, 1] == ts) & (g[:, 2] == -ts))]              # one corner voxel is not there
        c = torch.cat([torch.full((g.shape[0], 1), batch), g], dim=1).to(torch.int32)
    mgr = CoordinateManager(D=3, device=device)
    key = mgr.insert_unique(c.to(device), ts)
    return mgr, key, c


def interp_points(ts, batch):
    """Points on a corner, an edge, a face, inside; negative coordinates; far away; non-finite."""
    t = float(ts)
    p = [[0, 0, 0], [0, 0, 0.5 * t], [0, 0.25 * t, 0.5 * t], [0.125 * t, 0.25 * t, 0.5 * t],
         [-0.25 * t, 0.5 * t, 0.75 * t], [-1.0 * t, -1.0 * t, -0.25 * t], [-0.25 * t, -0.25 * t, -0.25 * t],
         [0.5 * t, 0.5 * t, 0.5 * t], [0.75 * t, 0.75 * t, -0.5 * t],            # next to the missing voxel (ts, ts, -ts)
         [50 * t, 50 * t, 50 * t], [1.5 * t, 0.5 * t, 0.25 * t],                # every corner absent; half of them absent
         [float("nan"), 0, 0], [0, float("inf"), 0], [0, 0, float("-inf")]]
    rnd = (torch.rand(40, 3, generator=_gen(9 + ts)) * 3 - 1.5) * t
    # one ulp below a voxel boundary: with a stride that is no power of two the fp32 quotient x / ts rounds onto the next integer
    rnd[0] = torch.tensor([float(torch.nextafter(torch.tensor(t), torch.tensor(0.0))), 0.5 * t, 0.5 * t])
    pts = torch.cat([torch.tensor(p, dtype=torch.float32), rnd.float()], dim=0)
    b = torch.full((pts.shape[0], 1), float(batch))
    b[3] = batch + 0.5                                  # floor(b) is the batch index
    b[-1] = batch + 1                                   # a batch index the map does not have
    return torch.cat([b, pts], dim=1)


def check_interp_map(ops, device, ts, batch, one=False, dtype=torch.float32):
    mgr, key, vox = voxel_map(device, ts, batch, one)
    pts = interp_points(ts, batch)
    cmap = mgr._maps[key]
    rows, weights = ops.interp_map(pts.to(device=device, dtype=dtype), cmap.tkeys, cmap.tvals, ts)
    want_rows, w64 = ref.interp_ref(pts, vox, ts)
    assert rows.shape == (8, pts.shape[0]) and torch.equal(rows.cpu(), want_rows), f"interp_map rows ts={ts} batch={batch}"
    err = (weights.cpu().double() - w64).abs()
    assert bool((err <= 8 * U * w64.abs()).all()), f"interp_map weights: {float((err / (8 * U * w64.abs()).clamp(min=1e-300)).max()):.2f} x the bound"
    assert bool((rows[:, 9] == -1).all()) and bool((rows[:, 11:14] == -1).all()) and bool((weights[:, 11:14] == 0).all())
    assert int((rows[:, 0] >= 0).sum()) == 1 and float(weights[:, 0].max()) == 1.0               # on a corner: one voxel, weight 1
    if not one:
        assert int((rows[:, 1] >= 0).sum()) == 2 and int((rows[:, 2] >= 0).sum()) == 4 and int((rows[:, 3] >= 0).sum()) == 8
    return mgr, key, vox, pts, rows, weights, w64


def check_interp_fwd(ops, device, c, ts=2, misalign=False):
    mgr, key, vox, pts, rows, weights, w64 = check_interp_map(ops, device, ts, 0)
    x = _place(values((vox.shape[0], c), 17 + c, device), misalign)
    out = ops.interp_fwd(x, rows, weights)
    want, mag = ref.interp_fwd_ref(x, rows, w64)
    _assert_within(out, want, 16 * U * mag, f"interp_fwd c={c}")
    assert bool((out[9] == 0).all()) and bool((out[11:14] == 0).all())
    assert _bits(out, ops.interp_fwd(x, rows, weights))
    # an Inf feature on a corner of the point's own cell that it does not touch (weight exactly 0): the result stays finite.
    # Point 0 sits on a corner of its cell (seven such corners), point 1 on an edge (six), point 2 on a face (four).
    table = {tuple(v): r for r, v in enumerate(vox.tolist())}
    for p_i, zero_corners in ((0, 7), (1, 6), (2, 4)):
        xyz = [float(v) for v in pts[p_i, 1:]]
        lower = [int(v // ts) * ts for v in xyz]
        hit = []
        for k in range(8):
            corner = (0, lower[0] + ((k >> 2) & 1) * ts, lower[1] + ((k >> 1) & 1) * ts, lower[2] + (k & 1) * ts)
            assert all(corner[1 + d] in (lower[d], lower[d] + ts) and lower[d] <= xyz[d] <= lower[d] + ts for d in range(3))
            if float(w64[k, p_i]) == 0.0:
                assert int(rows[k, p_i]) == -1 and float(weights[k, p_i]) == 0.0, "a zero-weight corner is listed as present"
                if corner in table:
                    hit.append(table[corner])
        assert int((w64[:, p_i] == 0).sum()) == zero_corners and len(hit) == zero_corners, (p_i, hit)    # all of them are in the map
        xi = x.clone()
        xi[hit] = float("inf")
        got = ops.interp_fwd(xi, rows, weights)
        assert bool(torch.isfinite(got[p_i]).all()) and _bits(got[p_i], out[p_i]), f"point {p_i}: an Inf on a zero-weight corner reached the row"
        # the literal product 0 * Inf over all eight corners of the cell would be NaN: the case is a real one
        cell = [table[(0, lower[0] + ((k >> 2) & 1) * ts, lower[1] + ((k >> 1) & 1) * ts, lower[2] + (k & 1) * ts)] for k in range(8)]
        assert not bool(torch.isfinite((w64[:, p_i].float()[:, None] * xi.cpu()[cell]).sum(dim=0)).all())


def check_interp_bwd(ops, device, c):
    """The composition the autograd function uses: group the flattened [8, M] table by input row, then the weighted segment sum
    with src_mod = M; against the fp64 sum over (k, p)."""
    mgr, key, vox, pts, rows, weights, w64 = check_interp_map(ops, device, 2, 0)
    m, n_in = rows.shape[1], vox.shape[0]
    dy = values((m, c), 23, device)
    offsets, perm = ops.group(rows.reshape(-1), n_in)
    dx = ops.seg_rows(dy, offsets, perm, SUM, w=weights.reshape(-1), src_mod=m)[0]
    members = ref.members_of(rows.reshape(-1), n_in)
    want, mag, cnt = ref.seg_sum_ref(dy, members, weights.reshape(-1), src_mod=m)
    lens = torch.tensor([len(v) for v in members], dtype=torch.float64)
    _assert_within(dx, want, lens[:, None] * U * mag, f"interpolation backward c={c}")         # the reference takes the same fp32 weights


def check_floor_below_boundaries(device):
    """One ulp below a multiple of a stride that is no power of two, a quotient formed as x * (1 / ts) rounds onto the next
    integer (14.999999 * fl(1 / 3) = 5.0); a rounded division does not, except for the smallest negative numbers (-> -0).  However the quotient is formed, the point lands in the
    voxel below: `floor_points`, `TensorField.sparse`."""
    from pasco_amd.me.core import floor_points
    x15 = torch.nextafter(torch.tensor(15.0), torch.tensor(0.0))
    assert float(x15) < 15.0 and float(x15 * (torch.tensor(1.0) / 3)) == 5.0               # the hazard is real for a reciprocal
    for ts in (3, 5, 6, 7):
        k = torch.arange(-200, 201, dtype=torch.float32)
        x = torch.nextafter(k * ts, torch.full_like(k, -1e9))                                # one ulp below every boundary
        pts = torch.stack([torch.zeros_like(x), x, k * ts, x], dim=1).to(device)
        got = floor_points(pts, ts).cpu()
        want = torch.stack([torch.zeros_like(k), (k - 1) * ts, k * ts, (k - 1) * ts], dim=1).to(torch.int32)
        assert torch.equal(got, want), ts
    below = float(torch.nextafter(torch.tensor(3.0), torch.tensor(0.0)))
    coords = torch.tensor([[0, below, 3.0, -below], [0, 0.0, 5.0, -3.0]]).to(device)
    st = ME.TensorField(torch.ones(2, 1, device=device), coords, quantization_mode=Q.UNWEIGHTED_SUM).sparse(tensor_stride=3)
    assert st.C.cpu().tolist() == [[0, 0, 3, -3]] and st.F.cpu().tolist() == [[2.0]]


# ---- the module layer ----------------------------------------------------------------------------------------------------------
def cloud(n=600, seed=0, box=6.0, batches=2, c=5, dtype=torch.float32):
    """-> (features [n, c], coordinates [n, 4] float): points in [-1.5, box - 1.5)^3 (some negative), several per voxel."""
    g = _gen(seed)
    xyz = torch.rand(n, 3, generator=g) * box - 1.5
    xyz[:8] = torch.floor(xyz[:8])                              # a few exactly on voxel corners
    b = torch.randint(0, batches, (n, 1), generator=g).float()
    b[-1] = batches - 1
    return values((n, c), seed + 1, "cpu", torch.float32).to(dtype), torch.cat([b, xyz], dim=1).to(dtype)      # fp32 values in either dtype


def check_sparse_against_dense(device, dtype, ts=1):
    """`TensorField.sparse()` in every mode against the dense fp64 twin (index_add_ into a grid, divided by bincount)."""
    feats, coords = cloud(dtype=dtype)
    mmax = None
    for mode, name in ((Q.UNWEIGHTED_AVERAGE, "avg"), (Q.UNWEIGHTED_SUM, "sum"), (Q.MAX_POOL, "max")):
        field = ME.TensorField(feats.to(device), coords.to(device), quantization_mode=mode)
        st = field.sparse(tensor_stride=ts)
        twin, cnt_pt = ref.dense_quantise(feats, coords, ts, name)
        mags, _ = ref.dense_quantise(feats.abs(), coords, ts, "avg" if name == "avg" else "sum")
        mmax = float(cnt_pt.max())
        C, Fv = st.C.cpu().tolist(), st.F.cpu().double()
        assert len(C) == len(twin) and st.tensor_stride == [ts] * 3
        for r, v in enumerate(C):
            want, mag = twin[tuple(v)], mags[tuple(v)]
            if name == "max":
                assert torch.equal(Fv[r], want), (name, v)
            else:
                assert bool(((Fv[r] - want).abs() <= (mmax + 1) * U * mag + (0 if dtype == torch.float32 else 1e-300)).all()), (name, v)
        # rows and order: those of SparseTensor(features, floored coordinates)
        plain = SparseTensor(feats.to(device).float(), torch.cat([torch.floor(coords[:, :1]), torch.floor(coords[:, 1:] / ts) * ts], 1).to(device),
                             tensor_stride=ts)
        assert torch.equal(plain.C, st.C) and torch.equal(plain.inverse_mapping, field.inverse_mapping(st.coordinate_map_key))
    return mmax


def check_slice_and_interpolation(device, dtype):
    feats, coords = cloud(dtype=dtype)
    field = ME.TensorField(feats.to(device), coords.to(device))
    st = field.sparse()
    inv = field.inverse_mapping(st.coordinate_map_key).long()
    sl = st.slice(field)
    assert isinstance(sl, ME.TensorField) and sl.coordinate_field_map_key == field.coordinate_field_map_key
    assert torch.equal(sl.F, st.F[inv]) and torch.equal(sl.C, field.C)
    cs = st.cat_slice(field)
    assert torch.equal(cs.F, torch.cat([st.F[inv], field.F], dim=1))
    # a coarser map some points have no voxel in: zero rows (ours)
    keep = torch.arange(len(st), device=device) % 3 != 0
    out_key, keep_rows = st.coordinate_manager.prune(st.coordinate_map_key, keep)
    pruned = SparseTensor(st.F[keep_rows.long()], coordinate_map_key=out_key, coordinate_manager=st.coordinate_manager)
    ps = pruned.slice(field)
    lost = ~keep[inv]
    assert bool((ps.F[lost] == 0).all()) and torch.equal(ps.F[~lost], st.F[inv][~lost])
    assert bool((field.inverse_mapping(pruned.coordinate_map_key)[lost] == -1).all())


def check_interpolation_against_grid_sample(device, dtype):
    """A fully occupied 4 x 4 x 4 block against F.grid_sample(bilinear, align_corners=True) on the dense volume, interior points."""
    n, c = 4, 3
    r = torch.arange(n)
    g = torch.stack(torch.meshgrid(r, r, r, indexing="ij"), dim=-1).reshape(-1, 3)
    g = g[torch.randperm(n ** 3, generator=_gen(5))]
    coords = torch.cat([torch.zeros(n ** 3, 1, dtype=torch.int64), g], dim=1).to(torch.int32)
    feats = values((n ** 3, c), 31, "cpu", dtype)
    st = SparseTensor(feats.to(device), coords.to(device))
    pts = torch.rand(50, 3, generator=_gen(6), dtype=torch.float64) * (n - 1)
    q = torch.cat([torch.zeros(50, 1, dtype=torch.float64), pts], dim=1).to(dtype)
    out, rows, weights = ME.MinkowskiInterpolation(return_kernel_map=True, return_weights=True)(st, q.to(device))
    assert out.shape == (50, c) and rows.shape == (8, 50) and weights.shape == (8, 50)
    dense = torch.zeros((1, c, n, n, n), dtype=torch.float64)
    dense[0, :, g[:, 0], g[:, 1], g[:, 2]] = feats.double().t()
    # grid_sample's grid is (x, y, z) = (W, H, D) order in [-1, 1]: the volume is [D, H, W] = [X, Y, Z] here
    qd = q.double()[:, 1:]
    grid = (qd[:, [2, 1, 0]] / (n - 1) * 2 - 1).reshape(1, 1, 1, 50, 3)
    want = F.grid_sample(dense, grid, mode="bilinear", align_corners=True).reshape(c, 50).t()
    mag = F.grid_sample(dense.abs(), grid, mode="bilinear", align_corners=True).reshape(c, 50).t()
    tol = (32 * U if dtype == torch.float32 else 1e-12) * mag
    assert bool(((out.cpu().double() - want).abs() <= tol).all()), float(((out.cpu().double() - want).abs() / tol.clamp(min=1e-300)).max())
    assert ME.MinkowskiInterpolation()(st, q.to(device)).shape == (50, c)


def module_runs(device, dtype, c=5, n=300):
    """name -> run(features [N, c] requiring grad or not) -> output rows, for every served route from points to rows."""
    feats, coords = cloud(n=n, c=c, dtype=dtype, box=6.0 if n >= 100 else 3.0)
    if n < 100:                        # the small cloud of the difference quotients: no tiny column, no near ties
        feats = torch.randn(n, c, generator=_gen(77), dtype=torch.float64).to(dtype)
    coords = coords.to(device)
    q = torch.cat([torch.zeros(40, 1), torch.rand(40, 3, generator=_gen(8)) * 3], dim=1).to(device=device, dtype=dtype)

    def sparse(mode):
        return lambda f: ME.TensorField(f, coords, quantization_mode=mode).sparse().F

    def sparse_ts2(f):
        return ME.TensorField(f, coords).sparse(tensor_stride=2).F

    def tensor_mode(mode):
        return lambda f: SparseTensor(f, coords, quantization_mode=mode).F

    def sliced(f):
        field = ME.TensorField(f, coords)
        return field.sparse(tensor_stride=2).slice(field).F

    def cat_sliced(f):
        field = ME.TensorField(f, coords, quantization_mode=Q.UNWEIGHTED_SUM)
        return field.sparse().cat_slice(field).F

    def interpolated(f):
        return ME.MinkowskiInterpolation()(ME.TensorField(f, coords).sparse(), q)

    runs = {f"sparse_{m.name.lower()}": sparse(m) for m in QUANT_MODES}
    runs.update({f"tensor_{m.name.lower()}": tensor_mode(m) for m in (Q.UNWEIGHTED_AVERAGE, Q.UNWEIGHTED_SUM, Q.MAX_POOL)})
    runs.update(sparse_ts2=sparse_ts2, slice=sliced, cat_slice=cat_sliced, interpolation=interpolated)
    return feats.to(device), runs


MODULE_NAMES = [f"sparse_{m.name.lower()}" for m in QUANT_MODES] + \
    [f"tensor_{m.name.lower()}" for m in (Q.UNWEIGHTED_AVERAGE, Q.UNWEIGHTED_SUM, Q.MAX_POOL)] + ["sparse_ts2", "slice", "cat_slice", "interpolation"]


def check_module_modes(device, dtype, name):
    """The forward values are the same bits under no_grad, inference_mode and on the autograd route."""
    feats, runs = module_runs(device, dtype)
    run = runs[name]
    with torch.no_grad():
        a = run(feats)
    with torch.inference_mode():
        b = run(feats)
    f = feats.clone().requires_grad_(True)
    cgrad = run(f)
    assert cgrad.requires_grad and cgrad.grad_fn is not None
    assert torch.equal(a, b) and torch.equal(a, cgrad.detach()), name
    cgrad.backward(torch.ones_like(cgrad))
    assert f.grad is not None and f.grad.shape == feats.shape


def module_gradients(device, dtype, name):
    feats, runs = module_runs(device, dtype)
    f = feats.clone().requires_grad_(True)
    out = runs[name](f)
    out.backward(values(tuple(out.shape), 41, device, torch.float32).to(dtype))
    return out.detach().double().cpu(), f.grad.double().cpu()


def check_gradients_against_differences(name):
    """The CPU route in fp64: the backward of the autograd functions against central differences of their forward
    (torch.autograd.gradcheck on a cloud small enough to perturb every entry)."""
    device, dtype = torch.device("cpu"), torch.float64
    feats, runs = module_runs(device, dtype, c=2, n=40)
    f = feats.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: runs[name](t), (f,), eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0.0)


def check_prologue(device, dtype=torch.float32):
    """A pending eval-mode BatchNorm / ReLU on the input is applied before slice and interpolation."""
    feats, coords = cloud(n=200, dtype=dtype)
    field = ME.TensorField(feats.to(device), coords.to(device))
    st = field.sparse()
    c = feats.shape[1]
    scale, shift = values((1, c), 51, device, dtype).reshape(-1), values((1, c), 52, device, dtype).reshape(-1)
    q = torch.cat([torch.zeros(20, 1), torch.rand(20, 3, generator=_gen(8)) * 3], dim=1).to(device=device, dtype=dtype)
    plain = SparseTensor(torch.relu(st.F * scale + shift), coordinate_map_key=st.coordinate_map_key, coordinate_manager=st.coordinate_manager)
    for use in (lambda t: t.slice(field).F, lambda t: ME.MinkowskiInterpolation()(t, q)):
        pending = SparseTensor.deferred(st, scale, shift, 1, 0.0)
        assert pending._pending is not None
        assert torch.equal(use(pending), use(plain))


def check_existing_behaviour(device):
    """`SparseTensor(f, c)` and `quantization_mode=RANDOM_SUBSAMPLE`: rows, order, unique_index and inverse_mapping as before (the
    first occurrence of every coordinate, in input order); the dropout wrappers' rebuild of a field from its key round-trips."""
    feats, coords = cloud(n=200, dtype=torch.float32)
    ci = torch.floor(coords).to(torch.int32)
    seen, first, inv = {}, [], []
    for i, v in enumerate(ci.tolist()):
        if tuple(v) not in seen:
            seen[tuple(v)] = len(first)
            first.append(i)
        inv.append(seen[tuple(v)])
    for kw in ({}, {"quantization_mode": Q.RANDOM_SUBSAMPLE}, {"quantization_mode": None}):
        st = SparseTensor(feats.to(device), ci.to(device), **kw)
        assert torch.equal(st.C.cpu(), ci[first]) and torch.equal(st.F.cpu(), feats[first])
        assert st.unique_index.cpu().tolist() == first and st.inverse_mapping.cpu().tolist() == inv
    field = ME.TensorField(feats.to(device), coords.to(device), quantization_mode=Q.UNWEIGHTED_SUM)
    again = ME.TensorField(field.F * 2, coordinate_field_map_key=field.coordinate_field_map_key,
                           coordinate_manager=field.coordinate_manager, quantization_mode=field.quantization_mode)
    assert isinstance(again, ME.TensorField) and again.C is field.C and again.quantization_mode is Q.UNWEIGHTED_SUM
    assert torch.equal(again.sparse().C, field.sparse().C) and again.sparse().coordinate_map_key == field.sparse().coordinate_map_key
    assert torch.equal(again.sparse().F, field.sparse().F * 2)
    mgr = field.coordinate_manager
    assert mgr.number_of_unique_batch_indices() == 2 and len(field) == 200 and field.dtype == torch.float32
    cs, fs = field.decomposed_coordinates_and_features
    assert len(cs) == 2 and sum(x.shape[0] for x in cs) == 200 and torch.equal(fs[1], field.features_at(1))
    assert torch.equal(cs[0], field.coordinates_at(0)) and len(field.decomposed_features) == 2 and len(field.decomposed_coordinates) == 2
    stc, stf = field.sparse().decomposed_coordinates_and_features
    assert len(stc) == 2 and torch.equal(stf[0], field.sparse().features_at(0)) and len(field.sparse().decomposed_features) == 2
    assert [m.value for m in (Q.RANDOM_SUBSAMPLE, Q.UNWEIGHTED_AVERAGE, Q.UNWEIGHTED_SUM, Q.NO_QUANTIZATION)] == [0, 1, 2, 3]
    assert ME.TensorField(feats.to(device), torch.tensor([[0, -0.5, 0.5, -1.0]] * 200).to(device)).sparse().C.cpu().tolist() == [[0, -1, 0, -1]]


def check_refusals(device):
    import pytest
    feats, coords = cloud(n=50, dtype=torch.float32)
    feats, coords = feats.to(device), coords.to(device)
    with pytest.raises(NotImplementedError, match="SPLAT_LINEAR_INTERPOLATION"):
        ME.TensorField(feats, coords, quantization_mode=Q.SPLAT_LINEAR_INTERPOLATION).sparse()
    with pytest.raises(NotImplementedError, match="SPLAT_LINEAR_INTERPOLATION"):
        SparseTensor(feats, coords, quantization_mode=Q.SPLAT_LINEAR_INTERPOLATION)
    bad = coords.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        ME.TensorField(feats, bad)
    bad[3, 2] = float("inf")
    with pytest.raises(ValueError, match="NaN or an infinity"):
        ME.TensorField(feats, bad)
    same = coords.clone()
    same[1] = same[0]
    with pytest.raises(ValueError, match="NO_QUANTIZATION: 1 of 50 points share a voxel"):
        ME.TensorField(feats, same * 100, quantization_mode=Q.NO_QUANTIZATION).sparse()
    spread = torch.cat([torch.zeros(50, 1), torch.arange(50.0)[:, None].expand(50, 3)], dim=1).to(device)
    assert torch.equal(ME.TensorField(feats, spread, quantization_mode=Q.NO_QUANTIZATION).sparse().F, feats)
    with pytest.raises(ValueError, match="not a SparseTensorQuantizationMode"):
        ME.TensorField(feats, coords, quantization_mode="median")


def check_dtype_refusals(ops_module):
    """A non-fp32 dtype on device tensors is refused at the Python check, before any launch (no GPU needed: the check reads
    `is_cuda` and the dtype of a meta-free stand-in)."""
    import pytest

    class OnDevice:
        is_cuda, dtype = True, torch.float16

    with pytest.raises(TypeError, match="fp32 rows on the device"):
        ops_module.field_ops(OnDevice())


# ---- the end-to-end net --------------------------------------------------------------------------------------------------------
NET_BOX = 12


class FieldNet(nn.Module):
    """points -> TensorField (average) -> sparse -> conv(4, 16, k = 3) -> BN -> ReLU -> slice -> Linear."""

    def __init__(self):
        super().__init__()
        self.conv = ME.MinkowskiConvolution(4, 16, kernel_size=3, dimension=3)
        self.bn = ME.MinkowskiBatchNorm(16)
        self.relu = ME.MinkowskiReLU()
        self.head = nn.Linear(16, 7)

    def forward(self, feats, coords):
        field = ME.TensorField(feats, coords, quantization_mode=Q.UNWEIGHTED_AVERAGE)
        y = self.relu(self.bn(self.conv(field.sparse())))
        return self.head(y.slice(field).F)


def net_inputs(n=3000, seed=0):
    g = _gen(seed)
    xyz = torch.rand(n, 3, generator=g, dtype=torch.float64) * NET_BOX
    b = torch.randint(0, 2, (n, 1), generator=g).double()
    feats = torch.randn(n, 4, generator=g, dtype=torch.float64)
    target = torch.randn(n, 7, generator=g, dtype=torch.float64)
    return feats, torch.cat([b, xyz], dim=1), target


def net_twin_gradients(params, feats, coords, target):
    """The same network as dense fp64 torch operators: average into a [B, 4, X, Y, Z] grid, conv3d with zero padding (an absent
    neighbour contributes nothing), training-mode batch norm over the occupied sites, ReLU, read back at every point's voxel,
    Linear, mean squared error.  -> name -> gradient fp64."""
    p = {k: v.detach().double().cpu().requires_grad_(True) for k, v in params.items()}
    f = feats.clone().requires_grad_(True)
    b, v = coords[:, 0].long(), torch.floor(coords[:, 1:]).long()
    X = NET_BOX
    cell = ((b * X + v[:, 0]) * X + v[:, 1]) * X + v[:, 2]
    cnt = torch.bincount(cell, minlength=2 * X ** 3).double()
    grid = torch.zeros((2 * X ** 3, 4), dtype=torch.float64).index_add(0, cell, f) / cnt.clamp(min=1)[:, None]
    dense = grid.reshape(2, X, X, X, 4).permute(0, 4, 1, 2, 3)
    # kernel [27, cin, cout], offsets enumerated with x fastest: k = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1)
    w = p["conv.kernel"].reshape(3, 3, 3, 4, 16).permute(4, 3, 2, 1, 0)          # [cout, cin, dx, dy, dz]
    y = F.conv3d(dense, w, padding=1).permute(0, 2, 3, 4, 1).reshape(-1, 16)
    occ = cnt > 0
    rows = y[occ]
    mean, var = rows.mean(dim=0), rows.var(dim=0, unbiased=False)
    z = torch.relu((rows - mean) / torch.sqrt(var + 1e-5) * p["bn.bn.weight"] + p["bn.bn.bias"])
    row_of = torch.cumsum(occ.long(), 0) - 1
    out = z[row_of[cell]] @ p["head.weight"].t() + p["head.bias"]
    F.mse_loss(out, target).backward()
    grads = {k: t.grad for k, t in p.items()}
    grads["x"] = f.grad
    return grads


def net_gradients(device, dtype=torch.float32, seed=0):
    feats, coords, target = net_inputs()
    torch.manual_seed(3)
    net = FieldNet().to(device=device, dtype=dtype).train()
    f = feats.to(device=device, dtype=dtype).requires_grad_(True)
    out = net(f, coords.to(device=device, dtype=dtype))
    F.mse_loss(out, target.to(device=device, dtype=dtype)).backward()
    grads = {k: t.grad.detach().clone() for k, t in net.named_parameters()}
    grads["x"] = f.grad.detach().clone()
    params = {k: t.detach().clone() for k, t in net.named_parameters()}
    return params, grads, (feats, coords, target)
