"""Edge cases of the frame-preparation kernels (include/pasco_frame.h, csrc/frame.hip): pf_points, pf_transform_coords and
pf_label_bounds, each a function of (lib, dev) with `lib` a FrameLib.  Every result is held to tests/frame_ref.py exactly:
`array_equal` (bit patterns for the feature rows), plus `signbit` for the voxel array.  The builders below are numpy only
and assert that they hit what they claim, so tests/test_frame_edges_cpu.py runs them without a GPU and ties the
reference to the host restatements on the same inputs."""
import functools
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch

from tests import frame_ref as ref
from tests.frame_ref import Args

F32, F64 = np.float32, np.float64
CHUNK = 2048 * 256                       # points at which a block's chunk goes from one tile of 256 to two
SENT_F32 = 0x5A5A5A5A                    # bit pattern of every sentinel word
SENT_F64, SENT_I32, SENT_I64 = -12345.6789, -77, -99

# the two dataset layouts (data/kitti360.py, data/semantic_kitti.py) restated as numbers
EXTENT_LO, EXTENT_HI, ORIGIN = (0.0, -25.6, -2.0), (51.2, 25.6, 4.4), (0.0, -25.6, -2.0)
ROUNDED_UP = {b: float(F32(b)) > b for b in (-25.6, 51.2, 25.6, 4.4, -2.3, 0.1)}     # fp32 rounds the bounds both ways
assert len(set(ROUNDED_UP.values())) == 2 and all(float(F32(b)) != b for b in ROUNDED_UP), ROUNDED_UP


def k360_args(pts):
    return Args(EXTENT_LO, EXTENT_HI, (1, 1, 1), (0, 0, 0), ORIGIN, 0.2, True, [pts[:, 3:4]], [])


def sk_args(pts, vote, emb):
    return Args(EXTENT_LO, EXTENT_HI, (0, 0, 0), (0, 0, 0), ORIGIN, 0.2, False, [vote, pts[:, 3:4]], [emb])


# pts fp32 [P, 4]; args ref.Args; layouts: per segment "w" (the fourth column of pts itself), "plain", "transposed"
# ([w, P] in memory) or "slice" (columns of a wider tensor); host: None, "kitti360" or "semantic_kitti"
PointsCase = namedtuple("PointsCase", "pts args layouts host")


def inside(rng, n):
    return np.stack([rng.uniform(0.5, 50, n), rng.uniform(-25, 25, n), rng.uniform(-1.5, 4, n), rng.random(n)], 1).astype(F32)


def cloud(rng, n):
    """n points over and past the extent (about half are kept)."""
    return np.stack([rng.uniform(-10, 62, n), rng.uniform(-30, 30, n), rng.uniform(-2.6, 5, n), rng.random(n)], 1).astype(F32)


def with_layout(pts, layout, rng, wide=False):
    if layout == "kitti360":
        return PointsCase(pts, k360_args(pts), ["w"], "kitti360")
    n = pts.shape[0]
    v, e = (19, 256) if wide else (3, 5)
    vote, emb = rng.random((n, v)).astype(F32), rng.standard_normal((n, e)).astype(F32)
    return PointsCase(pts, sk_args(pts, vote, emb), ["plain", "w", "transposed"], "semantic_kitti")


# ---- builders: sizes ---------------------------------------------------------------------------------------------------
def sized(P, layout):
    rng = np.random.default_rng(P + 7)
    pts = cloud(rng, P)
    case = with_layout(pts, layout, rng)
    k = ref.keep_mask(pts, case.args)
    if P >= 63:
        assert 0 < k.sum() < P, "a size case keeps some points and drops some"
    return case


# ---- builders: keep masks ----------------------------------------------------------------------------------------------
MASKS = ("none", "all", "lane0", "lane63", "last", "alternating", "tile_then_empty", "random")


def masked(kind, layout):
    rng = np.random.default_rng(11)
    P = 512 if kind == "tile_then_empty" else 600
    i = np.arange(P)
    want = {"none": i < 0, "all": i >= 0, "lane0": i % 64 == 0, "lane63": i % 64 == 63, "last": i == P - 1,
            "alternating": i % 2 == 1, "tile_then_empty": i < 256, "random": rng.random(P) < 0.37}[kind]
    pts = inside(rng, P)
    out = np.flatnonzero(~want)
    pts[out, out % 3] = np.array([80.0, -26.0, 4.5], F32)[out % 3]           # outside through each axis in turn
    case = with_layout(pts, layout, rng)
    assert np.array_equal(ref.keep_mask(pts, case.args), want), kind
    return case


# ---- builders: crop flags ----------------------------------------------------------------------------------------------
FLAG_LO, FLAG_HI = (0.1, -25.6, -2.3), (51.3, 25.6, 4.7)
# A flag can only matter where fp32 rounds the bound DOWN (f < b): then f itself lies in [f, b), kept by `v >= f` and
# dropped by `v >= b` (and the reverse for `v < hi`).  Where fp32 rounds up no fp32 number lies between the two bounds.
FLAG_DOWN = [float(F32(b)) < b for b in FLAG_LO + FLAG_HI]


def flag_cloud():
    """Every bound, its fp32 rounding and that value's two fp32 neighbours, on an interior point."""
    pts = []
    for d in range(3):
        for b in (FLAG_LO[d], FLAG_HI[d]):
            f = F32(b)
            for v in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf)), F32(F64(b))):
                p = np.array([5.0, -3.0, 0.5, 0.25], F32)
                p[d] = v
                pts.append(p)
    pts.append(np.array([5.0, -3.0, 0.5, 0.75], F32))
    return np.stack(pts)


def flags(lo_fp64, hi_fp64, centre_fp64=True):
    pts = flag_cloud()
    return PointsCase(pts, Args(FLAG_LO, FLAG_HI, lo_fp64, hi_fp64, ORIGIN, 0.2, centre_fp64, [pts[:, 3:4]], []), ["w"], None)


def flag_claims():
    """Both rounding directions occur among the lower and among the upper bounds, and a flag alone changes which points are
    kept exactly where fp32 rounds its bound down."""
    assert all(float(F32(b)) != b for b in FLAG_LO + FLAG_HI)
    assert len(set(FLAG_DOWN[:3])) == 2 and len(set(FLAG_DOWN[3:])) == 2 and sum(FLAG_DOWN) == 3, FLAG_DOWN
    base = ref.keep_mask(flag_cloud(), flags((0, 0, 0), (0, 0, 0)).args)
    for d in range(3):
        one = tuple(int(a == d) for a in range(3))
        assert np.array_equal(ref.keep_mask(flag_cloud(), flags(one, (0, 0, 0)).args), base) != FLAG_DOWN[d], ("lo", d)
        assert np.array_equal(ref.keep_mask(flag_cloud(), flags((0, 0, 0), one).args), base) != FLAG_DOWN[3 + d], ("hi", d)


# ---- builders: centres, grids, floor division ---------------------------------------------------------------------------
def floor_div_branches(a, b):
    """npy_divmod's floor division restated; -> (quotient, the sign correction taken, the `div - fl > 0.5` correction taken)."""
    mod = np.fmod(a, b)
    div = (a - mod) / b
    sign = (mod != 0) & ((b < 0) != (mod < 0))
    div = np.where(sign, div - 1.0, div)
    fl = np.floor(div)
    up = (div != 0) & (div - fl > 0.5)
    return np.where(div != 0, np.where(up, fl + 1.0, fl), np.copysign(0.0, a / b)), sign, up


def gridded(origin, voxel, centre_fp64):
    """Random points and every voxel boundary origin + k voxel, k = -24..24, with its fp32 neighbours, on each axis; the crop
    extent is the origin +- 5 (fp64 bounds), so half the voxel indices are negative."""
    rng = np.random.default_rng(int(voxel * 100) + centre_fp64)
    o = np.asarray(origin, F64)
    rows = [(o + rng.uniform(-5.5, 5.5, (400, 3))).astype(F32)]
    base = (o + 0.37).astype(F32)
    for d in range(3):
        for k in range(-24, 25):
            f = F32(o[d] + k * voxel)
            for v in (np.nextafter(f, F32(-np.inf)), f, np.nextafter(f, F32(np.inf))):
                p = base.copy()
                p[d] = v
                rows.append(p[None])
    xyz = np.concatenate(rows)
    pts = np.concatenate([xyz, rng.random((xyz.shape[0], 1)).astype(F32)], 1)
    args = Args(tuple(o - 5), tuple(o + 5), (1, 1, 1), (1, 1, 1), tuple(o), voxel, centre_fp64, [pts[:, 3:4]], [])
    kept = pts[ref.keep_mask(pts, args), :3].astype(F64) - o
    q, sign, up = floor_div_branches(kept, F64(voxel))
    assert np.array_equal(q, kept // F64(voxel)) and (q < 0).any()
    assert sign.any(), "the sign correction of floor_div was not taken"
    if voxel != 0.25:                                   # 0.25 divides exactly: the quotient is never an ulp short
        assert up.any(), "the `div - fl > 0.5` correction of floor_div was not taken"
    return PointsCase(pts, args, ["w"], None)


# ---- builders: special coordinates --------------------------------------------------------------------------------------
def special(layout):
    rng = np.random.default_rng(5)
    good = inside(rng, 70)
    rows, expect = [], []
    for d in range(3):
        for v in (np.nan, np.inf, -np.inf):
            p = np.array([5.0, -3.0, 0.5, 0.1], F32)
            p[d] = v
            rows.append(p)
            expect.append(False)
    for x in (-0.0, 1e-45, 1e-40, 1.1754942e-38, -1e-45):              # -0.0 at the lower bound 0; subnormals either side of 0
        rows.append(np.array([x, -3.0, 0.5, 0.2], F32))
        expect.append(not (x < 0))
    rows.append(np.array([1e-20, 1e-20, 1e-20, 0.3], F32))            # squares and their sum are subnormal
    expect.append(True)
    rows.append(np.array([1e-40, 1e-41, 1e-42, 0.3], F32))
    expect.append(True)
    sp = np.stack(rows)
    pts = np.concatenate([good[:35], sp, good[35:]])                   # the special rows in the middle: they shift nothing
    case = with_layout(pts, layout, rng)
    keep = ref.keep_mask(pts, case.args)
    assert keep[:35].all() and keep[35 + len(rows):].all() and keep[35:35 + len(rows)].tolist() == expect
    feat, voxel, src, K = ref.ref_points(pts, case.args)
    zero = int(np.flatnonzero(src == 35 + 9)[0])                       # the -0.0 row
    assert voxel[zero, 0] == 0 and np.signbit(voxel[zero, 0]) and np.signbit(feat[zero, -3]), "-0.0 is kept as -0.0"
    assert np.isfinite(feat).all()
    return case


# ---- builders: segment layouts ------------------------------------------------------------------------------------------
SEGMENTS = {"none": ((), (), ()), "one_pre": ((2,), (), ("plain",)), "four_pre": ((1, 2, 3, 64), (), ("plain", "slice", "transposed", "plain")),
            "four_post": ((), (1, 64, 2, 3), ("transposed", "slice", "plain", "slice")), "transposed": ((3,), (2,), ("transposed", "transposed")),
            "slice": ((1,), (4,), ("slice", "slice")), "mixed": ((2, 1), (3, 1), ("slice", "w", "transposed", "plain"))}


def segmented(kind):
    rng = np.random.default_rng(len(kind))
    pts = cloud(rng, 300)
    pre_w, post_w, layouts = SEGMENTS[kind]
    mk = lambda w, lay: pts[:, 3:4] if lay == "w" else rng.standard_normal((300, w)).astype(F32)
    pre = [mk(w, lay) for w, lay in zip(pre_w, layouts)]
    post = [mk(w, lay) for w, lay in zip(post_w, layouts[len(pre_w):])]
    args = Args(EXTENT_LO, EXTENT_HI, (0, 1, 0), (1, 0, 0), ORIGIN, 0.2, False, pre, post)
    if kind.startswith("four"):
        assert 7 + sum(pre_w) + sum(post_w) > 64                         # the lane loop over the columns wraps
    return PointsCase(pts, args, list(layouts), None)


def real_size():
    rng = np.random.default_rng(120)
    return with_layout(cloud(rng, 120_000), "semantic_kitti", rng, wide=True)


POINT_BUILDERS = ([(f"size-{P}-{lay}", functools.partial(sized, P, lay)) for P in (0, 1, 63, 64, 65, 255, 256, 257, 511, 513)
                   for lay in ("kitti360", "semantic_kitti")]
                  + [(f"size-{P}-kitti360", functools.partial(sized, P, "kitti360")) for P in (CHUNK - 1, CHUNK, CHUNK + 1)]
                  + [(f"mask-{k}-{lay}", functools.partial(masked, k, lay)) for k in MASKS for lay in ("kitti360", "semantic_kitti")]
                  + [(f"grid-{v}-c{c}", functools.partial(gridded, o, v, c)) for o, v in (((0.3, -7.1, 1.9), 0.25), ((0.0, 0.0, 0.0), 0.1),
                                                                                         (ORIGIN, 0.2)) for c in (0, 1)]
                  + [(f"special-{lay}", functools.partial(special, lay)) for lay in ("kitti360", "semantic_kitti")]
                  + [(f"segments-{k}", functools.partial(segmented, k)) for k in SEGMENTS])


# ---- pf_points on the device --------------------------------------------------------------------------------------------
def filled(shape, dtype, dev):
    value = {torch.float32: float(np.array(SENT_F32, np.int32).view(F32)), torch.float64: SENT_F64, torch.int32: SENT_I32,
             torch.int64: SENT_I64}[dtype]
    return torch.full(shape, value, dtype=dtype, device=dev)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def device_segments(case, d_pts, dev):
    from pasco_amd.data.frame_lib import segment
    hold, segs = [], []
    for vals, lay in zip(list(case.args.pre) + list(case.args.post), case.layouts):
        P, w = vals.shape
        if lay == "w":
            t = d_pts[:, 3:]
        elif lay == "plain":
            t = torch.from_numpy(np.ascontiguousarray(vals)).to(dev)
        elif lay == "transposed":
            t = torch.from_numpy(np.ascontiguousarray(vals.T)).to(dev).t()
            assert P <= 1 or w == 1 or (t.stride(0), t.stride(1)) == (1, P)
        else:
            wide = torch.full((P, w + 5), 9e9, dtype=torch.float32, device=dev)
            wide[:, 2:2 + w] = torch.from_numpy(vals).to(dev)
            t = wide[:, 2:2 + w]
            assert P <= 1 or t.stride(0) > w
        if P == 0:                                                     # no storage behind an empty tensor: any non-null pointer
            t = torch.zeros((1, w), dtype=torch.float32, device=dev)
        hold.append(t)
        segs.append(segment(t))
    return segs, hold


def run_points(lib, dev, case):
    """Both calls (src given and null) against the reference; the rows from K on, and an unused src, keep the sentinel."""
    pts, a = case.pts, case.args
    P = pts.shape[0]
    d_pts = torch.from_numpy(np.ascontiguousarray(pts)).to(dev)
    segs, hold = device_segments(case, d_pts, dev)
    args = lib.points_args(a.lo, a.hi, a.lo_fp64, a.hi_fp64, a.origin, a.voxel, a.centre_fp64, segs[:len(a.pre)], segs[len(a.pre):])
    C = lib.channels(args)
    assert C == 7 + sum(s.shape[1] for s in list(a.pre) + list(a.post))
    e_feat, e_vox, e_src, K = ref.ref_points(pts, a)
    need = int(lib.lib.pf_points_workspace_bytes(P))
    got = []
    for want_src in (True, False):
        feat, vox = filled((P, C), torch.float32, dev), filled((P, 3), torch.float64, dev)
        src, kept = filled((P,), torch.int32, dev), filled((1,), torch.int64, dev)
        ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)[:need]
        lib.points_into(d_pts, args, feat, vox, src if want_src else None, kept, ws)
        feat, vox, src = feat.cpu().numpy(), vox.cpu().numpy(), src.cpu().numpy()
        assert int(kept.item()) == K, (int(kept.item()), K)
        assert np.array_equal(bits(feat[:K]), bits(e_feat)), int((bits(feat[:K]) != bits(e_feat)).any(1).sum())
        assert np.array_equal(vox[:K], e_vox) and np.array_equal(np.signbit(vox[:K]), np.signbit(e_vox))
        assert (bits(feat[K:]) == SENT_F32).all() and (vox[K:] == SENT_F64).all(), "rows from K on were written"
        if want_src:
            assert np.array_equal(src[:K], e_src) and (src[K:] == SENT_I32).all()
        else:
            assert (src == SENT_I32).all()
        got.append((feat, vox))
    assert np.array_equal(bits(got[0][0]), bits(got[1][0])) and np.array_equal(bits(got[0][1]), bits(got[1][1]))
    return K


def points(lib, dev, build):
    run_points(lib, dev, build())


def points_flags(lib, dev):
    """All 64 combinations of lo_fp64 / hi_fp64 on the cloud of bounds and neighbours, under both centre modes."""
    flag_claims()
    seen = set()
    for n, (lo, hi) in enumerate(itertools.product(itertools.product((0, 1), repeat=3), repeat=2)):
        case = flags(lo, hi, centre_fp64=bool(n % 2))
        run_points(lib, dev, case)
        seen.add(ref.keep_mask(case.pts, case.args).tobytes())
    assert len(seen) == 2 ** sum(FLAG_DOWN), "every flag on a bound that fp32 rounds down selects another set"


def points_workspace(lib, dev):
    """A workspace one byte short is refused with an error text, before anything is written."""
    for P in (0, 300, CHUNK + 1):
        case = sized(min(P, 300), "kitti360")
        d_pts = torch.zeros((P, 4), dtype=torch.float32, device=dev)
        a = case.args
        from pasco_amd.data.frame_lib import segment
        w = torch.zeros((max(P, 1), 1), dtype=torch.float32, device=dev)
        args = lib.points_args(a.lo, a.hi, a.lo_fp64, a.hi_fp64, a.origin, a.voxel, a.centre_fp64, [segment(w)], [])
        need = int(lib.lib.pf_points_workspace_bytes(P))
        assert need >= 4
        feat, vox, kept = filled((P, 8), torch.float32, dev), filled((P, 3), torch.float64, dev), filled((1,), torch.int64, dev)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        with pytest.raises(RuntimeError, match="pf_points: workspace of"):
            lib.points_into(d_pts, args, feat, vox, None, kept, ws[:need - 1])
        assert int(kept.item()) == SENT_I64 and (bits(feat.cpu().numpy()) == SENT_F32).all()


# ---- pf_transform_coords ------------------------------------------------------------------------------------------------
def rot_z(deg):
    c, s = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}[deg]
    T = np.eye(4, dtype=F32)
    T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    return T


def shift(metres):
    T = np.eye(4, dtype=F32)
    T[:3, 3] = F32(metres)
    return T


def transforms(kind, M=None):
    """-> list of fp32 [4, 4]: the eval table of M, or a named set."""
    if kind == "table":
        from pasco_amd.eval.kitti import subnet_transforms
        return [T.numpy().astype(F32) for T in subnet_transforms(M)]
    sets = {"identity": [np.eye(4, dtype=F32)], "quarter": [rot_z(90), rot_z(180), rot_z(270)], "shift40": [shift(8.0)],
            "half": [shift(0.1)], "quarter_shift": [rot_z(90) @ shift(8.0), rot_z(270), shift(-8.0)]}
    Ts = sets[kind]
    return Ts if M is None else [Ts[m % len(Ts)] for m in range(M)]


def coords_for(n, int_path, seed=0):
    rng = np.random.default_rng(n + seed)
    c = rng.integers(-64, 321, (n, 3)).astype(np.int64)
    if n >= 4:
        c[0], c[1], c[-1] = -64, 320, 0
    if int_path:
        return c
    c = c.astype(F64)
    if n >= 4:
        c[2] = -0.0
        c[-1, 1] = -0.0
    return c


def run_transform(lib, dev, coords, Ts, int_path, d_n="absent"):
    n, M = coords.shape[0], len(Ts)
    exp, val, near = ref.ref_transform(coords, Ts, int_path)
    d = torch.from_numpy(np.ascontiguousarray(coords)).to(dev)
    out = filled((M, n, 3), torch.int64, dev)
    n_dev = None if d_n == "absent" else torch.tensor([d_n], dtype=torch.int64, device=dev)
    lib.transform_coords(d, [torch.from_numpy(T) for T in Ts], n_dev=n_dev, out=out)
    got = out.cpu().numpy()
    lim = n if d_n == "absent" else min(d_n, n)
    assert np.array_equal(got[:, :lim], exp[:, :lim]), int((got[:, :lim] != exp[:, :lim]).sum())
    assert (got[:, lim:] == SENT_I64).all(), "rows from d_n[0] on were written"
    return val, near


def transform_sizes(lib, dev, n, int_path, M=3):
    run_transform(lib, dev, coords_for(n, int_path), transforms("table", M), int_path)


def transform_count(lib, dev, d_n, int_path):
    """d_n absent, 0, 1, inside a block, n, and beyond n (clamped): rows from min(d_n, n) on keep the sentinel for every m."""
    run_transform(lib, dev, coords_for(1000, int_path), transforms("table", 3), int_path, d_n)


def transform_kinds(lib, dev, kind, int_path):
    """Identity, quarter turns, 40 voxels, the eval table of 8 - and half a voxel, where every value sits on a tie and the
    defined order alone decides the rounding."""
    Ts = transforms(kind, 8 if kind == "table" else None)
    val, near = run_transform(lib, dev, coords_for(1000, int_path, seed=3), Ts, int_path)
    frac = np.abs(val - np.floor(val))
    if kind == "half":
        assert (np.abs(frac - 0.5) < 1e-3).all(), "a half-voxel translation puts every coordinate on a tie"
        assert near.mean() > 0.5
    elif kind != "table":
        assert (np.minimum(frac, 1 - frac) < 1e-3).all() and not near.any()


# ---- pf_label_bounds ----------------------------------------------------------------------------------------------------
PATTERNS = ("random", "all_unknown", "all_known", "ins_zero", "ins_last_site", "ins_on_unknown", "ins_255_or_0") + tuple(
    f"corner{k}" for k in range(8))


def labels(grid, pattern, seed=0):
    rng = np.random.default_rng(seed + sum(grid))
    sem = rng.integers(0, 20, grid).astype(np.uint8)
    sem[rng.random(grid) < 0.4] = 255
    ins = np.zeros(grid, np.uint8)
    ins[rng.random(grid) < 0.1] = 3
    ins[rng.random(grid) < 0.05] = 255
    if pattern == "all_unknown":
        sem[:] = 255
    elif pattern == "all_known":
        sem[sem == 255] = 0
    elif pattern == "ins_zero":
        ins[:] = 0
    elif pattern == "ins_last_site":
        ins[:] = 0
        ins[-1, -1, -1] = 7
        assert sem.size % 256 != 0 and sem.size > 256
    elif pattern == "ins_on_unknown":
        ins[:] = 0
        ins[sem == 255] = 4
        sem[0, 0, 0], ins[0, 0, 0] = 255, 4
    elif pattern == "ins_255_or_0":
        ins[:] = 0
        ins[rng.random(grid) < 0.5] = 255
        assert set(np.unique(ins)) == {0, 255}
    elif pattern.startswith("corner"):
        k = int(pattern[-1])
        sem[:] = 255
        sem[tuple((g - 1) * ((k >> (2 - d)) & 1) for d, g in enumerate(grid))] = 1
        assert (sem != 255).sum() == 1
    return sem, ins


def bounds_inputs(grid, kind, M, pattern):
    sem, ins = labels(grid, pattern)
    Ts = transforms(kind, M)
    Tinvs = [torch.inverse(torch.from_numpy(T)).numpy() for T in Ts]
    return sem, ins, Ts, Tinvs


def run_bounds(lib, dev, sem, ins, Ts, Tinvs, exp=None):
    """The loose host bound, the exact box and a one-voxel box size the second pass: the twelve words are the reference's
    all three times, on an `out` full of garbage, and twice over."""
    from pasco_amd.data.frame_lib import BOUNDS, box_upper_bound
    M = len(Ts)
    if exp is None:
        exp, _ = ref.ref_label_bounds(sem, ins, Ts, Tinvs)
    tT, tI = [torch.from_numpy(T) for T in Ts], [torch.from_numpy(T) for T in Tinvs]
    sd, idv = torch.from_numpy(sem).to(dev), torch.from_numpy(ins).to(dev)
    exact = torch.from_numpy(exp[:, :6].copy())
    exact[torch.from_numpy(exp[:, 0] == ref.INT32_MAX)] = 0              # an empty box: any valid bound
    for name, bb in (("loose", box_upper_bound(sem.shape, tT)), ("exact", exact), ("one voxel", torch.zeros((M, 6), dtype=torch.int32))):
        for run in range(2):
            out = filled((M, BOUNDS), torch.int32, dev)
            assert lib.label_bounds(sd, idv, tT, tI, bb, out=out) is out
            got = out.cpu().numpy()
            assert np.array_equal(got, exp), (name, run, got.tolist(), exp.tolist())
    return exp


def bounds(lib, dev, grid, kind, M, pattern="random"):
    sem, ins, Ts, Tinvs = bounds_inputs(grid, kind, M, pattern)
    exp = run_bounds(lib, dev, sem, ins, Ts, Tinvs)
    if pattern == "all_unknown":
        assert (exp[:, [0, 1, 2, 6, 7, 8]] == ref.INT32_MAX).all() and (exp[:, [3, 4, 5, 9, 10, 11]] == ref.INT32_MIN).all()
    if kind == "quarter":
        assert (exp[:, :3] < 0).any(), "the quarter turns put the box at negative indices"


BOUNDS_CASES = ([dict(grid=g, kind="table", M=3) for g in ((12, 10, 8), (9, 31, 7), (1, 40, 8), (40, 1, 8), (16, 16, 1))]
                + [dict(grid=(64, 64, 16), kind="quarter_shift", M=3)]
                + [dict(grid=(12, 10, 8), kind=k, M=M) for k, M in (("table", 1), ("table", 8), ("quarter", 3), ("shift40", 1), ("half", 1),
                                                                     ("quarter", 8))]
                + [dict(grid=g, kind="quarter", M=3) for g in ((1, 40, 8), (40, 1, 8), (16, 16, 1))]
                + [dict(grid=(9, 31, 7), kind="table", M=3, pattern=p) for p in PATTERNS[1:]])


# ---- a real frame's size ------------------------------------------------------------------------------------------------
def full_labels():
    rng = np.random.default_rng(8)
    grid = (256, 256, 32)
    sem = np.full(grid, 255, np.uint8)
    sem[90:190, 60:180, 2:18] = rng.integers(0, 20, (100, 120, 16))
    sem[rng.random(grid) < 0.3] = 255
    ins = np.zeros(grid, np.uint8)
    ins[100:110, 70:80, 3:9] = 4
    ins[:, 250:, :] = 255
    return sem, ins


def full_size(lib, dev):
    """120 000 points in the 283-channel layout; a 256 x 256 x 32 grid under the eval table of 8."""
    case = real_size()
    assert run_points(lib, dev, case) > 30_000
    sem, ins = full_labels()
    Ts = transforms("table", 8)
    run_bounds(lib, dev, sem, ins, Ts, [torch.inverse(torch.from_numpy(T)).numpy() for T in Ts])


def _case(fn, **kw):
    f = functools.partial(fn, **kw)
    return pytest.param(f, id="-".join([fn.__name__] + [str(v).replace(" ", "") for v in kw.values()]))


CASES = ([pytest.param(functools.partial(points, build=b), id="points-" + name) for name, b in POINT_BUILDERS]
         + [_case(points_flags), _case(points_workspace)]
         + [_case(transform_sizes, n=n, int_path=p) for n in (0, 1, 255, 256, 257, CHUNK + 1) for p in (True, False)]
         + [_case(transform_sizes, n=257, int_path=p, M=M) for M in (1, 8) for p in (True, False)]
         + [_case(transform_count, d_n=d, int_path=p) for d in ("absent", 0, 1, 300, 1000, 1005) for p in (True, False)]
         + [_case(transform_kinds, kind=k, int_path=p) for k in ("table", "identity", "quarter", "shift40", "half") for p in (True, False)]
         + [_case(bounds, **kw) for kw in BOUNDS_CASES])
