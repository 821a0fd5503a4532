"""An independent reference of the three frame-preparation operations (include/pasco_frame.h, csrc/frame.hip), in plain
numpy from the header's definitions.  It shares no code with the host restatements (data/semantic_kitti.py,
data/kitti360.py, data/device_prep.py); tests/test_frame_edges_cpu.py ties it to them and to the recorded outputs of the
reference project, tests/test_hip_frame_edges.py holds the kernels to it.

How the fmaf is exact.  fmaf(a, b, c) is the fp32 rounding of the real number a b + c.  The product of two fp32 numbers
has at most 48 significant bits, so p = a b is exact in fp64.  The sum p + c need not be: it is taken as an error-free
sum (Knuth's TwoSum), s = fl64(p + c) and e with s + e = p + c exactly.  |e| is at most half an fp64 ulp of s, so s + e
lies on the same side of every fp32 midpoint as s does - midpoints are fp64 numbers - unless s IS a midpoint.  There
fp32(s) would break the tie to even although the real sum is not a tie: the sign of e decides instead.  Everywhere else
fp32(s) is the correctly rounded result.  No step rounds twice."""
from collections import namedtuple

import numpy as np

F32, F64 = np.float32, np.float64
MINB = np.array([0, -25.6, -2], F32)          # min_bound of transform_coords: fp32
INT32_MAX, INT32_MIN = 2 ** 31 - 1, -2 ** 31

# lo / hi / origin: 3 floats; lo_fp64 / hi_fp64: 3 flags; pre / post: lists of fp32 [P, w] arrays (the VALUES of the
# pass-through columns, whatever strides the device segment reads them with)
Args = namedtuple("Args", "lo hi lo_fp64 hi_fp64 origin voxel centre_fp64 pre post")


def keep_mask(pts, a):
    """lo <= v < hi per axis, each bound compared in fp32 (the bound rounded to fp32) or in fp64 as flagged."""
    pts = np.asarray(pts, F32)
    keep = np.ones(pts.shape[0], bool)
    for d in range(3):
        v = pts[:, d]
        lo, hi = F64(a.lo[d]), F64(a.hi[d])
        keep &= (v.astype(F64) >= lo) if a.lo_fp64[d] else (v >= F32(lo))
        keep &= (v.astype(F64) < hi) if a.hi_fp64[d] else (v < F32(hi))
    return keep


def ref_points(pts, a):
    """-> (feat fp32 [K, C], voxel fp64 [K, 3], src int32 [K], K): the kept points in input order."""
    pts = np.asarray(pts, F32)
    keep = keep_mask(pts, a)
    src = np.nonzero(keep)[0].astype(np.int32)
    xyz = pts[keep, :3]
    origin = np.asarray(a.origin, F64).reshape(1, 3)
    voxel = (xyz.astype(F64) - origin) // F64(a.voxel)                   # numpy's floor division, signs as they come
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    radius = np.sqrt((x * x + y * y) + z * z)
    assert radius.dtype == F32
    if a.centre_fp64:
        centre = (voxel + 0.5) * F64(a.voxel) + origin
    else:
        centre = ((voxel.astype(F32) + F32(0.5)) * F32(a.voxel)).astype(F64) + origin
    dxyz = (xyz.astype(F64) - centre).astype(F32)
    cols = [np.asarray(s, F32)[keep] for s in a.pre] + [radius[:, None]] + [np.asarray(s, F32)[keep] for s in a.post]
    feat = np.concatenate(cols + [dxyz, xyz], axis=1).astype(F32)
    return feat, voxel, src, int(src.size)


def fmaf(a, b, c):
    """The fp32 rounding of a b + c for fp32 arrays, exact (module docstring)."""
    a, b, c = (np.asarray(v, F32).astype(F64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    r = s.astype(F32)
    up, down = np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf))
    r64 = r.astype(F64)
    r = np.where((s == (r64 + up.astype(F64)) / 2) & (e > 0), up, r)     # s on a midpoint, the real sum above it
    r = np.where((s == (r64 + down.astype(F64)) / 2) & (e < 0), down, r)
    return r.astype(F32)


def metres(coords, int_path):
    if int_path:
        return MINB + (np.asarray(coords).astype(F32) * F32(0.2) + F32(0.1))
    return (MINB.astype(F64) + (np.asarray(coords, F64) * 0.2 + 0.1)).astype(F32)


def near_tie(v):
    """Within one ulp of a .5 tie of the rounding (the definition of tests/test_hip_frame.py)."""
    return np.abs(np.abs(v - np.floor(v)) - F32(0.5)) <= np.spacing(np.abs(v))


def ref_transform(coords, Ts, int_path):
    """coords int64 (int_path) or fp64 [n, 3], Ts [M, 4, 4] -> (int64 [M, n, 3], the fp32 values before the rounding
    [M, n, 3], near_tie bool [M, n, 3]).  The defined order: metres, the fmaf chain k = 0..3 from 0,
    ((v - mb) - 0.1f) / 0.2f, round half to even."""
    h = metres(coords, int_path)
    n = h.shape[0]
    h4 = np.concatenate([h, np.ones((n, 1), F32)], 1)
    M = len(Ts)
    val = np.empty((M, n, 3), F32)
    for m in range(M):
        T = np.asarray(Ts[m], F32).reshape(4, 4)
        for i in range(3):
            acc = np.zeros(n, F32)
            for k in range(4):
                acc = fmaf(np.full(n, T[i, k], F32), h4[:, k], acc)
            val[m, :, i] = ((acc - MINB[i]) - F32(0.1)) / F32(0.2)
    return np.rint(val).astype(np.int32).astype(np.int64), val, near_tie(val)


def ref_label_bounds(sem, ins, Ts, Tinvs):
    """-> (int32 [M, 12], any value of either pass near a tie), brute force from the header: words 0..5 the box of the
    transformed known voxels, words 6..11 the min / max over every sample of that box that T^-1 maps into the grid onto
    sem != 255 or, when any ins != 0, onto ins != 255.  Empty sets stay at INT32_MAX / INT32_MIN."""
    sem, ins = np.asarray(sem, np.uint8), np.asarray(ins, np.uint8)
    X, Y, Z = sem.shape
    M = len(Ts)
    out = np.empty((M, 12), np.int64)
    out[:, [0, 1, 2, 6, 7, 8]] = INT32_MAX
    out[:, [3, 4, 5, 9, 10, 11]] = INT32_MIN
    sites = np.argwhere(sem != 255).astype(np.int64)
    flag = bool((ins != 0).any())
    hit = (sem != 255) | ((ins != 255) if flag else False)
    tie = False
    for m in range(M):
        if sites.shape[0] == 0:
            continue
        to, _, near = ref_transform(sites, [Ts[m]], True)
        tie = tie or bool(near.any())
        lo, hi = to[0].min(0), to[0].max(0)
        out[m, 0:3], out[m, 3:6] = lo, hi
        axes = [np.arange(lo[d], hi[d] + 1, dtype=np.int64) for d in range(3)]
        samples = np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], 1)
        back, _, near = ref_transform(samples, [Tinvs[m]], True)
        tie = tie or bool(near.any())
        b = back[0]
        inside = (b[:, 0] >= 0) & (b[:, 0] < X) & (b[:, 1] >= 0) & (b[:, 1] < Y) & (b[:, 2] >= 0) & (b[:, 2] < Z)
        s, b = samples[inside], b[inside]
        s = s[hit[b[:, 0], b[:, 1], b[:, 2]]]
        if s.shape[0]:
            out[m, 6:9], out[m, 9:12] = s.min(0), s.max(0)
    return out.astype(np.int32), tie
