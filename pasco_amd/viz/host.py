"""numpy restatement of every `pv_*` entry point (include/pasco_view.h, csrc/view.hip): the same operations in the same order,
one rounded fp32 operation at a time (numpy never contracts a multiply and an add).  `python -m pasco_amd.viz --device cpu`
runs these; tests/test_hip_view.py holds the kernels equal to them on every byte."""
from __future__ import annotations

import numpy as np

MAX_LABEL = 32
MAX_SEGMENTS = 128
BRICK = 8
SENTINEL = np.float32(255.0)
STATUS_LABEL_RANGE, STATUS_STEP_CAP, STATUS_PALETTE = 1, 2, 4
OPS = {"median": 0, "max": 1, "avg": 2}
VIEWS = {"semantic": 0, "panoptic": 1, "mask": 2, "vox_conf": 3, "ins_conf": 4}
INSTANCE_BASE, RAMP_BASE, STUFF_FIRST, STUFF_LAST = 32, 1, 9, 19
FACE_INSIDE, FACE_NONE = 6, 255

_F = np.float32
_INF = np.float32(np.inf)


def majority_pool(grid: np.ndarray, k: int):
    """uint8 [X, Y, Z] -> (uint8 [X//k, Y//k, Z//k], status)."""
    assert grid.dtype == np.uint8 and grid.ndim == 3 and k in (2, 4, 8)
    X, Y, Z = grid.shape
    ox, oy, oz = X // k, Y // k, Z // k
    cells = grid[:ox * k, :oy * k, :oz * k].reshape(ox, k, oy, k, oz, k).transpose(0, 2, 4, 1, 3, 5).reshape(ox, oy, oz, k ** 3)
    best = np.zeros((ox, oy, oz), np.int32)
    best_n = np.zeros((ox, oy, oz), np.int32)
    for l in range(1, MAX_LABEL):
        n = (cells == l).sum(-1).astype(np.int32)
        take = n > best_n
        best_n = np.where(take, n, best_n)
        best = np.where(take, l, best)
    has0 = (cells == 0).any(-1)
    bad = ((cells >= MAX_LABEL) & (cells != 255)).any()
    out = np.where(best_n > 0, best, np.where(has0, 0, 255)).astype(np.uint8)
    return out, (STATUS_LABEL_RANGE if bad else 0)


def window_filter(grid: np.ndarray, op: str, mask: np.ndarray = None) -> np.ndarray:
    """fp32 [X, Y, Z] -> fp32 [X, Y, Z]; `op` in median / max / avg; `mask` uint8 [X, Y, Z] or None."""
    assert grid.dtype == np.float32 and grid.ndim == 3 and op in OPS
    X, Y, Z = grid.shape
    ok = grid != SENTINEL
    if mask is not None:
        ok &= mask != 0
    pad_v = np.full((X + 2, Y + 2, Z + 2), _INF, np.float32)
    pad_ok = np.zeros((X + 2, Y + 2, Z + 2), bool)
    pad_v[1:-1, 1:-1, 1:-1] = grid
    pad_ok[1:-1, 1:-1, 1:-1] = ok
    n = np.zeros((X, Y, Z), np.int32)
    total = np.zeros((X, Y, Z), np.float32)
    mx = np.full((X, Y, Z), -_INF, np.float32)
    vals = np.empty((X, Y, Z, 27), np.float32) if op == "median" else None
    slot = 0
    for dx in range(3):                      # raster order of the window: x, then y, then z fastest
        for dy in range(3):
            for dz in range(3):
                v = pad_v[dx:dx + X, dy:dy + Y, dz:dz + Z]
                o = pad_ok[dx:dx + X, dy:dy + Y, dz:dz + Z]
                n += o
                if op == "avg":
                    total = np.where(o, total + v, total)
                elif op == "max":
                    mx = np.where(o & (v > mx), v, mx)
                else:
                    vals[..., slot] = np.where(o, v, _INF)
                slot += 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if op == "avg":
            r = total / n.astype(np.float32)
        elif op == "max":
            r = mx
        else:
            vals.sort(axis=-1)
            lo, hi = (n - 1) >> 1, n >> 1
            a = np.take_along_axis(vals, np.maximum(lo, 0)[..., None], -1)[..., 0]
            b = np.take_along_axis(vals, hi[..., None], -1)[..., 0]
            r = np.where(lo == hi, a, (a + b) * _F(0.5))
    return np.where(n == 0, SENTINEL, r).astype(np.float32)


def quantise(c, vmin, vmax) -> np.ndarray:
    c = np.asarray(c, np.float32)
    vmin, vmax = _F(vmin), _F(vmax)
    if not vmax > vmin:
        return np.zeros(c.shape, np.uint32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (c - vmin) / (vmax - vmin)
        t = np.where(t > 0, t, _F(0))
        t = np.where(t < 1, t, _F(1))
        return (t * _F(255.0) + _F(0.5)).astype(np.int32).astype(np.uint32)


def compose(view: str, shape, panoptic=None, seg=None, sem=None, conf=None, vmin=0.0, vmax=1.0) -> np.ndarray:
    """-> uint32 [X, Y, Z] colour indices.  seg: int32 [4, n_seg] (id, isthing, category, confidence bits) or None."""
    v = VIEWS[view]
    out = np.zeros(shape, np.uint32)
    if v == 0:
        return np.where((sem != 0) & (sem != 255), sem, 0).astype(np.uint32)
    if v == 3:
        return np.where(sem != 0, RAMP_BASE + quantise(conf, vmin, vmax), 0).astype(np.uint32)
    seg = np.zeros((4, 0), np.int32) if seg is None else np.asarray(seg, np.int32)
    n_seg = seg.shape[1]
    assert n_seg <= MAX_SEGMENTS
    thing = seg[1] != 0
    rank = np.cumsum(thing)
    q = quantise(seg[3].view(np.float32), vmin, vmax)
    done = panoptic == 0                       # the first segment with a voxel's id owns it
    for s in range(n_seg):
        m = (panoptic == seg[0, s]) & ~done
        done |= m
        if thing[s]:
            out[m] = RAMP_BASE + q[s] if v == 4 else INSTANCE_BASE + rank[s] - 1
    if v == 1:
        stuff = (out == 0) & (sem >= STUFF_FIRST) & (sem <= STUFF_LAST)
        out[stuff] = sem[stuff]
    return out


def brick_dims(shape):
    return tuple((int(n) + BRICK - 1) // BRICK for n in shape)


def brick_words(shape) -> int:
    nb = brick_dims(shape)
    return (nb[0] * nb[1] * nb[2] + 31) // 32


def bricks(colour: np.ndarray) -> np.ndarray:
    """uint32 [X, Y, Z] -> uint32 [brick_words] occupancy bits."""
    X, Y, Z = colour.shape
    nb = brick_dims(colour.shape)
    pad = np.zeros((nb[0] * BRICK, nb[1] * BRICK, nb[2] * BRICK), bool)
    pad[:X, :Y, :Z] = colour != 0
    occ = pad.reshape(nb[0], BRICK, nb[1], BRICK, nb[2], BRICK).any(axis=(1, 3, 5)).reshape(-1)
    words = np.zeros(brick_words(colour.shape) * 32, np.uint32)
    words[:occ.size] = occ
    return (words.reshape(-1, 32) << np.arange(32, dtype=np.uint32)).sum(1, dtype=np.uint32)


def _clamp_cell(p, lo, hi):
    flo, fhi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    p = np.where(p > flo, p, flo)
    p = np.where(p < fhi, p, fhi)
    return p.astype(np.int32)


def render(colour: np.ndarray, bits: np.ndarray, cam, W: int, H: int, palette: np.ndarray, factors=(256, 256, 256),
           background=(255, 255, 255), step_cap: int = 0):
    """-> (hit int32 [H, W], face uint8 [H, W], rgb uint8 [H, W, 3], status); the walk of pasco_view.h, every ray at once."""
    cam = np.asarray(cam, np.float32)
    assert cam.shape == (12,) and colour.dtype == np.uint32 and palette.dtype == np.uint8
    n = np.array(colour.shape, np.int32)
    nb = np.array(brick_dims(colour.shape), np.int32)
    flat = colour.reshape(-1)
    N = W * H
    fi = np.tile(np.arange(W, dtype=np.float32), H)
    fj = np.repeat(np.arange(H, dtype=np.float32), W)
    cap_fine, cap_coarse = int(n.sum()) + 3, int(nb.sum()) + 3
    if step_cap > 0:
        cap_fine, cap_coarse = min(cap_fine, step_cap), min(cap_coarse, step_cap)

    with np.errstate(all="ignore"):
        o = np.empty((3, N), np.float32)
        d = np.empty((3, N), np.float32)
        inv = np.zeros((3, N), np.float32)
        st = np.zeros((3, N), np.int32)
        miss = np.zeros(N, bool)
        t0 = np.zeros(N, np.float32)
        t1 = np.full(N, _INF, np.float32)
        ea = np.full(N, -1, np.int32)
        for a in range(3):
            o[a] = cam[a]
            d[a] = (cam[3 + a] + fi * cam[6 + a]) + fj * cam[9 + a]
            ext = _F(n[a])
            zero = d[a] == 0
            miss |= zero & ~((o[a] >= 0) & (o[a] < ext))
            st[a] = np.where(zero, 0, np.where(d[a] > 0, 1, -1))
            inv[a] = np.where(zero, _F(0), _F(1) / np.where(zero, _F(1), d[a]))
            ta, tb = (_F(0) - o[a]) * inv[a], (ext - o[a]) * inv[a]
            tn, tf = np.where(ta < tb, ta, tb), np.where(ta < tb, tb, ta)
            up = ~zero & (tn > t0)
            t0 = np.where(up, tn, t0)
            ea = np.where(up, a, ea)
            t1 = np.where(~zero & (tf < t1), tf, t1)
        miss |= ~(t0 <= t1)

        c = np.empty((3, N), np.int32)
        for a in range(3):
            c[a] = _clamp_cell(o[a] + t0 * d[a], 0, n[a] - 1)
        face = np.full(N, FACE_INSIDE, np.int32)
        for a in range(3):
            e = ea == a
            c[a] = np.where(e, np.where(st[a] > 0, 0, n[a] - 1), c[a])
            face = np.where(e, 2 * a + (st[a] < 0), face)
        bc = c >> 3

        result = np.full(N, -1, np.int32)
        index = np.zeros(N, np.uint32)
        status = 0
        fine = np.zeros(N, np.int32)
        coarse = np.zeros(N, np.int32)
        live = np.flatnonzero(~miss)          # rays still walking; everything below is indexed by it
        while live.size:
            L = live
            b = (bc[0, L] * nb[1] + bc[1, L]) * nb[2] + bc[2, L]
            occ = ((bits[b >> 5] >> (b & 31).astype(np.uint32)) & 1).astype(bool)
            site = (c[0, L] * n[1] + c[1, L]) * n[2] + c[2, L]
            v = flat[site]
            got = occ & (v != 0)
            result[L[got]] = site[got]
            index[L[got]] = v[got]
            capped = (occ & ~got & (fine[L] >= cap_fine)) | (~occ & (coarse[L] >= cap_coarse))
            if capped.any():
                status |= STATUS_STEP_CAP
            go = ~got & ~capped
            L, occ = L[go], occ[go]
            fine[L] += occ
            coarse[L] += ~occ
            s, oo, ii, dd = st[:, L], o[:, L], inv[:, L], d[:, L]
            plus = (s > 0).astype(np.int32)
            plane = np.where(occ[None], c[:, L] + plus, (bc[:, L] + plus) * BRICK).astype(np.float32)
            tm = np.where(s == 0, _INF, (plane - oo) * ii)
            a = np.zeros(L.size, np.int32)
            a = np.where(tm[1] < tm[0], 1, a)
            a = np.where(tm[2] < np.take_along_axis(tm, a[None], 0)[0], 2, a)
            t = np.take_along_axis(tm, a[None], 0)[0]
            out = np.zeros(L.size, bool)
            cc, bb = c[:, L], bc[:, L]
            for k in range(3):
                ax = a == k
                # a voxel step on axis k
                ck = np.where(ax & occ, cc[k] + s[k], cc[k])
                out |= ax & occ & ((ck < 0) | (ck >= n[k]))
                # a brick step on axis k, or the re-derived cell of the other axes
                bk = np.where(ax & ~occ, bb[k] + s[k], bb[k])
                out |= ax & ~occ & ((bk < 0) | (bk >= nb[k]))
                lo = bk * BRICK
                hi = np.minimum(lo + BRICK - 1, n[k] - 1)
                entered = np.where(s[k] > 0, lo, lo + BRICK - 1)
                other = _clamp_cell(oo[k] + t * dd[k], lo, hi)
                ck = np.where(occ, ck, np.where(ax, entered, other))
                bk = np.where(occ, ck >> 3, bk)
                face[L] = np.where(ax, 2 * k + (s[k] < 0), face[L])
                c[k, L], bc[k, L] = ck, bk
            live = L[~out]

    hit_mask = result >= 0
    over = hit_mask & (index >= palette.shape[0])
    if over.any():
        status |= STATUS_PALETTE
    index = np.where(over, palette.shape[0] - 1, index)
    f = np.asarray(factors, np.int32)[np.where(face == FACE_INSIDE, 2, face >> 1)]
    rgb = (palette[index].astype(np.int32) * f[:, None]) >> 8
    rgb = np.where(hit_mask[:, None], rgb, np.asarray(background, np.int32)[None]).astype(np.uint8)
    face = np.where(hit_mask, face, FACE_NONE).astype(np.uint8)
    return result.reshape(H, W), face.reshape(H, W), rgb.reshape(H, W, 3), status


def downsample(img: np.ndarray, s: int) -> np.ndarray:
    """uint8 [H*s, W*s, 3] -> uint8 [H, W, 3]."""
    assert img.dtype == np.uint8 and img.shape[0] % s == 0 and img.shape[1] % s == 0
    H, W = img.shape[0] // s, img.shape[1] // s
    total = img.reshape(H, s, W, s, 3).astype(np.int32).sum(axis=(1, 3))
    return ((total + s * s // 2) // (s * s)).astype(np.uint8)
