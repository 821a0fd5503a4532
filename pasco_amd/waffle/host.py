"""Restatement of every `pw_*` entry point (include/pasco_waffle.h, csrc/waffle.hip) and of the network around them.

Decisions (voxel keys, crop, cell indices, the CSR, the neighbour searches) are numpy integers, fp32 and fp64, one rounded
operation at a time in the order the kernels use (numpy never contracts a multiply and an add), so they are equal bit for bit.
The network (`forward`) is plain torch on whatever device its tensors are on: `python -m pasco_amd.waffle --device cpu` runs
it, and tools/waffle_time.py times it on the GPU beside the kernel route."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

MAX_K = 32
MAX_FEAT = 8
MAX_CELLS = 1 << 24
STATUS_OFF_GRID, STATUS_ORDER, STATUS_INDEX, STATUS_KEY_RANGE = 1, 2, 4, 8

_F = np.float32
_SHRINK = 1.0 - 2.0 ** -20          # the search stops when the worst kept d2 < _SHRINK * (lower bound of the next shell)


@dataclass(frozen=True)
class SearchGrid:
    """Uniform grid of cubic cells for `knn` / `nearest`: origin `lo`, edge `h`, `G` cells per axis (fp64 geometry)."""
    lo: Tuple[float, float, float]
    h: float
    G: Tuple[int, int, int]

    @property
    def ncell(self) -> int:
        return int(self.G[0]) * int(self.G[1]) * int(self.G[2])

    @staticmethod
    def around(mn: Sequence[float], mx: Sequence[float], h: float = 0.5, max_cells: int = 1 << 22) -> "SearchGrid":
        """The grid that holds every point of a cloud with per-axis minimum `mn` and maximum `mx` (fp32 values): the edge is
        doubled until the grid has at most `max_cells` cells."""
        lo = tuple(float(v) for v in mn)
        h = float(h)
        while True:
            G = tuple(int(np.floor((float(b) - a) / h)) + 1 for a, b in zip(lo, mx))
            if G[0] * G[1] * G[2] <= max_cells:
                return SearchGrid(lo, h, G)
            h *= 2.0


# ---- preparation ------------------------------------------------------------------------------------------------------
def voxel_keys(pc: np.ndarray, mn: np.ndarray, voxel: float):
    """fp32 [n, >= 3], fp32 [3] -> (int32 [n, 3], status)."""
    assert pc.dtype == np.float32 and mn.dtype == np.float32
    qf = (pc[:, :3] - mn[None, :3]) / _F(voxel)
    ok = (qf >= 0) & (qf < _F(2097152.0))
    key = np.where(ok, qf, 0).astype(np.int32)
    return key, (0 if ok.all() else STATUS_KEY_RANGE)


def first_of_keys(key: np.ndarray) -> np.ndarray:
    """int32 [n, 3] -> the index of the first row of every distinct key, in lexicographic key order (what
    `np.unique(key, axis=0, return_index=True)` returns)."""
    k = key.astype(np.int64)
    if k.shape[0] == 0:
        return np.zeros(0, np.int64)
    r1, r2 = int(k[:, 1].max()) + 1, int(k[:, 2].max()) + 1
    flat = (k[:, 0] * r1 + k[:, 1]) * r2 + k[:, 2]
    order = np.argsort(flat, kind="stable")
    s = flat[order]
    first = np.ones(s.shape[0], bool)
    first[1:] = s[1:] != s[:-1]
    return order[first]


def crop_mask(pc: np.ndarray, fov, eps: float = 1e-4) -> np.ndarray:
    """Strictly inside the field of view shrunk by eps; the bounds are rounded to fp32 once, the comparisons are fp32."""
    keep = np.ones(pc.shape[0], bool)
    for a in range(3):
        keep &= (pc[:, a] > _F(fov[0][a] + eps)) & (pc[:, a] < _F(fov[1][a] - eps))
    return keep


def cell_index(pc: np.ndarray, dims, lo, res, shape):
    """-> (int32 [n], status): fp64 quotient, truncated; a point off the grid sets STATUS_OFF_GRID (cell 0)."""
    t0 = (pc[:, dims[0]].astype(np.float64) - float(lo[0])) / float(res[0])
    t1 = (pc[:, dims[1]].astype(np.float64) - float(lo[1])) / float(res[1])
    ok = (t0 > -1.0) & (t0 < float(shape[0])) & (t1 > -1.0) & (t1 < float(shape[1]))
    cell = np.where(ok, np.where(ok, t0, 0).astype(np.int64) * int(shape[1]) + np.where(ok, t1, 0).astype(np.int64), 0)
    return cell.astype(np.int32), (0 if ok.all() else STATUS_OFF_GRID)


def _home(v: np.ndarray, lo: float, h: float, g: int):
    t = np.floor((v.astype(np.float64) - lo) / h)
    inside = (t >= 0) & (t < g)
    with np.errstate(invalid="ignore"):
        c = np.where(t >= 0, np.where(t < g, t, g - 1), 0)
    return np.nan_to_num(c).astype(np.int64), inside


def grid_cells(xyz: np.ndarray, g: SearchGrid):
    cx, ix = _home(xyz[:, 0], g.lo[0], g.h, g.G[0])
    cy, iy = _home(xyz[:, 1], g.lo[1], g.h, g.G[1])
    cz, iz = _home(xyz[:, 2], g.lo[2], g.h, g.G[2])
    ok = ix & iy & iz
    cell = np.where(ok, (cz * g.G[1] + cy) * g.G[0] + cx, 0)
    return cell.astype(np.int32), (0 if ok.all() else STATUS_OFF_GRID)


def cells_build(cell: np.ndarray, ncell: int, order: np.ndarray = None):
    """-> (start int32 [ncell + 1], order int32 [n], status)."""
    n = cell.shape[0]
    if order is None:
        order = np.argsort(cell, kind="stable").astype(np.int32)
    status = 0
    o = order.astype(np.int64)
    if n and (o.min() < 0 or o.max() >= n):
        return np.zeros(ncell + 1, np.int32), order, STATUS_ORDER
    c = cell[o].astype(np.int64)
    if n and (c.min() < 0 or c.max() >= ncell):
        status |= STATUS_ORDER
    if n > 1 and not (((c[:-1] < c[1:]) | ((c[:-1] == c[1:]) & (o[:-1] < o[1:]))).all()):
        status |= STATUS_ORDER
    start = np.searchsorted(c, np.arange(ncell + 1), side="left").astype(np.int32)
    return start, order, status


def _search_one(xyz, start, order, g: SearchGrid, q, k: int, self_idx: int):
    n = xyz.shape[0]
    G = g.G
    lo = np.asarray(g.lo, np.float64)
    qd = q.astype(np.float64)
    hc = []
    for a in range(3):
        c, _ = _home(q[a:a + 1], g.lo[a], g.h, G[a])
        hc.append(int(c[0]))
    below = lo - qd
    above = qd - (lo + np.asarray(G, np.float64) * g.h)
    o = np.maximum(np.maximum(below, above), 0.0)
    outside2 = o * o
    best_d = np.zeros(0, np.float32)
    best_i = np.zeros(0, np.int64)
    gx, gy, gz = G
    for r in range(max(G)):
        if r > 0:
            L = np.inf
            for a in range(3):
                rest = outside2[(a + 1) % 3] + outside2[(a + 2) % 3]
                if hc[a] + r <= G[a] - 1:
                    gap = max((lo[a] + float(hc[a] + r) * g.h) - qd[a], 0.0)
                    L = min(L, gap * gap + rest)
                if hc[a] - r >= 0:
                    gap = max(qd[a] - (lo[a] + float(hc[a] - r + 1) * g.h), 0.0)
                    L = min(L, gap * gap + rest)
            if L == np.inf:
                break
            if best_d.shape[0] == k and float(best_d[-1]) < _SHRINK * L:
                break
        z0, z1 = max(hc[2] - r, 0), min(hc[2] + r, gz - 1)
        y0, y1 = max(hc[1] - r, 0), min(hc[1] + r, gy - 1)
        x0, x1 = max(hc[0] - r, 0), min(hc[0] + r, gx - 1)
        runs = []
        for z in range(z0, z1 + 1):
            for y in range(y0, y1 + 1):
                row = (z * gy + y) * gx
                if abs(z - hc[2]) == r or abs(y - hc[1]) == r:
                    runs.append((start[row + x0], start[row + x1 + 1]))
                else:
                    xa, xb = hc[0] - r, hc[0] + r
                    if xa >= 0:
                        runs.append((start[row + xa], start[row + xa + 1]))
                    if xb <= gx - 1:
                        runs.append((start[row + xb], start[row + xb + 1]))
        runs = [(max(int(a), 0), min(int(b), n)) for a, b in runs]             # clipped to [0, n), as the kernel clips them
        cand = [order[a:b] for a, b in runs if b > a]
        if not cand:
            continue
        idx = np.concatenate(cand).astype(np.int64)
        idx = idx[(idx >= 0) & (idx < n) & (idx != self_idx)]
        if idx.size == 0:
            continue
        d = xyz[idx, :3] - q[None, :3]                                   # fp32
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        all_d, all_i = np.concatenate([best_d, d2]), np.concatenate([best_i, idx])
        keep = np.lexsort((all_i, all_d))[:k]                            # by d2, ties to the lower index
        best_d, best_i = all_d[keep], all_i[keep]
    out = np.full(k, -1, np.int32)
    out[:best_i.shape[0]] = best_i
    return out


def knn(xyz: np.ndarray, start, order, g: SearchGrid, k: int) -> np.ndarray:
    """int32 [n, k]: the k nearest other points of every point by (d2 fp32, index), through the same shells as the kernel."""
    assert xyz.dtype == np.float32 and 1 <= k <= MAX_K and k < xyz.shape[0]
    return np.stack([_search_one(xyz, start, order, g, xyz[p, :3], k, p) for p in range(xyz.shape[0])])


def nearest(xyz: np.ndarray, start, order, g: SearchGrid, q: np.ndarray) -> np.ndarray:
    assert xyz.dtype == np.float32 and q.dtype == np.float32 and xyz.shape[0] >= 1
    if q.shape[0] == 0:
        return np.zeros(0, np.int32)
    return np.stack([_search_one(xyz, start, order, g, q[i, :3], 1, -1)[0] for i in range(q.shape[0])]).astype(np.int32)


def knn_brute(xyz: np.ndarray, q: np.ndarray, k: int, exclude_self: bool) -> np.ndarray:
    """The ordering rule with no search structure: every pair, sorted by (d2 fp32, index)."""
    out = np.empty((q.shape[0], k), np.int32)
    idx = np.arange(xyz.shape[0])
    for i in range(q.shape[0]):
        d = xyz[:, :3] - q[i:i + 1, :3]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        if exclude_self:
            d2 = d2.copy()
            d2[i] = np.inf
        out[i] = np.lexsort((idx, d2))[:k]
    return out


# ---- network pieces ---------------------------------------------------------------------------------------------------
def flatten_checked(tokens: np.ndarray, scale, shift, start, order, ncell: int):
    """-> (grid fp32 [ncell, C], status).  A range of `start` that is reversed or leaves [0, n] is clipped and an entry of
    `order` outside [0, n) is skipped (it is not counted either); both set STATUS_INDEX, as pw_flatten does."""
    n, C = tokens.shape
    t = tokens * scale[None].astype(_F) + shift[None].astype(_F)
    a, b = start[:ncell].astype(np.int64), start[1:ncell + 1].astype(np.int64)
    bad = bool(((a < 0) | (b > n) | (a > b)).any())
    a, b = np.maximum(a, 0), np.minimum(b, n)
    length = np.maximum(b - a, 0)
    cnt = np.zeros(ncell, np.int64)
    total = np.zeros((ncell, C), np.float32)
    for i in range(int(length.max()) if ncell else 0):
        cells = np.nonzero(length > i)[0]
        p = order[a[cells] + i].astype(np.int64)
        ok = (p >= 0) & (p < n)
        bad |= not ok.all()
        cells, p = cells[ok], p[ok]
        total[cells] = total[cells] + t[p]
        cnt[cells] += 1
    w = _F(1.0) / (cnt.astype(np.float32) + _F(1e-6))
    grid = np.where(cnt[:, None] > 0, total * w[:, None], _F(0.0)).astype(np.float32)
    return grid, (STATUS_INDEX if bad else 0)


def flatten(tokens: np.ndarray, scale, shift, start, order, ncell: int) -> np.ndarray:
    return flatten_checked(tokens, scale, shift, start, order, ncell)[0]


def dwconv3x3(grid: np.ndarray, H: int, W: int, w: np.ndarray, bias: np.ndarray, relu: bool) -> np.ndarray:
    """grid fp32 [H*W, C] or [H, W, C], w fp32 [9, C] (tap (dy+1)*3 + (dx+1)), bias [C]."""
    C = grid.shape[-1]
    g = grid.reshape(H, W, C)
    pad = np.zeros((H + 2, W + 2, C), np.float32)
    pad[1:-1, 1:-1] = g
    acc = np.zeros((H, W, C), np.float32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + w[dy * 3 + dx][None, None] * pad[dy:dy + H, dx:dx + W]
    acc = acc + bias[None, None].astype(_F)
    if relu:
        acc = np.where(acc > 0, acc, _F(0.0))
    return acc.reshape(grid.shape).astype(np.float32)


def inflate_checked(tokens: np.ndarray, scale, grid: np.ndarray, cell):
    """-> (out fp32 [n, C], status).  A cell outside [0, ncell) leaves out[p] = tokens[p] and sets STATUS_INDEX."""
    c = np.asarray(cell).astype(np.int64)
    ok = (c >= 0) & (c < grid.shape[0])
    if grid.shape[0] == 0:
        return tokens.copy(), (0 if ok.all() else STATUS_INDEX)
    out = np.where(ok[:, None], tokens + scale[None].astype(_F) * grid[np.where(ok, c, 0)], tokens).astype(np.float32)
    return out, (0 if ok.all() else STATUS_INDEX)


def inflate(tokens: np.ndarray, scale, grid: np.ndarray, cell) -> np.ndarray:
    return inflate_checked(tokens, scale, grid, cell)[0]


def neigh_rows_checked(feat: np.ndarray, knn_idx: np.ndarray, p0: int, np_: int, A: np.ndarray, b: np.ndarray):
    """-> (fp32 [np * k, C], status).  A neighbour outside [0, n) counts as the point itself (every difference is 0) and sets
    STATUS_INDEX."""
    k, F = knn_idx.shape[1], feat.shape[1]
    nb = knn_idx[p0:p0 + np_].reshape(-1).astype(np.int64)
    me = np.repeat(np.arange(p0, p0 + np_), k)
    ok = (nb >= 0) & (nb < feat.shape[0])
    nb = np.where(ok, nb, me)
    d = feat[nb] - feat[me]
    acc = np.broadcast_to(b[None].astype(_F), (nb.shape[0], A.shape[1])).copy()
    for f in range(F):
        acc = acc + A[f][None] * d[:, f:f + 1]
    return np.where(acc > 0, acc, _F(0.0)).astype(np.float32), (0 if ok.all() else STATUS_INDEX)


def neigh_rows(feat: np.ndarray, knn_idx: np.ndarray, p0: int, np_: int, A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """-> fp32 [np * k, C]."""
    return neigh_rows_checked(feat, knn_idx, p0, np_, A, b)[0]


def group_max(rows: np.ndarray, np_: int, k: int) -> np.ndarray:
    return rows.reshape(np_, k, -1).max(axis=1)


# ---- the network in plain torch ---------------------------------------------------------------------------------------
def forward(net, feat, cells, knn_idx):
    """`net` = `pasco_amd.waffle.net.WaffleNet`; feat [N, F], cells = list of (cell int [N], (H, W)) per grid, knn_idx [N, k]
    -> (embedding [N, C], tokens [N, C], logits [N, classes]).  One vote, no padding: the reference's modules written for
    batch 1 on channels-last rows, with torch's own kernels and nothing folded."""
    import torch
    import torch.nn.functional as Fn
    m = net.modules_
    e = m.embed
    N = feat.shape[0]
    x = Fn.batch_norm(feat, e.norm.running_mean, e.norm.running_var, e.norm.weight, e.norm.bias, False, 0.0, e.norm.eps)
    point = Fn.linear(x, e.conv1.weight[:, :, 0], e.conv1.bias)
    idx = knn_idx.long()
    d = x[idx] - x[:, None, :]                                            # [N, k, F]
    bn1, lin1, bn2, lin2 = e.conv2[0], e.conv2[1], e.conv2[2], e.conv2[4]
    d = Fn.batch_norm(d.reshape(-1, d.shape[-1]), bn1.running_mean, bn1.running_var, bn1.weight, bn1.bias, False, 0.0, bn1.eps)
    d = Fn.linear(d, lin1.weight[:, :, 0, 0])
    d = torch.relu(Fn.batch_norm(d, bn2.running_mean, bn2.running_var, bn2.weight, bn2.bias, False, 0.0, bn2.eps))
    d = Fn.linear(d, lin2.weight[:, :, 0, 0]).reshape(N, idx.shape[1], -1).amax(dim=1)
    emb = Fn.linear(torch.cat((point, d), dim=1), e.final.weight[:, :, 0], e.final.bias)
    tokens = emb
    C = emb.shape[1]
    counts = []
    for cell, (H, W) in cells:
        counts.append(torch.zeros(H * W, dtype=torch.float32, device=feat.device).index_add_(
            0, cell.long(), torch.ones(N, dtype=torch.float32, device=feat.device)))
    for dpt, (sm, cm) in enumerate(zip(m.waffleiron.spatial_mix, m.waffleiron.channel_mix)):
        cell, (H, W) = cells[dpt % len(cells)]
        cnt = counts[dpt % len(cells)]
        r = Fn.batch_norm(tokens, sm.norm.running_mean, sm.norm.running_var, sm.norm.weight, sm.norm.bias, False, 0.0,
                          sm.norm.eps)
        g = torch.zeros((H * W, C), dtype=torch.float32, device=feat.device).index_add_(0, cell.long(), r)
        g = g * (1.0 / (cnt + 1e-6))[:, None]
        g = g.reshape(H, W, C).permute(2, 0, 1)[None]
        g = sm.ffn[2](torch.relu(sm.ffn[0](g)))
        g = g[0].permute(1, 2, 0).reshape(H * W, C)
        tokens = tokens + sm.scale.weight[:, 0, 0][None] * g[cell.long()]
        r = Fn.batch_norm(tokens, cm.norm.running_mean, cm.norm.running_var, cm.norm.weight, cm.norm.bias, False, 0.0,
                          cm.norm.eps)
        r = torch.relu(Fn.linear(r, cm.mlp[0].weight[:, :, 0], cm.mlp[0].bias))
        r = Fn.linear(r, cm.mlp[2].weight[:, :, 0], cm.mlp[2].bias)
        tokens = tokens + cm.scale.weight[:, 0, 0][None] * r
    logits = Fn.linear(tokens, m.classif.weight[:, :, 0], m.classif.bias)
    return emb, tokens, logits
