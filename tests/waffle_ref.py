"""Literal references of the point-feature kernels (include/pasco_waffle.h) for tests/waffle_edge_cases.py.  Nothing here
imports pasco_amd.waffle.host: the searches are all-pairs, the CSR is one `np.nonzero` per cell, the voxel and cell formulas
are the reference's `Voxelize` and `get_occupied_2d_cells` written out, the float kernels are float64 loops, and the status
paths are written from the header's text: which term is skipped, which bit is set, what is written."""
import numpy as np

# include/pasco_waffle.h, restated as numbers (tests/test_waffle_cpu.py holds host.py's constants to the header)
MAX_K, MAX_FEAT = 32, 8
STATUS_OFF_GRID, STATUS_ORDER, STATUS_INDEX, STATUS_KEY_RANGE = 1, 2, 4, 8
KEY_BOUND = 1 << 21


# ---- searches -----------------------------------------------------------------------------------------------------------
def all_pairs(xyz, q, k, exclude_self, present=None):
    """int32 [m, k]: for every query the k nearest of the points with `present` (all when None) under the header's ordering
    rule - d2 = (dx*dx + dy*dy) + dz*dz in fp32 with d = point - query, smaller first, equal d2 to the lower index; the
    query's own index is left out when `exclude_self`.  A list that runs out of points ends in -1."""
    xyz = np.ascontiguousarray(xyz[:, :3], np.float32)
    q = np.ascontiguousarray(q[:, :3], np.float32)
    index = np.arange(xyz.shape[0])
    out = np.full((q.shape[0], k), -1, np.int32)
    for i in range(q.shape[0]):
        dx, dy, dz = (xyz[:, a] - q[i, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == np.float32
        take = np.ones(xyz.shape[0], bool) if present is None else present.copy()
        if exclude_self:
            take[i] = False
        cand = index[take]
        best = cand[np.lexsort((cand, d2[take]))][:k]
        out[i, :best.shape[0]] = best
    return out


def csr(cell, ncell):
    """(start int32 [ncell + 1], order int32 [n]): the points of cell c in ascending index, cell after cell."""
    start, order = np.zeros(ncell + 1, np.int32), []
    for c in range(ncell):
        members = np.nonzero(cell == c)[0]
        order.extend(members.tolist())
        start[c + 1] = start[c] + members.shape[0]
    return start, np.asarray(order, np.int32).reshape(-1)


def search_cell(xyz, lo, h, G):
    """Cell of every point on the search grid: floor((double)p - lo) / h) per axis, x fastest."""
    c = [np.floor((xyz[:, a].astype(np.float64) - lo[a]) / h).astype(np.int64) for a in range(3)]
    for a in range(3):
        assert (c[a] >= 0).all() and (c[a] < G[a]).all(), "a point outside the search grid"
    return ((c[2] * G[1] + c[1]) * G[0] + c[0]).astype(np.int32)


# ---- keys and cells -------------------------------------------------------------------------------------------------------
def voxel_keys(pc, voxel):
    """Voxelize: `((pc[:, :3] - pc[:, :3].min(0, keepdims=True)) / voxel).astype("int")` on fp32 points.  -> (key with every
    key outside [0, 2^21) written as 0, status)."""
    shift = pc[:, :3] - pc[:, :3].min(0, keepdims=True)
    quot = shift / np.float32(voxel)
    assert quot.dtype == np.float32
    ok = (quot >= 0) & (quot < KEY_BOUND)
    key = np.where(ok, quot, 0).astype("int")
    return key.astype(np.int32), (0 if ok.all() else STATUS_KEY_RANGE)


def cell_index(pc, dims, fov_lo, fov_hi, shape):
    """get_occupied_2d_cells: res = (hi - lo) / shape, quant = ((pc[:, dims] - lo) / res).astype("int"), cell = q0 * W + q1.
    The reference would index out of its grid where a quotient leaves (-1, shape): the header refuses those (cell 0, bit)."""
    dims = list(dims)
    lo, hi = np.asarray(fov_lo, np.float64)[dims], np.asarray(fov_hi, np.float64)[dims]
    res = (hi - lo) / np.array(shape)[None]
    t = (pc[:, dims] - lo) / res
    assert t.dtype == np.float64
    ok = ((t > -1.0) & (t < np.array(shape, np.float64)[None])).all(1)
    quant = np.where(ok[:, None], t, 0).astype("int")
    cell = np.where(ok, quant[:, 0] * shape[1] + quant[:, 1], 0)
    return cell.astype(np.int32), (0 if ok.all() else STATUS_OFF_GRID)


# ---- float kernels in float64 ---------------------------------------------------------------------------------------------
def flatten64(tokens, scale, shift, start, order, ncell):
    """-> (grid float64 [ncell, C], status).  Header: the mean over the points a cell lists; an index out of range is skipped
    (it is no term and it is not counted) and sets STATUS_INDEX; a range that is reversed or leaves [0, n] is clipped and
    sets it too."""
    n, C = tokens.shape
    t = tokens.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64)
    grid, status = np.zeros((ncell, C)), 0
    for c in range(ncell):
        a, b = int(start[c]), int(start[c + 1])
        if a < 0 or b > n or a > b:
            status |= STATUS_INDEX
        total, count = np.zeros(C), 0
        for s in range(max(a, 0), min(b, n)):
            p = int(order[s])
            if p < 0 or p >= n:
                status |= STATUS_INDEX
                continue
            total += t[p]
            count += 1
        if count:
            grid[c] = total / (count + 1e-6)
    return grid, status


def dwconv64(grid, H, W, w, bias, relu):
    """Depthwise 3 x 3 with zero padding, tap (dy + 1) * 3 + (dx + 1) reading in[y + dy, x + dx]."""
    C = grid.shape[-1]
    g = grid.reshape(H, W, C).astype(np.float64)
    out = np.zeros((H, W, C))
    for y in range(H):
        for x in range(W):
            acc = np.zeros(C)
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        acc += w[(dy + 1) * 3 + (dx + 1)].astype(np.float64) * g[y + dy, x + dx]
            out[y, x] = acc + bias.astype(np.float64)
    return (np.maximum(out, 0.0) if relu else out).reshape(H * W, C)


def inflate64(tokens, scale, grid, cell):
    """-> (out float64, status): tokens + scale * grid[cell]; a cell out of range leaves the row as it was, STATUS_INDEX."""
    out, status = tokens.astype(np.float64).copy(), 0
    for p in range(tokens.shape[0]):
        c = int(cell[p])
        if 0 <= c < grid.shape[0]:
            out[p] += scale.astype(np.float64) * grid[c].astype(np.float64)
        else:
            status |= STATUS_INDEX
    return out, status


def neigh_rows64(feat, knn, p0, np_, A, b):
    """-> (rows float64 [np * k, C], status): max(0, b + sum_f A[f] * (feat[nb, f] - feat[p, f])); a neighbour out of range
    counts as the point itself (every difference 0, the row is max(0, b)) and sets STATUS_INDEX."""
    n, k = feat.shape[0], knn.shape[1]
    f64, rows, status = feat.astype(np.float64), np.zeros((np_ * k, A.shape[1])), 0
    for p in range(p0, p0 + np_):
        for j in range(k):
            nb = int(knn[p, j])
            if nb < 0 or nb >= n:
                nb = p
                status |= STATUS_INDEX
            rows[(p - p0) * k + j] = np.maximum(b.astype(np.float64) + (f64[nb] - f64[p]) @ A.astype(np.float64), 0.0)
    return rows, status
