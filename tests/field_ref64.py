"""Test helper: independent references of the point <-> voxel operators (include/pasco_field.h) - literal loops and fp64
formulas on the CPU, written from the header's text, sharing no code with pasco_amd/grad/host.py or the kernels."""
import math

import torch

U = 2.0 ** -24
CORNERS = 8


def group_ref(keys: torch.Tensor, n_seg: int):
    """-> (offsets int64 [n_seg + 1], list of the present indices in stable key order)."""
    k = keys.cpu().long()
    present = (k >= 0) & (k < n_seg)
    idx = torch.arange(k.numel())[present]
    order = torch.sort(k[present], stable=True).indices
    counts = torch.bincount(k[present], minlength=n_seg) if n_seg else torch.zeros(0, dtype=torch.int64)
    offsets = torch.zeros(n_seg + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    return offsets, idx[order]


def members_of(keys: torch.Tensor, n_seg: int):
    """list over segments of the list entries with that key, ascending."""
    k = keys.cpu().tolist()
    out = [[] for _ in range(n_seg)]
    for i, s in enumerate(k):
        if 0 <= s < n_seg:
            out[s].append(i)
    return out


def seg_sum_ref(x: torch.Tensor, members, w=None, src_mod=None):
    """-> (sum fp64 [n_seg, c], sum of |w x| fp64 [n_seg, c], count fp64 [n_seg]) from fp64 copies of the operands."""
    x64 = x.detach().cpu().double()
    w64 = None if w is None else w.detach().cpu().double()
    c = x64.shape[1]
    out = torch.zeros((len(members), c), dtype=torch.float64)
    mag = torch.zeros_like(out)
    cnt = torch.zeros(len(members), dtype=torch.float64)
    for s, js in enumerate(members):
        cnt[s] = len(js)
        for j in js:
            row = j if src_mod is None else j % src_mod
            term = x64[row] if w64 is None else w64[j] * x64[row]
            out[s] += term
            mag[s] += term.abs()
    return out, mag, cnt


def seg_max_loop(x: torch.Tensor, members, src_mod=None):
    """The maximum and its arg by the header's words: the first member, in list order, whose value equals the maximum; -1 and a
    zero for an empty segment, -1 and NaN for a NaN among the members.  -> (out in x's dtype, arg int32)."""
    xc = x.detach().cpu()
    c = xc.shape[1]
    out = torch.zeros((len(members), c), dtype=xc.dtype)
    arg = torch.full((len(members), c), -1, dtype=torch.int32)
    for s, js in enumerate(members):
        for ch in range(c):
            best, at, nan = None, -1, False
            for j in js:
                v = xc[j if src_mod is None else j % src_mod, ch]
                if math.isnan(float(v)):
                    nan, best = True, v
                    break
                if best is None or float(v) > float(best):
                    best, at = v, j
            if best is not None:
                out[s, ch] = best
                arg[s, ch] = -1 if nan else at
    return out, arg


def interp_ref(points: torch.Tensor, voxels: torch.Tensor, ts: int):
    """points [m, 4] (their own precision, taken to fp64 exactly), voxels int [n, 4] = the map's rows -> (rows int32 [8, m],
    weights fp64 [8, m]): a literal loop over the eight corners.  A corner of weight 0 and every corner of a point with a
    non-finite coordinate are absent; the weights are not renormalised."""
    table = {tuple(v): i for i, v in enumerate(voxels.cpu().tolist())}
    p = points.detach().cpu().double()
    m = p.shape[0]
    rows = torch.full((CORNERS, m), -1, dtype=torch.int32)
    weights = torch.zeros((CORNERS, m), dtype=torch.float64)
    for i in range(m):
        b, xyz = float(p[i, 0]), [float(v) for v in p[i, 1:]]
        if not all(math.isfinite(v) for v in [b] + xyz):
            continue
        lower = [math.floor(v / ts) * ts for v in xyz]
        for k in range(CORNERS):
            o = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
            corner = [lower[d] + o[d] * ts for d in range(3)]
            wk = 1.0
            for d in range(3):
                wk *= 1.0 - abs(xyz[d] - corner[d]) / ts
            weights[k, i] = wk
            if wk != 0.0:
                rows[k, i] = table.get((int(math.floor(b)), *[int(v) for v in corner]), -1)
    return rows, weights


def interp_fwd_ref(x: torch.Tensor, rows: torch.Tensor, weights64: torch.Tensor):
    """-> (out fp64 [m, c], sum_k |w_k x_k| fp64 [m, c]) over the present corners."""
    x64 = x.detach().cpu().double()
    m = rows.shape[1]
    out = torch.zeros((m, x64.shape[1]), dtype=torch.float64)
    mag = torch.zeros_like(out)
    r = rows.cpu().long()
    for k in range(CORNERS):
        have = (r[k] >= 0) & (r[k] < x64.shape[0])
        term = torch.where(have[:, None], weights64[k][:, None] * x64[r[k].clamp(0, max(x64.shape[0] - 1, 0))], torch.zeros_like(out))
        out += term
        mag += term.abs()
    return out, mag


def dense_quantise(feats: torch.Tensor, coords: torch.Tensor, ts: int, mode: str):
    """The dense fp64 twin of `TensorField.sparse()`: points into a grid by floor(c / ts), `index_add_` / `bincount` (`amax` for
    the maximum) -> dict voxel coordinate tuple -> fp64 row."""
    f = feats.detach().cpu().double()
    c = coords.detach().cpu().double()
    vox = torch.cat([torch.floor(c[:, :1]), torch.floor(c[:, 1:] / ts) * ts], dim=1).long()
    lo = vox.min(dim=0).values
    ext = (vox.max(dim=0).values - lo + 1).tolist()
    rel = vox - lo
    cell = ((rel[:, 0] * ext[1] + rel[:, 1]) * ext[2] + rel[:, 2]) * ext[3] + rel[:, 3]
    cells = ext[0] * ext[1] * ext[2] * ext[3]
    cnt = torch.bincount(cell, minlength=cells).double()
    if mode == "max":
        grid = torch.full((cells, f.shape[1]), float("-inf"), dtype=torch.float64).scatter_reduce(
            0, cell[:, None].expand(-1, f.shape[1]), f, "amax", include_self=True)
    else:
        grid = torch.zeros((cells, f.shape[1]), dtype=torch.float64).index_add_(0, cell, f)
        if mode == "avg":
            grid = grid / cnt.clamp(min=1)[:, None]
    return {tuple(v): grid[ce] for v, ce in zip(vox.tolist(), cell.tolist())}, cnt[cell]
