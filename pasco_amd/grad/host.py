"""Torch restatement of include/pasco_grad.h, include/pasco_rowgrad.h, include/pasco_pool.h, include/pasco_attngrad.h and include/pasco_norm.h for CPU tensors: index
operations and matrix products in the tensor's dtype.  The
CPU tests run on it and `pasco_amd.me.autograd` uses it where the features are not on a GPU.  Same results as the kernels up to
the order of the fp32 sums.  `knn_*` restates include/pasco_knn.h (the search by brute force under the header's ordering
rule: the same indices, the same fp32 d2 and weights).  The last section restates include/pasco_optim.h (`optim_*`): the optimiser step of
`pasco_amd.grad.optim.AdamW` on CPU parameters, the same bits as the kernels given the same sum of squares."""
from __future__ import annotations

import math

import torch


def nbr_invert(nbr: torch.Tensor, n_in: int) -> torch.Tensor:
    """nbr int32 [K, n_out] (-1 = none) -> inv int32 [K, n_in]: inv[k][nbr[k][o]] = o, -1 elsewhere.  Per offset the present
    neighbours must be distinct (include/pasco_grad.h)."""
    K, n_out = nbr.shape
    inv = torch.full((K, n_in), -1, dtype=torch.int32, device=nbr.device)
    if n_out == 0 or n_in == 0:
        return inv
    k, o = torch.nonzero((nbr >= 0) & (nbr < n_in), as_tuple=True)
    inv[k, nbr[k, o].long()] = o.to(torch.int32)
    return inv


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, nbr: torch.Tensor) -> torch.Tensor:
    """x [n_in, cin], dy [n_out, cout], nbr int32 [K, n_out] -> dw [K, cin, cout] = sum_o x[nbr[k][o]]^T dy[o]."""
    K, n_out = nbr.shape
    n_in, cin = x.shape
    cout = dy.shape[1]
    dw = torch.zeros((K, cin, cout), dtype=x.dtype, device=x.device)
    if n_out == 0 or n_in == 0:
        return dw
    for k in range(K):
        o = torch.nonzero((nbr[k] >= 0) & (nbr[k] < n_in)).reshape(-1)
        if o.numel():
            dw[k] = x[nbr[k, o].long()].t() @ dy[o]
    return dw


def colsum(dy: torch.Tensor) -> torch.Tensor:
    """dy [n, c] -> [c]."""
    return dy.sum(dim=0)


# ---- include/pasco_rowgrad.h ------------------------------------------------------------------------------------------------
def _dense_sites(coords: torch.Tensor, min3, ts: int, dims4, wrap: bool):
    """coords int [n, 4] -> (ok bool [n], b, x, y, z int64 [n]): the site of every row by ph_to_dense's rule (`wrap`: an index in
    [-dim, 0) wraps) or ph_dense_gather's (min 0, ts 1, no wrap); ok = the forward does not skip the row."""
    c = coords.long()
    dims = [int(v) for v in dims4]
    ok = (c[:, 0] >= 0) & (c[:, 0] < dims[0])
    idx = [c[:, 0]]
    for a in range(3):
        v = torch.div(c[:, 1 + a] - int(min3[a]), int(ts), rounding_mode="floor")
        if wrap:
            v = torch.where(v < 0, v + dims[1 + a], v)
        ok = ok & (v >= 0) & (v < dims[1 + a])
        idx.append(v)
    return (ok, *idx)


def dense_rows(dense: torch.Tensor, coords: torch.Tensor, min3, ts: int) -> torch.Tensor:
    """dense [B, C, X, Y, Z], coords int32 [n, 4] -> rows [n, C] = dense[b_i, :, site(i)], zero rows where the forward skips."""
    B, C, X, Y, Z = dense.shape
    ok, b, x, y, z = _dense_sites(coords, min3, ts, (B, X, Y, Z), True)
    rows = torch.zeros((coords.shape[0], C), dtype=dense.dtype, device=dense.device)
    if bool(ok.any()):
        rows[ok] = dense[b[ok], :, x[ok], y[ok], z[ok]]
    return rows


def rows_dense(rows: torch.Tensor, site_coords: torch.Tensor, shape5) -> torch.Tensor:
    """rows [n, C], site_coords int32 [n, 4] (distinct in-range sites) -> dense of `shape5`, zero except rows[i] at row i's site."""
    B, C, X, Y, Z = (int(v) for v in shape5)
    ok, b, x, y, z = _dense_sites(site_coords, (0, 0, 0), 1, (B, X, Y, Z), False)
    dense = torch.zeros((B, C, X, Y, Z), dtype=rows.dtype, device=rows.device)
    if bool(ok.any()):
        dense[b[ok], :, x[ok], y[ok], z[ok]] = rows[ok]
    return dense


def maxpool_arg(x: torch.Tensor, nbr: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """x [n_in, C], nbr int32 [K, n_out], out [n_out, C] -> arg int32 [n_out, C]: the input row of the first offset (ascending k)
    whose value == out, -1 where there is none."""
    K, n_out = nbr.shape
    n_in = x.shape[0]
    arg = torch.full(out.shape, -1, dtype=torch.int32, device=x.device)
    for k in range(K - 1, -1, -1):                # descending, so the smallest k is written last
        r = nbr[k].long()
        have = (r >= 0) & (r < n_in)
        hit = have[:, None] & (x[r.clamp(0, max(n_in - 1, 0))] == out) if n_in else torch.zeros_like(out, dtype=torch.bool)
        arg = torch.where(hit, nbr[k][:, None].expand_as(arg), arg)
    return arg


def maxpool_bwd(dy: torch.Tensor, arg: torch.Tensor, inv: torch.Tensor, n_in: int) -> torch.Tensor:
    """dy [n_out, C], arg int32 [n_out, C], inv int32 [K, n_in] -> dx [n_in, C]: terms added in ascending k."""
    n_out, C = dy.shape
    dx = torch.zeros((n_in, C), dtype=dy.dtype, device=dy.device)
    if n_in == 0 or n_out == 0:
        return dx
    rows = torch.arange(n_in, device=dy.device, dtype=arg.dtype)[:, None]
    for k in range(inv.shape[0]):
        o = inv[k].long()
        have = (o >= 0) & (o < n_out)
        oc = o.clamp(0, n_out - 1)
        dx = dx + torch.where(have[:, None] & (arg[oc] == rows), dy[oc], torch.zeros_like(dx))
    return dx


# ---- include/pasco_pool.h ---------------------------------------------------------------------------------------------------
POOL_SUM, POOL_AVG, POOL_MAX = 0, 1, 2
POOL_BC_ADD, POOL_BC_MUL, POOL_BC_CAT, POOL_BC_COPY = 0, 1, 2, 3


def _batch_rows(coords: torch.Tensor, B: int):
    """-> (in range bool [n], batch index int64 [n] clamped into [0, B))."""
    b = coords[:, 0].long()
    return (b >= 0) & (b < B), b.clamp(0, B - 1)


def pool_seg_reduce(x: torch.Tensor, coords: torch.Tensor, B: int, mode: int):
    """pp_seg_reduce in torch, in the dtype of `x`: x [n, c], coords int32 [n, 4] -> (out [B, c], count [B], arg int32 [B, c] |
    None).  A batch index without rows gives a zero row; the max's arg is the first row whose value == the maximum, -1 for an
    empty segment or a NaN maximum."""
    n, c = x.shape
    ok, b = _batch_rows(coords, B)
    count = torch.zeros(B, dtype=x.dtype, device=x.device).index_add_(0, b[ok], torch.ones(int(ok.sum()), dtype=x.dtype, device=x.device))
    if mode != POOL_MAX:
        out = torch.zeros((B, c), dtype=x.dtype, device=x.device).index_add_(0, b[ok], x[ok])
        if mode == POOL_AVG:
            out = torch.where(count[:, None] > 0, out / count.clamp(min=1)[:, None], out)
        return out, count, None
    out = torch.zeros((B, c), dtype=x.dtype, device=x.device)
    arg = torch.full((B, c), -1, dtype=torch.int32, device=x.device)
    rows = torch.arange(n, device=x.device)
    for s in range(B):
        sel = rows[ok & (b == s)]
        if sel.numel() == 0:
            continue
        seg = x[sel]
        nan = torch.isnan(seg).any(dim=0)
        m = torch.where(nan, torch.full_like(seg[0], float("nan")), torch.nan_to_num(seg, nan=float("-inf")).max(dim=0).values)
        hit = seg == m                                        # nothing equals a NaN
        first = torch.where(hit.any(dim=0), hit.to(torch.int64).argmax(dim=0), torch.zeros(c, dtype=torch.int64, device=x.device))
        arg[s] = torch.where(hit.any(dim=0), sel[first], torch.full_like(first, -1)).to(torch.int32)
        out[s] = torch.where(nan, m, seg.gather(0, first[None, :])[0])       # the first row's bits (+0 against -0)
    return out, count, arg


def pool_seg_max_bwd(dy: torch.Tensor, arg: torch.Tensor, n: int) -> torch.Tensor:
    """pp_seg_max_bwd in torch: dy [B, c], arg int32 [B, c] -> dx [n, c], dy[b][ch] stored at row arg[b][ch]."""
    B, c = dy.shape
    dx = torch.zeros((n, c), dtype=dy.dtype, device=dy.device)
    ok = (arg >= 0) & (arg < n)
    ch = torch.arange(c, device=dy.device)[None, :].expand(B, c)
    dx[arg.long()[ok], ch[ok]] = dy[ok]
    return dx


def pool_broadcast(x, g: torch.Tensor, coords: torch.Tensor, mode: int, cnt=None) -> torch.Tensor:
    """pp_broadcast in torch: x [n, c] (None for copy), g [B, cg] -> x + v | x * v | cat(x, v) | v with v = g[b_i] (divided by
    cnt[b_i] where `cnt` is given); a batch index outside [0, B) gives a zero output row."""
    ok, b = _batch_rows(coords, g.shape[0])
    v = g if cnt is None else torch.where(cnt[:, None] > 0, g / cnt.clamp(min=1)[:, None], torch.zeros_like(g))
    v = v[b]
    out = {POOL_BC_ADD: lambda: x + v, POOL_BC_MUL: lambda: x * v, POOL_BC_CAT: lambda: torch.cat([x, v], dim=1),
           POOL_BC_COPY: lambda: v}[mode]()
    return torch.where(ok[:, None], out, torch.zeros_like(out))


def pool_broadcast_mul_bwd(dy, x, g, coords, need_x: bool = True, need_g: bool = True):
    """pp_broadcast_mul_bwd in torch: -> (dx = dy * g[b_i] | None, dg[b] = sum dy * x | None)."""
    ok, b = _batch_rows(coords, g.shape[0])
    dx = torch.where(ok[:, None], dy * g[b], torch.zeros_like(dy)) if need_x else None
    dg = torch.zeros_like(g).index_add_(0, b[ok], (dy * x)[ok]) if need_g else None
    return dx, dg


def _window_rows(table: torch.Tensor, k: int, n_src: int):
    r = table[k].long()
    return (r >= 0) & (r < n_src), r.clamp(0, max(n_src - 1, 0))


def pool_pool(x: torch.Tensor, nbr: torch.Tensor, mode: int):
    """pp_pool in torch: x [n_in, c], nbr int32 [K, n_out] -> (out [n_out, c], cnt [n_out]); terms added in ascending k; the
    average divides by the number of PRESENT neighbours; an empty window gives a zero row."""
    K, n_out = nbr.shape
    n_in, c = x.shape
    out = torch.zeros((n_out, c), dtype=x.dtype, device=x.device)
    cnt = torch.zeros(n_out, dtype=x.dtype, device=x.device)
    if n_in:
        for k in range(K):
            have, r = _window_rows(nbr, k, n_in)
            out = out + torch.where(have[:, None], x[r], torch.zeros_like(out))
            cnt = cnt + have.to(x.dtype)
    if mode == POOL_AVG:
        out = torch.where(cnt[:, None] > 0, out / cnt.clamp(min=1)[:, None], out)
    return out, cnt


def pool_pool_bwd(dy: torch.Tensor, cnt, inv: torch.Tensor, n_in: int, mode: int) -> torch.Tensor:
    """pp_pool_bwd in torch: dy [n_out, c], cnt [n_out], inv int32 [K, n_in] -> dx [n_in, c], terms in ascending k, each
    dy[o] * (1 / cnt[o]) for the average."""
    n_out, c = dy.shape
    dx = torch.zeros((n_in, c), dtype=dy.dtype, device=dy.device)
    if n_out == 0 or n_in == 0:
        return dx
    if mode == POOL_AVG:
        dy = torch.where(cnt[:, None] > 0, dy * (1.0 / cnt.clamp(min=1))[:, None], torch.zeros_like(dy))
    for k in range(inv.shape[0]):
        have, o = _window_rows(inv, k, n_out)
        dx = dx + torch.where(have[:, None], dy[o], torch.zeros_like(dx))
    return dx


def pool_chconv_fwd(x: torch.Tensor, nbr: torch.Tensor, w: torch.Tensor, bias=None) -> torch.Tensor:
    """pp_chconv_fwd in torch: out[o][ch] = sum_k x[nbr[k][o]][ch] * w[k][ch] (+ bias[ch]), terms in ascending k."""
    K, n_out = nbr.shape
    n_in, c = x.shape
    out = torch.zeros((n_out, c), dtype=x.dtype, device=x.device)
    if n_in:
        for k in range(K):
            have, r = _window_rows(nbr, k, n_in)
            out = out + torch.where(have[:, None], x[r] * w[k], torch.zeros_like(out))
    return out if bias is None else out + bias.reshape(1, c)


def pool_chconv_wgrad(x: torch.Tensor, dy: torch.Tensor, nbr: torch.Tensor) -> torch.Tensor:
    """pp_chconv_wgrad in torch: dw[k][ch] = sum_o x[nbr[k][o]][ch] * dy[o][ch]."""
    K, n_out = nbr.shape
    n_in, c = x.shape
    dw = torch.zeros((K, c), dtype=x.dtype, device=x.device)
    if n_in and n_out:
        for k in range(K):
            have, r = _window_rows(nbr, k, n_in)
            dw[k] = torch.where(have[:, None], x[r] * dy, torch.zeros_like(dy)).sum(dim=0)
    return dw


# ---- include/pasco_field.h --------------------------------------------------------------------------------------------------
FIELD_SUM, FIELD_AVG, FIELD_MAX = 0, 1, 2
FIELD_CORNERS = 8


def field_group(keys: torch.Tensor, n_seg: int):
    """pq_group in torch: keys int32 [n] (absent: negative or >= n_seg) -> (offsets int32 [n_seg + 1], perm int32 [n]), the stable
    sort by key with the absent entries behind every segment."""
    n_seg = int(n_seg)
    k = keys.long()
    k = torch.where((k < 0) | (k >= n_seg), torch.full_like(k, n_seg), k)
    perm = torch.sort(k, stable=True).indices.to(torch.int32)
    counts = torch.bincount(k, minlength=n_seg + 1)[:n_seg]
    offsets = torch.zeros(n_seg + 1, dtype=torch.int64, device=keys.device)
    offsets[1:] = torch.cumsum(counts, dim=0)
    return offsets.to(torch.int32), perm


def _field_members(offsets: torch.Tensor, perm: torch.Tensor, n_src: int, src_mod):
    """-> (segment int64 [L], list entry int64 [L], source row int64 [L]) of the members that contribute, in list order."""
    n_seg, n_list = offsets.numel() - 1, perm.numel()
    src_mod = max(n_list, 1) if src_mod is None else int(src_mod)
    o = offsets.long().clamp(0, n_list)
    counts = (o[1:] - o[:-1]).clamp(min=0)
    seg = torch.repeat_interleave(torch.arange(n_seg, device=perm.device), counts)
    pos = o[:-1][seg] + (torch.arange(seg.numel(), device=perm.device) - (torch.cumsum(counts, 0) - counts)[seg])
    j = perm.long()[pos]
    row = j if src_mod >= n_list else j % src_mod
    ok = (j >= 0) & (j < n_list) & (row < n_src)
    return seg[ok], j[ok], row[ok], counts


def field_seg_rows(x: torch.Tensor, offsets: torch.Tensor, perm: torch.Tensor, mode: int, w=None, src_mod=None):
    """pq_seg_rows in torch, in the dtype of `x`: -> (out [n_seg, c], cnt [n_seg], arg int32 [n_seg, c] | None).  Member j of a
    segment reads row j % src_mod (j itself by default) and the weight w[j]; an empty segment gives a zero row; the max's arg is
    the first member, in list order, whose value == the maximum, -1 for an empty segment or a NaN maximum."""
    n_src, c = x.shape
    n_seg = offsets.numel() - 1
    seg, j, row, counts = _field_members(offsets, perm, n_src, src_mod)
    cnt = counts.to(x.dtype)
    if mode != FIELD_MAX:
        vals = x[row] if w is None else w.to(x.dtype)[j][:, None] * x[row]
        out = torch.zeros((n_seg, c), dtype=x.dtype, device=x.device).index_add_(0, seg, vals)
        if mode == FIELD_AVG:
            out = torch.where(cnt[:, None] > 0, out / cnt.clamp(min=1)[:, None], out)
        return out, cnt, None
    assert w is None, "the maximum takes no weights"
    vals = x[row]
    L = vals.shape[0]
    isn = torch.isnan(vals)
    ninf = torch.full_like(vals, float("-inf"))
    clean = torch.where(isn, ninf, vals)
    segc = seg[:, None].expand(L, c)
    nan_any = torch.zeros((n_seg, c), dtype=torch.int64, device=x.device).scatter_add_(0, segc, isn.long()) > 0
    m = torch.full((n_seg, c), float("-inf"), dtype=x.dtype, device=x.device).scatter_reduce(0, segc, clean, "amax", include_self=True)
    hit = (clean == m[seg]) & ~isn
    pos = torch.arange(L, device=x.device)[:, None].expand(L, c)
    first = torch.full((n_seg, c), L, dtype=torch.int64, device=x.device).scatter_reduce(
        0, segc, torch.where(hit, pos, torch.full_like(pos, L)), "amin", include_self=True)
    has = first < L
    fc = first.clamp(max=max(L - 1, 0))
    if L:
        picked, pj = vals.gather(0, fc), j[fc]
    else:
        picked, pj = torch.zeros((n_seg, c), dtype=x.dtype, device=x.device), torch.zeros((n_seg, c), dtype=torch.int64, device=x.device)
    out = torch.where(nan_any, torch.full_like(picked, float("nan")), torch.where(has, picked, torch.zeros_like(picked)))
    arg = torch.where(has & ~nan_any, pj, torch.full_like(pj, -1)).to(torch.int32)
    return out, cnt, arg


def field_seg_max_bwd(dy: torch.Tensor, arg: torch.Tensor, n_src: int, src_mod=None) -> torch.Tensor:
    """pq_seg_max_bwd in torch: dy [n_seg, c], arg int32 [n_seg, c] -> dx [n_src, c], dy[s][ch] stored at row arg[s][ch] % src_mod."""
    n_seg, c = dy.shape
    dx = torch.zeros((int(n_src), c), dtype=dy.dtype, device=dy.device)
    a = arg.long()
    row = a if src_mod is None else a % int(src_mod)
    ok = (a >= 0) & (row < n_src)
    ch = torch.arange(c, device=dy.device)[None, :].expand(n_seg, c)
    dx[row[ok], ch[ok]] = dy[ok]
    return dx


def field_gather_w(x: torch.Tensor, idx: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """pq_gather_w in torch: out[i] = x[idx[i]] * (1 / d[idx[i]]); a zero row where d == 0 or the index is outside [0, n_src)."""
    n_src = x.shape[0]
    i = idx.long()
    ok = (i >= 0) & (i < n_src)
    if n_src == 0:
        return torch.zeros((i.numel(), x.shape[1]), dtype=x.dtype, device=x.device)
    ic = i.clamp(0, n_src - 1)
    dv = d.to(x.dtype)[ic]
    ok = ok & (dv != 0)
    scale = 1.0 / torch.where(ok, dv, torch.ones_like(dv))
    return torch.where(ok[:, None], x[ic] * scale[:, None], torch.zeros((), dtype=x.dtype, device=x.device))


def field_interp_map(points: torch.Tensor, tkeys: torch.Tensor, tvals: torch.Tensor, ts: int):
    """pq_interp_map in torch, in the dtype of `points` [m, 4] = (b, x, y, z): -> (rows int32 [8, m], weights [8, m]).  Corner
    k = 4 ox + 2 oy + oz; weight (f_x f_y) f_z with f_d = 1 - |x_d - corner_d| / ts, not renormalised; a corner of weight 0 and
    every corner of a point with a non-finite coordinate are absent.  The table is probed by the backend that serves the
    tensors' device (`me.backend.backend_for`)."""
    from ..me.backend import backend_for
    m = points.shape[0]
    ts = int(ts)
    b, xyz = points[:, 0], points[:, 1:]
    fine = torch.isfinite(points).all(dim=1) & (b >= 0) & (b < 1024) & (xyz.abs() < 262144).all(dim=1)
    xyz = torch.where(fine[:, None], xyz, torch.zeros_like(xyz))
    lower = torch.floor(xyz / ts) * ts
    lower = torch.where(lower > xyz, lower - ts, lower)            # x * (1 / ts), torch's device quotient, can land on the next integer
    lower = torch.where(lower + ts <= xyz, lower + ts, lower)      # (lower + ts is exact; x - lower would round)
    f = torch.stack([((lower + ts) - xyz) / ts, (xyz - lower) / ts])          # [2, m, 3]: 1 - |x - corner| / ts, nothing cancels
    bi = torch.where(fine, torch.floor(b), torch.zeros_like(b)).to(torch.int32)
    rows = torch.full((FIELD_CORNERS, m), -1, dtype=torch.int32, device=points.device)
    weights = torch.zeros((FIELD_CORNERS, m), dtype=points.dtype, device=points.device)
    be = backend_for(points.device) if m else None
    for k in range(FIELD_CORNERS):
        o = ((k >> 2) & 1, (k >> 1) & 1, k & 1)
        wk = (f[o[0], :, 0] * f[o[1], :, 1]) * f[o[2], :, 2]
        wk = torch.where(fine, wk, torch.zeros_like(wk))
        weights[k] = wk
        if m:
            corner = lower.to(torch.int32) + torch.tensor(o, dtype=torch.int32, device=points.device) * ts
            found = be.map_find(torch.cat([bi[:, None], corner], dim=1).contiguous(), tkeys, tvals)
            rows[k] = torch.where(fine & (wk != 0), found, torch.full_like(found, -1))
    return rows, weights


def field_interp_fwd(x: torch.Tensor, rows: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """pq_interp_fwd in torch: out[p] = sum over the present corners, in ascending k, of weights[k][p] * x[rows[k][p]]."""
    n_in, c = x.shape
    m = rows.shape[1]
    out = torch.zeros((m, c), dtype=x.dtype, device=x.device)
    if n_in:
        for k in range(FIELD_CORNERS):
            have, r = _window_rows(rows, k, n_in)
            out = out + torch.where(have[:, None], weights[k].to(x.dtype)[:, None] * x[r], torch.zeros_like(out))
    return out


# ---- include/pasco_knn.h ----------------------------------------------------------------------------------------------------
KNN_MAX_K = 16                  # PK_MAX_K
KNN_PAIRS = 1 << 22             # (query, candidate) pairs of one chunk of the brute force


def knn_search(cand: torch.Tensor, q: torch.Tensor, k: int):
    """pk_knn in torch, in the dtype of `cand` [n, 3] / `q` [m, 3]: -> (idx int32 [k, m], d2 [k, m]), nearest first, by brute
    force under the header's ordering rule: d2 = (dx*dx + dy*dy) + dz*dz with d = cand - q, a smaller d2 is nearer, equal d2 goes
    to the lower candidate index (a stable sort along the candidates).  Fewer than k candidates leave idx = -1, d2 = +inf; a
    query with a non-finite coordinate has all k absent."""
    k = int(k)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError(f"k = {k}: 1 .. {KNN_MAX_K} neighbours are served")
    n, m = cand.shape[0], q.shape[0]
    idx = torch.full((k, m), -1, dtype=torch.int32, device=q.device)
    d2 = torch.full((k, m), float("inf"), dtype=cand.dtype, device=q.device)
    kk = min(k, n)
    if kk == 0 or m == 0:
        return idx, d2
    q = q.to(cand.dtype)
    step = max(1, KNN_PAIRS // n)
    for a in range(0, m, step):
        qa = q[a:a + step]
        d = cand[None, :, :3] - qa[:, None, :3]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        val, pos = torch.sort(dd, dim=1, stable=True)
        fine = torch.isfinite(qa[:, :3]).all(dim=1)
        idx[:kk, a:a + step] = torch.where(fine[None, :], pos[:, :kk].t().to(torch.int32), torch.full_like(idx[:kk, a:a + step], -1))
        d2[:kk, a:a + step] = torch.where(fine[None, :], val[:, :kk].t(), torch.full_like(d2[:kk, a:a + step], float("inf")))
    return idx, d2


def knn_weights(d2: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """pk_weights in torch, in the dtype of `d2` [k, m]: r_j = 1 / (d2_j + 1e-8) over the present entries (idx >= 0), the norm
    added in ascending j, w_j = r_j / norm; zero weights for an absent entry and where the norm is zero or not finite.  The
    constant is the fp32 nearest 1e-8 for fp32 rows (the kernel's), 1e-8 itself otherwise."""
    eps = torch.tensor(1e-8, dtype=d2.dtype, device=d2.device)
    present = idx >= 0
    r = torch.where(present, 1.0 / (torch.where(present, d2, torch.zeros_like(d2)) + eps), torch.zeros_like(d2))
    norm = torch.zeros_like(d2[0]) if d2.shape[0] else None
    for j in range(d2.shape[0]):
        norm = norm + r[j]
    if norm is None:
        return torch.zeros_like(d2)
    ok = present.any(dim=0) & (norm != 0) & torch.isfinite(norm)
    return torch.where(present & ok[None, :], r / torch.where(ok, norm, torch.ones_like(norm))[None, :], torch.zeros_like(d2))


def knn_interp(x: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """pk_interp_fwd in torch: out[p] = the sum over the entries with idx[j][p] in [0, n), in ascending j, of w[j][p] * x[idx[j][p]]."""
    n, c = x.shape
    k, m = idx.shape
    out = torch.zeros((m, c), dtype=x.dtype, device=x.device)
    if n:
        for j in range(k):
            have, r = _window_rows(idx, j, n)
            out = out + torch.where(have[:, None], w[j].to(x.dtype)[:, None] * x[r], torch.zeros_like(out))
    return out


def knn_interp_bwd(dy: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, n: int) -> torch.Tensor:
    """The backward of `knn_interp` with respect to x: the flattened [k, m] table grouped by candidate row (`field_group`), the
    terms w[j][p] * dy[p] of a row added in ascending (j, p) (`field_seg_rows`, src_mod = m)."""
    m = idx.shape[1]
    offsets, perm = field_group(idx.reshape(-1), int(n))
    return field_seg_rows(dy, offsets, perm, FIELD_SUM, w=w.reshape(-1), src_mod=max(m, 1))[0]


# ---- include/pasco_attngrad.h -----------------------------------------------------------------------------------------------
def _attn_allow(bits, any_, B: int, N: int, Q: int, device):
    """bits int32 [B, N, 4] | None, any int32 [B, 4] | None -> allow bool [B, Q, N] | None by the forward's rules: bit q of a
    key's word, and a query with no bit in `any` attends everywhere.  Bits at positions >= Q are never looked at."""
    if bits is None:
        return None
    qs = torch.arange(Q, device=device)
    word, shift = (qs >> 5), (qs & 31).to(torch.int32)
    allow = ((bits[:, :, word] >> shift) & 1).bool().transpose(1, 2)                    # [B, Q, N]
    if any_ is not None:
        allow = allow | ~((any_[:, word] >> shift) & 1).bool()[:, :, None]
    return allow


def attn_cross_bwd(q, k, v, bits, any_, out, dout, need_q: bool = True, need_k: bool = True, need_v: bool = True):
    """The backward of `attn_cross_fwd` (include/pasco_attngrad.h) in torch, fp32: q [B,H,Q,Dh] (pre-scaled), k / v [B,N,H*Dh],
    out / dout [B,Q,H*Dh] -> (dq, dk, dv), None where not needed.  One (b, h) at a time: P = softmax(q k^T + mask),
    delta = sum_d dout out, dV = P^T dout, dS = P (dout v^T - delta), dK = dS^T q, dQ = dS k.  A query with nothing allowed has
    P = 0 (zero output row, zero dq row)."""
    B, H, Q, Dh = q.shape
    N = k.shape[1]
    allow = _attn_allow(bits, any_, B, N, Q, q.device)
    dq = torch.zeros_like(q) if need_q else None
    dk = torch.zeros_like(k) if need_k else None
    dv = torch.zeros_like(v) if need_v else None
    for b in range(B):
        for h in range(H):
            sl = slice(h * Dh, (h + 1) * Dh)
            qq, kk, vv, do, o = q[b, h], k[b, :, sl], v[b, :, sl], dout[b, :, sl], out[b, :, sl]
            s = qq @ kk.t()                                                             # [Q, N]
            if allow is not None:
                s = s.masked_fill(~allow[b], float("-inf"))
            m = s.max(dim=1, keepdim=True).values
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            p = torch.exp(s - m)
            l = p.sum(dim=1, keepdim=True)
            p = p / torch.where(l > 0, l, torch.ones_like(l))
            delta = (do @ o.t()).diagonal()[:, None]      # by the product that forms do @ vv.t(): where out == v the two cancel exactly
            if need_v:
                dv[b, :, sl] = p.t() @ do
            if need_q or need_k:
                ds = p * (do @ vv.t() - delta)
                if need_k:
                    dk[b, :, sl] = ds.t() @ qq
                if need_q:
                    dq[b, h] = ds @ kk
    return dq, dk, dv


# ---- include/pasco_match.h --------------------------------------------------------------------------------------------------
def target_bits(tbits: torch.Tensor, t: int) -> torch.Tensor:
    """tbits int32 [N, 4] -> bool [N, T]: bit k of a row's 128-bit word.  Bits at positions >= T are never looked at."""
    ks = torch.arange(t, device=tbits.device)
    return ((tbits[:, ks >> 5] >> (ks & 31).to(torch.int32)) & 1).bool()


def target_pack(masks: torch.Tensor, unknown, coords: torch.Tensor, origin=(0, 0, 0)):
    """pm_target_pack in torch: masks uint8 [T,X,Y,Z], unknown uint8 [X,Y,Z] | None, coords int32 [N,4] -> (tbits int32 [N,4],
    flags uint8 [N], oob int32 [1])."""
    t, dx, dy, dz = masks.shape
    n = coords.shape[0]
    c = coords[:, 1:].long() - torch.as_tensor([int(o) for o in origin], dtype=torch.int64, device=coords.device)
    inside = ((c >= 0) & (c < torch.as_tensor([dx, dy, dz], device=coords.device))).all(dim=1)
    cc = torch.where(inside[:, None], c, torch.zeros_like(c))
    idx = (cc[:, 0] * dy + cc[:, 1]) * dz + cc[:, 2]
    tgt = (masks.reshape(t, -1)[:, idx] != 0).t() & inside[:, None]                     # [N, T]
    known = inside if unknown is None else inside & (unknown.reshape(-1)[idx] == 0)
    words = torch.zeros((n, 4), dtype=torch.int64, device=coords.device)
    for k in range(t):
        words[:, k >> 5] |= tgt[:, k].long() << (k & 31)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    flags = (known.to(torch.uint8) | ((known & tgt.any(dim=1)).to(torch.uint8) << 1)).to(torch.uint8)
    oob = (~inside).sum().to(torch.int32).reshape(1)
    return words, flags, oob


def _mask_terms(x: torch.Tensor):
    """-> (p, 1 - p, softplus(x), softplus(-x)), none of which overflows or cancels for a finite x."""
    e = torch.exp(-x.abs())
    inv = 1.0 / (1.0 + e)
    pos = x >= 0
    p = torch.where(pos, inv, e * inv)
    omp = torch.where(pos, e * inv, inv)
    l = torch.log1p(e)
    return p, omp, x.clamp(min=0) + l, (-x).clamp(min=0) + l


def pair_sums(logits: torch.Tensor, tbits: torch.Tensor, flags: torch.Tensor, flag_bit: int, t: int):
    """pm_pair_sums in torch, in the dtype of `logits`: -> (focal_sum [Q,T], dice [Q,T], stats [Q,T,3], count int32 [1]) over the
    rows whose flag bit `flag_bit` is set."""
    q = logits.shape[1]
    on = ((flags >> flag_bit) & 1).bool()
    x = logits[on]
    tgt = target_bits(tbits[on], t).to(logits.dtype)
    p, omp, sp, sn = _mask_terms(x)
    fp = 0.25 * omp * omp * sn
    fn = 0.75 * p * p * sp
    focal_sum = (fp - fn).t() @ tgt + fn.sum(dim=0)[:, None]
    inter = p.t() @ tgt
    psum = p.sum(dim=0)[:, None].expand(q, t)
    tsum = tgt.sum(dim=0)[None, :].expand(q, t)
    dice = 1 - (2 * inter + 1) / (psum + tsum + 1)
    stats = torch.stack([inter, psum, tsum], dim=2).contiguous()
    return focal_sum, dice, stats, on.sum().to(torch.int32).reshape(1)


def mask_loss_bwd(logits: torch.Tensor, tbits: torch.Tensor, flags: torch.Tensor, tgt_of_query: torch.Tensor,
                  coef: torch.Tensor, t: int) -> torch.Tensor:
    """pm_mask_loss_bwd in torch: dlogits [N,Q]; exactly 0 in unmatched columns and unknown rows."""
    matched = (tgt_of_query >= 0) & (tgt_of_query < t)
    known = (flags & 1).bool()
    y = torch.gather(target_bits(tbits, t), 1, tgt_of_query.clamp(0, t - 1).long()[None, :].expand(logits.shape[0], -1))
    p, omp, sp, sn = _mask_terms(logits)
    dfp = -0.25 * omp * omp * (2 * p * sn + omp)
    dfn = 0.75 * p * p * (2 * omp * sp + p)
    c, a, b = coef[:, 0][None, :], coef[:, 1][None, :], coef[:, 2][None, :]
    g = c * torch.where(y, dfp, dfn) + p * omp * torch.where(y, a + b, b)
    return torch.where(known[:, None] & matched[None, :], g, torch.zeros_like(g))


def assign(cost: torch.Tensor):
    """pm_assign in torch (the method of csrc/pm_assign.h): cost [Q,T] -> (row int64 [K], col int64 [K]), K = min(Q, T), rows
    ascending.  A non-finite cost is refused."""
    c = cost.detach().to(torch.float64).cpu()
    q, t = c.shape
    if q == 0 or t == 0:
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    if not bool(torch.isfinite(c).all()):
        raise RuntimeError(f"assign: the {q} x {t} cost matrix has a non-finite entry")
    tr = q > t
    if tr:
        c = c.t()
    n, m = c.shape
    inf = float("inf")
    u, v = torch.zeros(n + 1, dtype=torch.float64), torch.zeros(m + 1, dtype=torch.float64)
    p, way = [0] * (m + 1), [0] * (m + 1)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = torch.full((m + 1,), inf, dtype=torch.float64)
        used = torch.zeros(m + 1, dtype=torch.bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = c[i0 - 1] - u[i0] - v[1:]
            better = (cur < minv[1:]) & ~used[1:]
            minv[1:] = torch.where(better, cur, minv[1:])
            for j in torch.nonzero(better).flatten().tolist():
                way[j + 1] = j0
            free = torch.where(used[1:], torch.full_like(cur, inf), minv[1:])
            delta = float(free.min())
            j1 = int(torch.nonzero(free == delta)[0]) + 1           # the first minimum, as the C++ loop finds it
            for j in torch.nonzero(used).flatten().tolist():
                u[p[j]] += delta
                v[j] -= delta
            minv = torch.where(used, minv, minv - delta)
            j0 = j1
            if p[j0] == 0:
                break
        while j0 != 0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    pairs = sorted((j - 1, p[j] - 1) if tr else (p[j] - 1, j - 1) for j in range(1, m + 1) if p[j] != 0)
    return (torch.tensor([a for a, _ in pairs], dtype=torch.int64), torch.tensor([b for _, b in pairs], dtype=torch.int64))


SEM_IGNORE, SEM_OUTSIDE = 255, 254


def sem_rows_fwd(logits: torch.Tensor, coords: torch.Tensor, target: torch.Tensor, box: torch.Tensor, scale: int,
                 weights: torch.Tensor):
    """ps_rows_fwd in torch, in the dtype of `logits`: -> (label uint8 [N], ce [3] = (num / den, num, den), class_count int32 [C],
    info int32 [4] = (rows inside the box, label indices outside the grid, labels in C..254, 0), err [C, N]).  `box` = int [6],
    min_C then max_C, inclusive.  err_c = |[y == c] - p_c| for a row inside the box (1 - p_y as the sum of the other exponentials
    over the sum), 0 outside; its fp32 bit pattern is the sort key."""
    n, c = logits.shape
    xyz = coords[:, 1:4].long()
    lo, hi = box[:3].long(), box[3:].long()
    inside = ((xyz >= lo) & (xyz <= hi)).all(dim=1)
    idx = torch.div(xyz - lo, int(scale), rounding_mode="floor")
    dims = torch.tensor(target.shape, dtype=torch.long)
    in_grid = (idx < dims).all(dim=1) & inside
    idx = idx.clamp(min=0).minimum(dims - 1)
    raw = target[idx[:, 0], idx[:, 1], idx[:, 2]].long() if n else torch.zeros(0, dtype=torch.long)
    bad_label = in_grid & (raw >= c) & (raw != SEM_IGNORE)
    y = torch.where(in_grid & ~bad_label, raw, torch.full_like(raw, SEM_IGNORE))
    y = torch.where(inside, y, torch.full_like(y, SEM_OUTSIDE))
    m = logits.max(dim=1, keepdim=True).values if n else logits.new_zeros((0, 1))
    e = torch.exp(logits - m)
    fg = y[:, None] == torch.arange(c)[None, :]
    total = e.sum(dim=1, keepdim=True)
    others = torch.where(fg, torch.zeros_like(e), e).sum(dim=1, keepdim=True)
    err = torch.where(fg, others / total, e / total)
    err = torch.where(inside[:, None], err, torch.zeros_like(err)).t().contiguous()
    known = y < c
    w = weights.to(logits.dtype)[y.clamp(max=c - 1)]
    nll = (torch.log(total[:, 0]) + m[:, 0]) - torch.gather(logits, 1, y.clamp(max=c - 1)[:, None])[:, 0]
    zero = logits.new_zeros(())
    num = torch.where(known, w * nll, zero).sum()
    den = torch.where(known, w, zero).sum()
    ce = torch.stack([num / den, num, den])
    class_count = torch.bincount(y[known], minlength=c).to(torch.int32)
    info = torch.tensor([int(inside.sum()), int((inside & ~in_grid).sum()), int(bad_label.sum()), 0], dtype=torch.int32)
    return y.to(torch.uint8), ce, class_count, info, err


def sem_sort_desc(keys: torch.Tensor) -> torch.Tensor:
    """ps_sort_desc in torch: keys [S, M] (any ordered dtype) -> perm int32 [S, M], descending, equal keys in ascending index
    order."""
    return torch.sort(keys, dim=1, descending=True, stable=True).indices.to(torch.int32)


def sem_lovasz_fwd(perm: torch.Tensor, label: torch.Tensor, err: torch.Tensor, class_count: torch.Tensor):
    """ps_lovasz_fwd in torch, in the dtype of `err` [C, N]: -> (loss_c [C], coef [N, C], lovasz [1], present int32 [1]).  The
    increments are the closed form in integers (include/pasco_semloss.h), formed in fp64 and rounded once."""
    c, n = err.shape
    p = perm.long()
    lab = label.long()[p]                                   # [C, N] along the sorted order
    cls = torch.arange(c)[:, None]
    fg = lab == cls
    inside = lab != SEM_OUTSIDE
    g = class_count.long()[:, None]
    cf = fg.long().cumsum(dim=1)                            # inclusive
    i1 = inside.long().cumsum(dim=1)                        # i + 1 at a row inside the box
    u = (g + i1 - cf).double()
    inc = torch.where(fg, 1.0 / u, (g - cf).double() / ((u - 1.0) * u))
    live = inside & (g > 0)
    inc = torch.where(live, inc, torch.zeros_like(inc)).to(err.dtype)
    loss_c = (torch.gather(err, 1, p) * inc).sum(dim=1)
    coef_sorted = torch.where(fg, -inc, inc)
    coef = torch.zeros((c, n), dtype=err.dtype).scatter_(1, p, coef_sorted).t().contiguous()
    present = (class_count > 0).sum().to(torch.int32).reshape(1)
    lovasz = (loss_c.sum() / present.clamp(min=1).to(err.dtype)).reshape(1)
    return loss_c, coef, lovasz, present


def sem_loss_bwd(logits: torch.Tensor, label: torch.Tensor, coef: torch.Tensor, weights: torch.Tensor, ce: torch.Tensor,
                 present: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """ps_loss_bwd in torch: dlogits [N, C]; g [2] = the incoming gradients of (ce, lovasz).  A row labelled 254 is exactly 0."""
    n, c = logits.shape
    y = label.long()
    p = torch.softmax(logits, dim=1)
    known = y < c
    onehot = y[:, None] == torch.arange(c)[None, :]
    w = weights.to(logits.dtype)[y.clamp(max=c - 1)]
    gc = torch.where(known, g[0] * w / ce[2], torch.zeros_like(w))
    np_ = int(present)
    gl = g[1] / np_ if np_ > 0 else torch.zeros_like(g[1])
    d = gc[:, None] * (p - onehot.to(p.dtype)) + gl * p * (coef - (coef * p).sum(dim=1, keepdim=True))
    return torch.where((y != SEM_OUTSIDE)[:, None], d, torch.zeros_like(d)) + 0.0


# ---- include/pasco_norm.h ---------------------------------------------------------------------------------------------------
NORM_TILE_ROWS = 128            # PN_TILE_ROWS
ACT_NONE, ACT_RELU, ACT_LEAKY = 0, 1, 2


def norm_moments_merge(recs: torch.Tensor) -> torch.Tensor:
    """pn_moments_merge in torch: recs fp64 [r, 3, c] -> [3, c], the pairwise update in ascending r from (0, 0, 0); a record of
    count 0 is skipped (the first record with rows comes out as it is: w = 1, n = 0)."""
    r, _, c = recs.shape
    n = torch.zeros(c, dtype=torch.float64, device=recs.device)
    mean, m2 = n.clone(), n.clone()
    for i in range(r):
        nb, mb, qb = recs[i, 0], recs[i, 1], recs[i, 2]
        has = nb > 0
        tot = n + torch.where(has, nb, torch.zeros_like(nb))
        w = torch.where(has, nb / torch.where(has, tot, torch.ones_like(tot)), torch.zeros_like(nb))
        d = mb - mean
        mean, m2, n = torch.where(has, mean + d * w, mean), torch.where(has, (m2 + qb) + (d * d) * (n * w), m2), tot
    return torch.stack([n, mean, m2])


def norm_moments(x: torch.Tensor) -> torch.Tensor:
    """pn_moments in torch: x [n, c] -> fp64 [3, c]; one record per NORM_TILE_ROWS rows, M2 about the tile's own mean, merged in
    ascending tile order."""
    n, c = x.shape
    recs = []
    for r0 in range(0, n, NORM_TILE_ROWS):
        t = x[r0:r0 + NORM_TILE_ROWS].double()
        mean = t.sum(dim=0) / t.shape[0]
        recs.append(torch.stack([torch.full_like(mean, t.shape[0]), mean, (t - mean).square().sum(dim=0)]))
    return norm_moments_merge(torch.stack(recs) if recs else torch.zeros((0, 3, c), dtype=torch.float64, device=x.device))


def norm_finish(rec: torch.Tensor, eps: float, momentum: float, running_mean, running_var, dtype=torch.float32) -> torch.Tensor:
    """pn_finish in torch: rec fp64 [3, c] -> mean_rstd [2, c] in `dtype`; the running statistics move in place where count > 0."""
    n, mean, m2 = rec[0], rec[1], rec[2]
    has = n > 0
    var = torch.where(has, m2 / torch.where(has, n, torch.ones_like(n)), torch.zeros_like(m2))
    out = torch.stack([torch.where(has, mean, torch.zeros_like(mean)), 1.0 / torch.sqrt(var + eps)]).to(dtype)
    with torch.no_grad():
        if running_mean is not None:
            new = (1.0 - momentum) * running_mean.double() + momentum * mean
            running_mean.copy_(torch.where(has, new, running_mean.double()).to(running_mean.dtype))
        if running_var is not None:
            new = (1.0 - momentum) * running_var.double() + momentum * (m2 / torch.where(n > 1, n - 1, torch.ones_like(n)))
            running_var.copy_(torch.where(has, new, running_var.double()).to(running_var.dtype))
    return out


def _norm_z(x, mean_rstd, weight, bias):
    xh = (x - mean_rstd[0]) * mean_rstd[1]
    z = xh if weight is None else xh * weight
    return xh, (z if bias is None else z + bias)


def _norm_act_grad(z, act: int, slope: float):
    if act == ACT_RELU:
        return (z > 0).to(z.dtype)
    if act == ACT_LEAKY:
        return torch.where(z > 0, torch.ones_like(z), torch.full_like(z, slope))
    return torch.ones_like(z)


def norm_apply(x, mean_rstd, weight, bias, act: int, slope: float) -> torch.Tensor:
    """pn_apply in torch, in the dtype of `x`."""
    _, z = _norm_z(x, mean_rstd, weight, bias)
    if act == ACT_RELU:
        return torch.where(z > 0, z, torch.zeros_like(z))
    if act == ACT_LEAKY:
        return torch.where(z > 0, z, slope * z)
    return z


def norm_sums_merge(sums: torch.Tensor) -> torch.Tensor:
    """pn_sums_merge in torch: fp64 [r, 2, c] -> [2, c], added in ascending r."""
    out = torch.zeros(sums.shape[1:], dtype=torch.float64, device=sums.device)
    for i in range(sums.shape[0]):
        out = out + sums[i]
    return out


def norm_bwd_sums(dy, x, mean_rstd, weight, bias, act: int, slope: float) -> torch.Tensor:
    """pn_bwd_sums in torch: -> fp64 [2, c] = (sum g, sum g * xhat), per-tile partials added in ascending tile order."""
    n, c = x.shape
    xh, z = _norm_z(x, mean_rstd, weight, bias)
    g = dy * _norm_act_grad(z, act, slope)
    parts = [torch.stack([g[r0:r0 + NORM_TILE_ROWS].double().sum(dim=0),
                          (g[r0:r0 + NORM_TILE_ROWS].double() * xh[r0:r0 + NORM_TILE_ROWS].double()).sum(dim=0)])
             for r0 in range(0, n, NORM_TILE_ROWS)]
    return norm_sums_merge(torch.stack(parts) if parts else torch.zeros((0, 2, c), dtype=torch.float64, device=x.device))


def norm_bwd_dx(dy, x, mean_rstd, weight, bias, act: int, slope: float, total_sums, total_rec) -> torch.Tensor:
    """pn_bwd_dx in torch, in the dtype of `x`: weight * rstd * (g - S0 / N - xhat * S1 / N), N from `total_rec`."""
    xh, z = _norm_z(x, mean_rstd, weight, bias)
    g = dy * _norm_act_grad(z, act, slope)
    cnt = total_rec[0]
    inv = torch.where(cnt > 0, 1.0 / torch.where(cnt > 0, cnt, torch.ones_like(cnt)), torch.zeros_like(cnt))
    a0, a1 = (total_sums[0] * inv).to(x.dtype), (total_sums[1] * inv).to(x.dtype)
    ws = mean_rstd[1] if weight is None else weight * mean_rstd[1]
    return ws * ((g - a0) - xh * a1)


# ---- include/pasco_optim.h --------------------------------------------------------------------------------------------------
OPTIM_CHUNK = 4096              # PO_CHUNK
OPTIM_SCALARS = ("decay", "omb1", "b2", "omb2", "bc2sqrt", "eps", "neg_step", "unused")      # po_scalars


def _round_f32(x: float) -> float:
    """The fp64 value rounded once to fp32 (and held in a Python float again)."""
    return float(torch.tensor(x, dtype=torch.float64).to(torch.float32))


def optim_sqnorm(grads) -> torch.Tensor:
    """po_sqnorm in torch: fp64 [C], per OPTIM_CHUNK consecutive elements of each gradient the sum of its exact fp64 squares
    (the order inside a chunk is torch's, not the kernel's: the two agree to fp64 rounding)."""
    parts = []
    for g in grads:
        sq = g.reshape(-1).double().square()
        pad = -sq.numel() % OPTIM_CHUNK
        if pad:
            sq = torch.cat([sq, sq.new_zeros(pad)])
        parts.append(sq.view(-1, OPTIM_CHUNK).sum(dim=1))
    return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float64)


def optim_clip(sumsq: float, max_norm: float, grad_scale: float):
    """The fp64 expressions of po_prepare: -> (norm, s) with norm = grad_scale * sqrt(sumsq) and the clip scale
    s = (float)(min(max_norm / (norm + 1e-6), 1) * grad_scale), a NaN staying a NaN; max_norm <= 0 does not clip."""
    norm = grad_scale * (math.sqrt(sumsq) if sumsq == sumsq and sumsq >= 0 else float("nan"))
    c = 1.0
    if max_norm > 0.0:
        c = max_norm / (norm + 1e-6)
        if c >= 1.0:
            c = 1.0
    return norm, _round_f32(c * grad_scale)


def optim_scalars(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, beta1_pow: float,
                  beta2_pow: float) -> torch.Tensor:
    """The fp32 scalars of one tensor's update, fp32 [8] in the order of po_scalars, each formed in fp64 and rounded once;
    `beta*_pow` are the powers AFTER the step was counted."""
    bc2 = 1.0 - beta2_pow
    bc1 = 1.0 - beta1_pow
    vals = [1.0 - lr * weight_decay, 1.0 - beta1, beta2, 1.0 - beta2, math.sqrt(bc2) if bc2 >= 0 else float("nan"), eps,
            -lr / bc1 if bc1 != 0 else (float("-inf") if lr > 0 else float("nan")), 0.0]
    return torch.tensor(vals, dtype=torch.float64).to(torch.float32)


def optim_prepare(partials: torch.Tensor, table, hyper, max_norm: float, grad_scale: float, skip: bool, states: torch.Tensor,
                  scalars: torch.Tensor, result: torch.Tensor, step: torch.Tensor):
    """po_prepare in torch on host buffers laid out as the header's records: `table` = (group, state index) per tensor,
    `hyper` = (lr, beta1, beta2, eps, weight_decay) per group, states fp64 [P, 3] (the step an int64 in the first word),
    scalars fp32 [P, 8], result fp64 [3] (skipped an int64 in the third word), step int32 [2] (the clip an fp32 in the first)."""
    sumsq = 0.0
    for x in partials.tolist():
        sumsq += x
    finite = sumsq == sumsq and abs(sumsq) != float("inf")
    apply = finite or not skip
    norm, s = optim_clip(sumsq, max_norm, grad_scale)
    result[0], result[1] = sumsq, norm
    if not apply:
        result.view(torch.int64)[2] += 1
    step.view(torch.float32)[0] = s
    step[1] = int(apply)
    if not apply:
        return
    steps = states.view(torch.int64)
    for group, i in table:
        lr, b1, b2, eps, wd = (float(x) for x in hyper[group])
        steps[i, 0] += 1
        b1p, b2p = float(states[i, 1]) * b1, float(states[i, 2]) * b2
        states[i, 1], states[i, 2] = b1p, b2p
        scalars[i] = optim_scalars(lr, b1, b2, eps, wd, b1p, b2p)


def optim_adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, s: float, k: torch.Tensor):
    """po_adamw in torch on one tensor, IN PLACE on p, m, v, in their dtype: `s` the clip scale, `k` the eight scalars.  The
    order and the grouping are the header's; every torch op below rounds once, so on fp32 these are the kernel's bits."""
    k = k.to(p.dtype)
    decay, omb1, b2, omb2, bc2sqrt, eps, neg_step = (k[i] for i in range(7))
    with torch.no_grad():
        gs = g * torch.tensor(s, dtype=p.dtype)
        p.copy_(p * decay)
        m.copy_(m + (gs - m) * omb1)
        v.copy_(v * b2 + (gs * gs) * omb2)
        # the IEEE square root: torch's vectorised fp32 sqrt on the CPU is one ulp off it in ~0.6 % of elements, while the fp64
        # root rounded to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2 bits: the second rounding is innocuous)
        root = v.sqrt() if v.dtype == torch.float64 else v.double().sqrt().to(v.dtype)
        d = root / bc2sqrt + eps
        p.copy_(p + (m / d) * neg_step)
