"""Test helper: references of the dense <-> rows adjoints and of max pooling's backward (include/pasco_rowgrad.h), written from the
formulas with numpy index arithmetic and torch index operations, and the torch twins the autograd tests and the bottleneck-shaped
stack of tests/rowgrad_cases.py are held to.

The dense <-> rows kernels are copies: `torch.equal`, no tolerance.  Max pooling's backward adds up to K terms in fp32 in
ascending k:  |dx - dx64| <= (K - 1) * 2^-24 * sum |terms|, the bound of a sequential sum of K terms (K - 1 additions, each
rounded at no more than the running magnitude); with kernel == stride there is one term and the result is exact."""
import numpy as np
import torch
import torch.nn.functional as F

from tests.grad_ref64 import conv_twin

# the stack test: max |g - g64| <= ROW_STACK_M * max |g32 - g64| per gradient tensor, g32 / g64 = the torch twin in fp32 / fp64.
# Measured worst ratio over the eleven tensors (the error is a chain of fp32 sums in two different orders, tests/grad_ref64.py):
# 3.574 on the CPU (host restatement, the input features), 4.411 on the MI355X (c1.bias); asserted at 4 x the larger of the two.
ROW_STACK_M_MEASURED = {"cpu": 3.574, "mi355x": 4.411}
ROW_STACK_M = 4 * max(ROW_STACK_M_MEASURED.values())


def sites_of(coords, min3, ts, dims4):
    """coords int [n, 4] -> (ok bool [n], b, x, y, z int64 [n]) by ph_to_dense's rule: floor((coord - min) / ts) per axis, an index
    in [-dim, 0) wraps, ok = inside afterwards and the batch index in [0, B)."""
    c = coords.cpu().numpy().astype(np.int64)
    dims = np.asarray(dims4, dtype=np.int64)
    q = np.floor_divide(c[:, 1:] - np.asarray(min3, dtype=np.int64), int(ts))
    q = np.where(q < 0, q + dims[1:], q)
    ok = (c[:, 0] >= 0) & (c[:, 0] < dims[0]) & ((q >= 0) & (q < dims[1:])).all(axis=1)
    t = [torch.from_numpy(np.ascontiguousarray(v)) for v in (ok, c[:, 0], q[:, 0], q[:, 1], q[:, 2])]
    return tuple(v.to(coords.device) for v in t)


def dense_rows_ref(dense, coords, min3, ts):
    """rows[i] = dense[b_i, :, site(i)], zero rows where the forward skips the row."""
    B, C, X, Y, Z = dense.shape
    ok, b, x, y, z = sites_of(coords, min3, ts, (B, X, Y, Z))
    rows = torch.zeros((coords.shape[0], C), dtype=dense.dtype, device=dense.device)
    rows[ok] = dense[b[ok], :, x[ok], y[ok], z[ok]]
    return rows


def rows_dense_ref(rows, site_coords, shape5):
    """zeros of `shape5` with rows[i] stored at (b_i, :, x_i, y_i, z_i); rows with any index out of range are skipped."""
    B, C, X, Y, Z = shape5
    c = site_coords.long()
    ok = ((c >= 0) & (c < torch.tensor([B, X, Y, Z], device=c.device))).all(dim=1)
    dense = torch.zeros(tuple(shape5), dtype=rows.dtype, device=rows.device)
    dense[c[ok, 0], :, c[ok, 1], c[ok, 2], c[ok, 3]] = rows[ok]
    return dense


def maxpool_arg_loop(x, nbr, out):
    """Brute force: the input row of the first offset (ascending k) whose value == out[o][c]; -1 where there is none."""
    xs, nb, os_ = x.cpu().tolist(), nbr.cpu().tolist(), out.cpu().tolist()
    K, n_out, C = len(nb), out.shape[0], out.shape[1]
    arg = [[-1] * C for _ in range(n_out)]
    for o in range(n_out):
        for c in range(C):
            for k in range(K):
                r = nb[k][o]
                if r >= 0 and xs[r][c] == os_[o][c]:
                    arg[o][c] = r
                    break
    return torch.tensor(arg, dtype=torch.int32).reshape(n_out, C).to(x.device)


def maxpool_out_ref(x, nbr):
    """max over the present neighbours; 0 for an empty window (ph_maxpool_fwd)."""
    n_in = x.shape[0]
    xz = torch.cat([x, torch.full((1, x.shape[1]), float("-inf"), dtype=x.dtype, device=x.device)])
    nb = torch.where(nbr >= 0, nbr.long(), torch.full_like(nbr, n_in).long())
    m = xz[nb].max(dim=0).values
    return torch.where((nbr >= 0).any(dim=0)[:, None], m, torch.zeros_like(m))


def maxpool_bwd_ref(dy, arg, n_in, dtype):
    """dx[arg[o][c]][c] += dy[o][c] over the (o, c) with arg >= 0, in `dtype`; -> (dx, sum of the |terms| per element)."""
    n_out, C = dy.shape
    dx = torch.zeros((n_in, C), dtype=dtype, device=dy.device)
    mag = torch.zeros_like(dx)
    has = arg >= 0
    ch = torch.arange(C, device=dy.device).expand(n_out, C)
    dx.index_put_((arg[has].long(), ch[has]), dy.to(dtype)[has], accumulate=True)
    mag.index_put_((arg[has].long(), ch[has]), dy.to(dtype)[has].abs(), accumulate=True)
    return dx, mag


# ---- torch twins of the four operators (differentiable by torch's autograd) ---------------------------------------------------
def dense_twin(feats, coords, min3, ts, shape5):
    """`SparseTensor.dense()` with index_put (not accumulating: several rows on one site each get its gradient)."""
    B, C, X, Y, Z = shape5
    ok, b, x, y, z = sites_of(coords, min3, ts, (B, X, Y, Z))
    grid = torch.zeros((B, X, Y, Z, C), dtype=feats.dtype, device=feats.device)
    grid = grid.index_put((b[ok], x[ok], y[ok], z[ok]), feats[ok])
    return grid.permute(0, 4, 1, 2, 3)


def to_sparse_twin(x, site_coords):
    """The features of `to_sparse()` by advanced indexing at the sites the operator chose."""
    c = site_coords.long()
    return x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]]


def maxpool_twin(x, nbr):
    n_in = x.shape[0]
    xz = torch.cat([x, torch.full((1, x.shape[1]), float("-inf"), dtype=x.dtype, device=x.device)])
    nb = torch.where(nbr >= 0, nbr.long(), torch.full_like(nbr, n_in).long())
    return xz[nb].max(dim=0).values           # every window of the maps used here has a present neighbour


def row_stack_twin(params, maps, x, tgt, dtype):
    """The stack of tests/rowgrad_cases.py `RowStack` in plain torch on the recorded maps, in `dtype` -> {name: gradient}, "x"
    included."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xi = x.detach().to(dtype).requires_grad_(True)
    y1 = conv_twin(xi, p["c1.kernel"], maps["nbr1"], p["c1.bias"])
    h = F.batch_norm(y1, None, None, p["bn.bn.weight"], p["bn.bn.bias"], True, 0.1, 1e-5)
    h = conv_twin(torch.relu(h), p["c2.kernel"], maps["nbr2"])
    d = dense_twin(h, maps["coords2"], maps["min3"], 2, maps["shape5"])
    d = torch.relu(F.conv3d(d, p["dense3d.weight"], p["dense3d.bias"], padding=1))
    h = to_sparse_twin(d, maps["sites"])
    h = conv_twin(h, p["up.kernel"], maps["nbr4"])
    h = h[maps["keep"].long()]
    u = torch.cat([h, torch.zeros(maps["n_union"] - h.shape[0], h.shape[1], dtype=dtype, device=x.device)])
    u = u.index_add(0, maps["b2o"].long(), y1)
    out = conv_twin(u, p["head.kernel"], None, p["head.bias"])
    pool = maxpool_twin(y1, maps["nbr_pool"])
    loss = (out - tgt.to(dtype)).square().mean() + pool.square().mean()
    loss.backward()
    g = {k: v.grad for k, v in p.items()}
    g["x"] = xi.grad
    return g
