"""Test helper: the references of the pooling / broadcast / channel-wise tests (tests/pool_cases.py).  Every reference here is the
formula of include/pasco_pool.h in fp64, written without the index operations of pasco_amd/grad/host.py (one-hot products and
scatters over the FORWARD table where the code under test gathers over the inverse one), and returns with the value the two
figures the a-priori bound needs: mag = the sum of the absolute addends and T = the number of addends of each output element.
The dense twins (`dense_*`) restate the operators with torch's dense 3-D operators on a zero-filled grid."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24

# the one measured constant of tests/pool_cases.pool_stack_ratios: the worst max |g - g64| / max |g32 - g64| over the
# gradient tensors of the stack was 7.30 on the CPU (pw.bias) and 10.21 on the MI355X (fc2.linear.weight); 4 x the larger one,
# rounded up to a power of two (the rule of DESIGN.md 4k)
POOL_STACK_M = 64.0


def onehot(b: torch.Tensor, B: int) -> torch.Tensor:
    """fp64 [B, n]: 1 where row i belongs to batch index b (rows outside [0, B) belong to none)."""
    return (b.long()[None, :] == torch.arange(B, device=b.device)[:, None]).double()


def within(got: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor, T, extra: int = 0):
    """|got - ref| <= (T + 2 + extra) u mag element-wise -> (ok, the worst ratio of the error to the bound)."""
    err = (got.double() - ref).abs()
    bound = (torch.as_tensor(T, dtype=torch.float64, device=ref.device) + 2 + extra) * EPS * mag
    bad = err > bound
    worst = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    return not bool(bad.any()), worst


def seg_sum_ref(x, coords, B, y=None):
    """-> (sum fp64 [B, c], mag, T [B, 1], count fp64 [B]) of x (times y)."""
    oh = onehot(coords[:, 0], B)
    a = x.double() if y is None else x.double() * y.double()
    count = oh.sum(dim=1)
    return oh @ a, oh @ a.abs(), count[:, None], count


def seg_max_loop(x, coords, B):
    """-> (out [B, c] in x's dtype, arg int32 [B, c]) by a loop over the rows in ascending order: the first row that holds the
    maximum wins (==, so +0 and -0 tie), a NaN makes the maximum NaN and the arg -1, an empty segment gives 0 and -1."""
    xs, bs = x.detach().cpu().numpy(), coords[:, 0].cpu().numpy()
    n, c = xs.shape
    out = np.zeros((B, c), dtype=xs.dtype)
    arg = np.full((B, c), -1, dtype=np.int32)
    seen = np.zeros(B, dtype=bool)
    for i in range(n):
        b = int(bs[i])
        if b < 0 or b >= B:
            continue
        v = xs[i]
        if not seen[b]:
            seen[b] = True
            out[b] = v
            arg[b] = np.where(np.isnan(v), -1, i)
            continue
        was_nan = np.isnan(out[b])
        take_nan = ~was_nan & np.isnan(v)
        take = ~was_nan & ~np.isnan(v) & (v > out[b])
        out[b] = np.where(take | take_nan, v, out[b])
        arg[b] = np.where(take, i, np.where(take_nan, -1, arg[b]))
    return torch.from_numpy(out).to(x.device), torch.from_numpy(arg).to(x.device)


def present(table, n_src):
    return (table >= 0) & (table < n_src)


def pool_ref(x, nbr, avg: bool):
    """-> (out fp64 [n_out, c], mag, T [n_out, 1], cnt fp64 [n_out])."""
    K, n_out = nbr.shape
    n_in, c = x.shape
    have = present(nbr, n_in)
    cnt = have.double().sum(dim=0)
    out = torch.zeros((n_out, c), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    xd = x.double()
    for k in range(K):
        o = torch.nonzero(have[k]).reshape(-1)
        out[o] += xd[nbr[k, o].long()]
        mag[o] += xd[nbr[k, o].long()].abs()
    if avg:
        d = cnt.clamp(min=1)[:, None]
        out, mag = out / d, mag / d
    return out, mag, cnt[:, None], cnt


def pool_bwd_ref(dy, nbr, n_in, avg: bool):
    """The adjoint of `pool_ref` by a scatter over the forward table -> (dx fp64 [n_in, c], mag, T [n_in, 1])."""
    K, n_out = nbr.shape
    c = dy.shape[1]
    have = present(nbr, n_in)
    g = dy.double()
    if avg:
        g = g / have.double().sum(dim=0).clamp(min=1)[:, None]
    dx = torch.zeros((n_in, c), dtype=torch.float64, device=dy.device)
    mag = torch.zeros_like(dx)
    T = torch.zeros((n_in, 1), dtype=torch.float64, device=dy.device)
    for k in range(K):
        o = torch.nonzero(have[k]).reshape(-1)
        r = nbr[k, o].long()
        dx.index_put_((r,), g[o], accumulate=True)
        mag.index_put_((r,), g[o].abs(), accumulate=True)
        T.index_put_((r,), torch.ones((o.numel(), 1), dtype=torch.float64, device=dy.device), accumulate=True)
    return dx, mag, T


def chconv_ref(x, nbr, w, bias=None):
    """-> (out fp64 [n_out, c], mag, T [n_out, 1]); the bias is one more addend."""
    K, n_out = nbr.shape
    n_in, c = x.shape
    have = present(nbr, n_in)
    out = torch.zeros((n_out, c), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(out)
    xd, wd = x.double(), w.double()
    for k in range(K):
        o = torch.nonzero(have[k]).reshape(-1)
        t = xd[nbr[k, o].long()] * wd[k]
        out[o] += t
        mag[o] += t.abs()
    T = have.double().sum(dim=0)[:, None]
    if bias is not None:
        out, mag, T = out + bias.double().reshape(1, c), mag + bias.double().abs().reshape(1, c), T + 1
    return out, mag, T


def chconv_wgrad_ref(x, dy, nbr):
    """-> (dw fp64 [K, c], mag, T [K, 1])."""
    K, n_out = nbr.shape
    n_in, c = x.shape
    have = present(nbr, n_in)
    dw = torch.zeros((K, c), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(dw)
    for k in range(K):
        o = torch.nonzero(have[k]).reshape(-1)
        t = x.double()[nbr[k, o].long()] * dy.double()[o]
        dw[k], mag[k] = t.sum(dim=0), t.abs().sum(dim=0)
    return dw, mag, have.double().sum(dim=1)[:, None]


# ---- dense twins ---------------------------------------------------------------------------------------------------------------
def to_grid(rows, coords, dims, ts=1):
    """rows [n, c] at coords int32 [n, 4] (multiples of ts) -> dense [B, c, X, Y, Z] of `dims` = (B, X, Y, Z), zero elsewhere."""
    B, X, Y, Z = dims
    d = torch.zeros((B, rows.shape[1], X, Y, Z), dtype=rows.dtype, device=rows.device)
    c = coords.long()
    d[c[:, 0], :, c[:, 1] // ts, c[:, 2] // ts, c[:, 3] // ts] = rows
    return d


def at_sites(dense, coords, ts=1):
    c = coords.long()
    return dense[c[:, 0], :, c[:, 1] // ts, c[:, 2] // ts, c[:, 3] // ts]


def dense_pool(rows, coords, out_coords, dims, ks: int, stride: int, avg: bool):
    """Sum / average pooling as F.avg_pool3d(divisor_override=1) of the zero-filled grid (and of its occupancy mask)."""
    pad = ks // 2 if stride == 1 else 0
    d = to_grid(rows, coords, dims)
    s = F.avg_pool3d(d, ks, stride, pad, divisor_override=1)
    if avg:
        m = to_grid(torch.ones((rows.shape[0], 1), dtype=rows.dtype, device=rows.device), coords, dims)
        s = s / F.avg_pool3d(m, ks, stride, pad, divisor_override=1).clamp(min=1)
    return at_sites(s, out_coords, stride)


def dense_chconv(rows, coords, out_coords, dims, kernel, bias, ks: int, stride: int):
    """The channel-wise convolution as F.conv3d(groups=C): kernel [kvol, C] in `kernel_offsets` order (x fastest)."""
    c = rows.shape[1]
    w = kernel.reshape(ks, ks, ks, c).permute(3, 2, 1, 0).unsqueeze(1).contiguous()           # [C, 1, x, y, z]
    out = F.conv3d(to_grid(rows, coords, dims), w, None if bias is None else bias.reshape(-1), stride, ks // 2 if stride == 1 else 0,
                   groups=c)
    return at_sites(out, out_coords, stride)


def dense_global_avg(rows, coords, dims):
    """The masked mean per batch element of the zero-filled grid."""
    d = to_grid(rows, coords, dims)
    m = to_grid(torch.ones((rows.shape[0], 1), dtype=rows.dtype, device=rows.device), coords, dims)
    return d.sum(dim=(2, 3, 4)) / m.sum(dim=(2, 3, 4)).clamp(min=1)


def pool_stack_twin(params, feats, coords, tgt, dims, dtype):
    """`tests/pool_cases.PoolStack` in plain dense torch in `dtype` -> {name: gradient} of every parameter and of the input
    features ("x").  coords: the input's; tgt: the dense target [B, 4C, X, Y, Z]; the output sites are the children of the occupied
    stride-2 cells."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    x = feats.detach().to(dtype).requires_grad_(True)
    C = x.shape[1]
    m0 = to_grid(torch.ones((x.shape[0], 1), dtype=dtype, device=x.device), coords, dims)
    X0 = to_grid(x, coords, dims)
    b5 = lambda g: g[:, :, None, None, None]
    # squeeze and excitation
    gavg = X0.sum(dim=(2, 3, 4)) / m0.sum(dim=(2, 3, 4))
    h = torch.relu(gavg @ p["fc1.linear.weight"].t() + p["fc1.linear.bias"])
    se = torch.sigmoid(h @ p["fc2.linear.weight"].t() + p["fc2.linear.bias"])
    S = X0 * b5(se)
    # depthwise separable
    wd = p["dw.kernel"].reshape(3, 3, 3, C).permute(3, 2, 1, 0).unsqueeze(1)
    Y = F.conv3d(S, wd, p["dw.bias"].reshape(-1), padding=1, groups=C) * m0
    Y = (torch.einsum("bcxyz,cd->bdxyz", Y, p["pw.kernel"]) + b5(p["pw.bias"].reshape(1, -1))) * m0
    cnt = F.avg_pool3d(m0, 2, divisor_override=1)
    m1 = (cnt > 0).to(dtype)
    D = F.avg_pool3d(Y, 2, divisor_override=1)
    H = (D + D / cnt.clamp(min=1)) * m1
    up = lambda t: t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)
    U, m2 = up(H), up(m1)
    g2 = U.sum(dim=(2, 3, 4)) / m2.sum(dim=(2, 3, 4))
    V = torch.cat([(U + b5(g2)) * m2, b5(g2) * m2], dim=1)
    loss = ((V - tgt.to(dtype)) * m2).square().sum() / (m2.sum() * V.shape[1])
    loss.backward()
    out = {k: v.grad for k, v in p.items()}
    out["x"] = x.grad
    return out
