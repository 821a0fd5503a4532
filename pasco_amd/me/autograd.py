"""Autograd of the sparse convolution family: `MinkowskiConvolution` / `...Transpose` / `...GenerativeConvolutionTranspose`,
`MinkowskiPruning` and the two-map `SparseTensor.__add__`; and of the operators between them: `SparseTensor.dense()`,
`to_sparse()`, the duplicate-dropping `SparseTensor(features, coordinates)` and `MinkowskiMaxPooling`; and of the pooling,
broadcast and channel-wise modules (include/pasco_pool.h); and of the point <-> voxel operators (include/pasco_field.h):
`TensorField.sparse()` and `SparseTensor(features, coordinates, quantization_mode=...)` under a sum / average / max mode,
`SparseTensor.slice` and `MinkowskiInterpolation`.

Each function's `forward` performs the very launches the module performs without autograd (the caller passes its own launch
helper), so the forward values are the same bits in every mode; only the `grad_fn` is new.  The backward launches are
include/pasco_grad.h, include/pasco_rowgrad.h and include/pasco_pool.h on the device and `pasco_amd.grad.host` for CPU tensors.  Once differentiable:
no double backward.

Used only when autograd is enabled and an input requires grad (`modules._ConvBase.conv_rows`, `MinkowskiPruning.forward`,
`MinkowskiMaxPooling.forward`, `SparseTensor.__init__` / `._binary` / `.dense`, `core.to_sparse`); the inference paths never come
here."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from .. import grad as G


def wants_grad(*tensors) -> bool:
    """Autograd is enabled and one of the tensors (None entries skipped) requires grad."""
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


class ConvFunction(torch.autograd.Function):
    """out = sum_k feats[nbr[k]] @ kernel[k] + bias.  `launch(feats)` is the module's forward launch sequence for its present
    state (kernel and bias detached inside it)."""

    @staticmethod
    def forward(ctx, feats, kernel, bias, launch, be, nbr, n_out, mgr):
        feats = feats.contiguous()
        out = launch(feats)
        ctx.save_for_backward(feats, kernel, nbr)
        ctx.be, ctx.mgr, ctx.has_bias = be, mgr, bias is not None
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        feats, kernel, nbr = ctx.saved_tensors
        dy = dy.contiguous()
        n_in, cin = feats.shape
        cout = dy.shape[1]
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        d_x = d_w = d_b = None
        if nbr is None:                       # k = 1, stride 1: plain products
            w = kernel.detach().reshape(cin, cout)
            if need_x:
                d_x = dy @ w.t()
            if need_w:
                d_w = (feats.t() @ dy).reshape(kernel.shape)
        else:
            K = nbr.shape[0]
            if need_x:
                if n_in == 0 or dy.shape[0] == 0:
                    d_x = torch.zeros_like(feats)
                else:
                    inv = ctx.mgr.kernel_map_inverse(nbr, n_in) if ctx.mgr is not None else G.nbr_invert(nbr, n_in)
                    w_t = kernel.detach().reshape(K, cin, cout).transpose(1, 2).contiguous()
                    d_x = ctx.be.conv_fwd(dy, w_t, inv, n_in)          # the exact fp32 route of the forward kernels
            if need_w:
                d_w = G.conv_wgrad(feats, dy, nbr).reshape(kernel.shape)
        if need_b:
            d_b = G.colsum(dy).reshape(1, cout)
        return d_x, d_w, d_b, None, None, None, None, None


class GatherRowsFunction(torch.autograd.Function):
    """out = x[keep] (`keep` int32, distinct rows): the backward scatters the gradient into zeros of x's shape."""

    @staticmethod
    def forward(ctx, x, keep, be):
        ctx.save_for_backward(keep)
        ctx.be, ctx.shape = be, tuple(x.shape)
        return be.gather_rows(x.contiguous(), keep)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (keep,) = ctx.saved_tensors
        d_x = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
        if keep.shape[0]:
            ctx.be.scatter_add_rows(g.contiguous(), keep, d_x)
        return d_x, None, None


class UnionAddFunction(torch.autograd.Function):
    """The two-map `a + b`: `launch(a, b)` builds the union rows (lhs rows first, rhs rows added at `b2o`)."""

    @staticmethod
    def forward(ctx, a, b, b2o, launch, be):
        ctx.save_for_backward(b2o)
        ctx.be, ctx.na = be, a.shape[0]
        return launch(a, b)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (b2o,) = ctx.saved_tensors
        g = g.contiguous()
        d_a = g[:ctx.na] if ctx.needs_input_grad[0] else None
        d_b = ctx.be.gather_rows(g, b2o.contiguous()) if ctx.needs_input_grad[1] else None
        return d_a, d_b, None, None, None


class DenseFunction(torch.autograd.Function):
    """`SparseTensor.dense()`: dense[b_i, :, site(i)] = feats[i] (`be.to_dense`).  The backward reads every row's site back:
    d_feats[i] = g[b_i, :, site(i)], a zero row where the forward skipped the row (outside the grid after the wrap of an index in
    [-dim, 0), or a batch index outside).  Several rows on one site (only a wrap produces them) EACH receive that site's
    gradient although the forward kept only one of them: it is what torch's autograd gives for `index_put_`, and which row
    stayed is not recorded anywhere."""

    @staticmethod
    def forward(ctx, feats, coords, min3, step, dims, be):
        ctx.save_for_backward(coords)
        ctx.min3, ctx.step = tuple(min3), int(step)
        return be.to_dense(feats.contiguous(), coords, min3, step, dims)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (coords,) = ctx.saved_tensors
        return G.dense_rows(g.contiguous(), coords, ctx.min3, ctx.step), None, None, None, None, None


class ToSparseFunction(torch.autograd.Function):
    """`to_sparse()`: -> (coords, feats) of `be.to_sparse` (the site scan, then `be.dense_gather`).  The coordinates are decided
    from the values and carry no gradient; the backward stores g[i] at row i's site of a zero tensor of the dense's shape (the
    sites are distinct and in range by construction)."""

    @staticmethod
    def forward(ctx, x, be):
        coords, feats = be.to_sparse(x)
        ctx.mark_non_differentiable(coords)
        ctx.save_for_backward(coords)
        ctx.shape = tuple(x.shape)
        return coords, feats

    @staticmethod
    @once_differentiable
    def backward(ctx, _g_coords, g):
        (coords,) = ctx.saved_tensors
        return G.rows_dense(g.contiguous(), coords, ctx.shape), None


class MaxPoolFunction(torch.autograd.Function):
    """`MinkowskiMaxPooling`: out = `be.maxpool_fwd(x, nbr)`.  The forward also records arg[o][c] = the input row of the first
    offset whose value == out[o][c] (-1: empty window or a NaN maximum); the backward routes dy[o][c] to that one row,
    dx[i][c] = sum over k ascending with o = inv[k][i] >= 0 of dy[o][c] [arg[o][c] == i]."""

    @staticmethod
    def forward(ctx, x, nbr, be, mgr):
        x = x.contiguous()
        out = be.maxpool_fwd(x, nbr)
        ctx.save_for_backward(G.maxpool_arg(x, nbr, out), nbr)
        ctx.mgr, ctx.n_in = mgr, x.shape[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        arg, nbr = ctx.saved_tensors
        inv = ctx.mgr.kernel_map_inverse(nbr, ctx.n_in) if ctx.mgr is not None else G.nbr_invert(nbr, ctx.n_in)
        return G.maxpool_bwd(dy.contiguous(), arg, inv, ctx.n_in), None, None, None


# ---- include/pasco_pool.h: per-batch reductions, broadcast, local sum / average pooling, pooling transpose, channel-wise convolution
class SegReduceFunction(torch.autograd.Function):
    """`MinkowskiGlobal{Sum,Avg,Max}Pooling`: out [B, c] = the per-batch sum / average / maximum of the rows (`ops.seg_reduce`).
    Backward: the sum copies dy[b_i] to every row, the average copies dy[b_i] / count[b_i], the maximum stores dy[b][ch] at the
    one row arg[b][ch] (none for an empty segment or a NaN maximum)."""

    @staticmethod
    def forward(ctx, x, coords, B, mode):
        x = x.contiguous()
        ops = G.pool_ops(x)
        out, count, arg = ops.seg_reduce(x, coords, B, mode)
        ctx.save_for_backward(coords, count, arg)
        ctx.ops, ctx.mode, ctx.n = ops, mode, x.shape[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        coords, count, arg = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.mode == G.host.POOL_MAX:
            return ctx.ops.seg_max_bwd(dy, arg, ctx.n), None, None, None
        cnt = count if ctx.mode == G.host.POOL_AVG else None
        return ctx.ops.broadcast(None, dy, coords, G.host.POOL_BC_COPY, cnt), None, None, None


class BroadcastFunction(torch.autograd.Function):
    """`MinkowskiBroadcast{Addition,Multiplication,Concatenation}` and `MinkowskiBroadcast`: out[i] = x[i] (+, *, cat) g[b_i], or
    g[b_i] alone (x is None).  Backward: the product's two gradients come out of one pass (`ops.broadcast_mul_bwd`); for the
    others the rows' gradient is dy (or its leading columns) and the global tensor's is the per-batch sum of dy (or of its
    trailing columns)."""

    @staticmethod
    def forward(ctx, x, g, coords, mode):
        g = g.contiguous()
        x = None if x is None else x.contiguous()
        ops = G.pool_ops(g)
        ctx.save_for_backward(coords, *((x, g) if mode == G.host.POOL_BC_MUL else ()))
        ctx.ops, ctx.mode, ctx.B, ctx.c = ops, mode, g.shape[0], 0 if x is None else x.shape[1]
        return ops.broadcast(x, g, coords, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        coords = ctx.saved_tensors[0]
        dy = dy.contiguous()
        need_x, need_g = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        d_x = d_g = None
        if ctx.mode == G.host.POOL_BC_MUL:
            _, x, g = ctx.saved_tensors
            d_x, d_g = ctx.ops.broadcast_mul_bwd(dy, x, g, coords, need_x, need_g)
        else:
            if need_x:
                d_x = dy[:, :ctx.c] if ctx.mode == G.host.POOL_BC_CAT else dy
            if need_g:
                d_g = ctx.ops.seg_reduce(dy[:, ctx.c:] if ctx.mode == G.host.POOL_BC_CAT else dy, coords, ctx.B, G.host.POOL_SUM)[0]
        return d_x, d_g, None, None


def gather_parents(x, parent, be):
    """x[parent]: the backend's row gather on the device, the index operation for CPU tensors (any dtype)."""
    return be.gather_rows(x, parent) if x.is_cuda else x[parent.long()]


def _inverse(mgr, nbr, n_in):
    return mgr.kernel_map_inverse(nbr, n_in) if mgr is not None else G.nbr_invert(nbr, n_in)


class PoolFunction(torch.autograd.Function):
    """`MinkowskiSumPooling` / `MinkowskiAvgPooling`: out[o] = the sum of the present neighbours (/ their number).  Backward over
    the inverse table: dx[i] = sum_k dy[inv[k][i]] (* 1 / cnt[inv[k][i]])."""

    @staticmethod
    def forward(ctx, x, nbr, mode, mgr):
        x = x.contiguous()
        ops = G.pool_ops(x)
        out, cnt = ops.pool(x, nbr, mode)
        ctx.save_for_backward(nbr, cnt)
        ctx.ops, ctx.mode, ctx.mgr, ctx.n_in = ops, mode, mgr, x.shape[0]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        nbr, cnt = ctx.saved_tensors
        return ctx.ops.pool_bwd(dy.contiguous(), cnt, _inverse(ctx.mgr, nbr, ctx.n_in), ctx.n_in, ctx.mode), None, None, None


class PoolTransposeFunction(torch.autograd.Function):
    """`MinkowskiPoolingTranspose` at kernel == stride: out[child] = x[parent] (`be.gather_rows`; every child has one parent).
    Backward: dx[parent] = the sum of its children's gradients, the local sum pooling over the inverse of the same table."""

    @staticmethod
    def forward(ctx, x, parent, nbr, be, mgr):
        x = x.contiguous()
        ctx.save_for_backward(nbr)
        ctx.ops, ctx.mgr, ctx.n_in = G.pool_ops(x), mgr, x.shape[0]
        return gather_parents(x, parent, be)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (nbr,) = ctx.saved_tensors
        return ctx.ops.pool(dy.contiguous(), _inverse(ctx.mgr, nbr, ctx.n_in), G.host.POOL_SUM)[0], None, None, None, None


class ChannelwiseConvFunction(torch.autograd.Function):
    """`MinkowskiChannelwiseConvolution`: out[o][ch] = sum_k x[nbr[k][o]][ch] * kernel[k][ch] (+ bias[ch]).  Backward: the input
    gradient is the same operator over the inverse table with the same weights, the kernel's is `ops.chconv_wgrad`, the bias's
    the column sum of dy."""

    @staticmethod
    def forward(ctx, x, kernel, bias, nbr, mgr):
        x = x.contiguous()
        ops = G.pool_ops(x)
        w = kernel.detach().contiguous()
        ctx.save_for_backward(x, w, nbr)
        ctx.ops, ctx.mgr, ctx.has_bias = ops, mgr, bias is not None
        return ops.chconv_fwd(x, nbr, w, None if bias is None else bias.detach().reshape(-1).contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, nbr = ctx.saved_tensors
        dy = dy.contiguous()
        d_x = d_w = d_b = None
        if ctx.needs_input_grad[0]:
            d_x = ctx.ops.chconv_fwd(dy, _inverse(ctx.mgr, nbr, x.shape[0]), w, None)
        if ctx.needs_input_grad[1]:
            d_w = ctx.ops.chconv_wgrad(x, dy, nbr)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            d_b = G.colsum(dy).reshape(1, -1)
        return d_x, d_w, d_b, None, None


# ---- include/pasco_field.h: quantisation of points to voxels, slice, interpolation
class FieldReduceFunction(torch.autograd.Function):
    """`TensorField.sparse()` under a sum / average / max mode: out [n_vox, c] = `ops.seg_rows` over the points of every voxel
    (`offsets`, `perm`: the grouping of `inv`, the voxel row of every point).  Backward: the sum hands dy[inv[p]] to point p, the
    average dy[inv[p]] * (1 / cnt[inv[p]]) (`ops.gather_w`), the maximum stores dy[v][ch] at the one point arg[v][ch].  A point
    without a voxel gets a zero row.  No gradient goes to the coordinates."""

    @staticmethod
    def forward(ctx, x, offsets, perm, inv, mode, be):
        x = x.contiguous()
        ops = G.field_ops(x)
        out, cnt, arg = ops.seg_rows(x, offsets, perm, mode)
        ctx.save_for_backward(inv, cnt, arg)
        ctx.ops, ctx.mode, ctx.n, ctx.be = ops, mode, x.shape[0], be
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        from .core import gather_or_zero
        inv, cnt, arg = ctx.saved_tensors
        dy = dy.contiguous()
        if ctx.mode == G.host.FIELD_MAX:
            d_x = ctx.ops.seg_max_bwd(dy, arg, ctx.n)
        elif ctx.mode == G.host.FIELD_AVG:
            d_x = ctx.ops.gather_w(dy, inv, cnt)
        else:
            d_x = gather_or_zero(dy, inv, ctx.be)
        return d_x, None, None, None, None, None


class SliceFunction(torch.autograd.Function):
    """`SparseTensor.slice`: out[p] = x[inv[p]] (a zero row where inv[p] is -1).  Backward: dx[v] = the sum of the gradients of
    the voxel's points in ascending point order (`ops.seg_rows`, sum) over the grouping `grouping(ops)` the manager caches."""

    @staticmethod
    def forward(ctx, x, inv, grouping, be):
        from .core import gather_or_zero
        x = x.contiguous()
        ctx.ops, ctx.grouping = G.field_ops(x), grouping
        return gather_or_zero(x, inv, be)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        offsets, perm = ctx.grouping(ctx.ops)
        return ctx.ops.seg_rows(dy.contiguous(), offsets, perm, G.host.FIELD_SUM)[0], None, None, None


class InterpolationFunction(torch.autograd.Function):
    """`MinkowskiInterpolation`: out[p] = sum_k weights[k][p] * x[rows[k][p]] (`ops.interp_fwd`).  Backward: the [8, M] table
    flattened is a list of 8 M entries keyed by input row; grouped (`ops.group`), the terms weights[j] * dy[j % M] of every input
    row are added in ascending (k, p) (`ops.seg_rows` with w = weights, src_mod = M).  No gradient goes to the points."""

    @staticmethod
    def forward(ctx, x, rows, weights):
        x = x.contiguous()
        ops = G.field_ops(x)
        ctx.save_for_backward(rows, weights)
        ctx.ops, ctx.n_in = ops, x.shape[0]
        return ops.interp_fwd(x, rows, weights)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        rows, weights = ctx.saved_tensors
        m = rows.shape[1]
        offsets, perm = ctx.ops.group(rows.reshape(-1), ctx.n_in)
        d_x = ctx.ops.seg_rows(dy.contiguous(), offsets, perm, G.host.FIELD_SUM, w=weights.reshape(-1), src_mod=max(m, 1))[0]
        return d_x, None, None
