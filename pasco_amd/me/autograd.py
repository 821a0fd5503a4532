"""Autograd of the sparse convolution family: `MinkowskiConvolution` / `...Transpose` / `...GenerativeConvolutionTranspose`,
`MinkowskiPruning` and the two-map `SparseTensor.__add__`; and of the operators between them: `SparseTensor.dense()`,
`to_sparse()`, the duplicate-dropping `SparseTensor(features, coordinates)` and `MinkowskiMaxPooling`.

Each function's `forward` performs the very launches the module performs without autograd (the caller passes its own launch
helper), so the forward values are the same bits in every mode; only the `grad_fn` is new.  The backward launches are
include/pasco_grad.h and include/pasco_rowgrad.h on the device and `pasco_amd.grad.host` for CPU tensors.  Once differentiable:
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
