"""Autograd of the sparse convolution family: `MinkowskiConvolution` / `...Transpose` / `...GenerativeConvolutionTranspose`,
`MinkowskiPruning` and the two-map `SparseTensor.__add__`.

Each function's `forward` performs the very launches the module performs without autograd (the caller passes its own launch
helper), so the forward values are the same bits in every mode; only the `grad_fn` is new.  The backward launches are
include/pasco_grad.h on the device and `pasco_amd.grad.host` for CPU tensors.  Once differentiable: no double backward.

Used only when autograd is enabled and an input requires grad (`modules._ConvBase.conv_rows`, `MinkowskiPruning.forward`,
`SparseTensor._binary`); the inference paths never come here."""
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
