"""Torch restatement of include/pasco_grad.h for CPU tensors: index operations and matrix products in the tensor's dtype.  The
CPU tests run on it and `pasco_amd.me.autograd` uses it where the features are not on a GPU.  Same results as the kernels up to
the order of the fp32 sums."""
from __future__ import annotations

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
