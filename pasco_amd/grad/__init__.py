"""Training operators of the sparse convolution family (include/pasco_grad.h): the inverse of a neighbour table, the weight
gradient and the bias gradient.  `host` restates the three in torch (CPU tensors, the tensor's dtype), `lib` binds the `pg_*`
entry points; `nbr_invert`, `conv_wgrad` and `colsum` here serve a tensor from the one its device calls for.  The autograd
functions that use them are `pasco_amd.me.autograd`."""
from __future__ import annotations

import torch

from . import host  # noqa: F401


def nbr_invert(nbr: torch.Tensor, n_in: int) -> torch.Tensor:
    if nbr.is_cuda:
        from .lib import grad_lib
        return grad_lib().nbr_invert(nbr, n_in)
    return host.nbr_invert(nbr, n_in)


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, nbr: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        from .lib import grad_lib
        return grad_lib().conv_wgrad(x, dy, nbr)
    return host.conv_wgrad(x, dy, nbr)


def colsum(dy: torch.Tensor) -> torch.Tensor:
    if dy.is_cuda:
        from .lib import grad_lib
        return grad_lib().colsum(dy)
    return host.colsum(dy)
