"""Training operators of the sparse convolution family (include/pasco_grad.h): the inverse of a neighbour table, the weight
gradient and the bias gradient; of the dense <-> rows operators and local max pooling (include/pasco_rowgrad.h); and of the
masked cross-attention (include/pasco_attngrad.h); the matcher and mask losses (include/pasco_match.h); and the semantic
completion losses (include/pasco_semloss.h); and of training-mode batch normalisation over rows, local or synchronised
(include/pasco_norm.h: `normlib` binds the `pn_*` entry points, `norm.batch_norm_rows` is the operator).  `host` restates them in torch (CPU tensors, the tensor's dtype), `lib` binds the
`pg_*` entry points, `rowlib` the `pr_*` ones, `poollib` the `pp_*` ones (include/pasco_pool.h: pooling, broadcast and the
channel-wise convolution; `pool_ops` picks the binding or `host` for a tensor), `fieldlib` the `pq_*` ones (include/pasco_field.h:
point <-> voxel grouping, segment rows and interpolation; `field_ops`), `knnlib` the `pk_*` ones (include/pasco_knn.h: the
bipartite k-nearest-neighbour search, weights and gather behind `knn.knn_up`; `knn.knn_ops`), `attnlib` the `pa_*` ones, `matchlib` the `pm_*` ones and `semlib` the `ps_*` ones;
the functions here serve a tensor from the one its device calls for.  The autograd functions that use them are
`pasco_amd.me.autograd`, `pasco_amd.grad.attention`, `pasco_amd.grad.criterion` and `pasco_amd.grad.semloss`.  The step that
consumes the gradients is `optim.AdamW` (include/pasco_optim.h: `optimlib` binds the `po_*` entry points)."""
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


def dense_rows(dense: torch.Tensor, coords: torch.Tensor, min3, ts: int) -> torch.Tensor:
    if dense.is_cuda:
        from .rowlib import rowgrad_lib
        return rowgrad_lib().dense_rows(dense, coords, min3, ts)
    return host.dense_rows(dense, coords, min3, ts)


def rows_dense(rows: torch.Tensor, site_coords: torch.Tensor, shape5) -> torch.Tensor:
    if rows.is_cuda:
        from .rowlib import rowgrad_lib
        return rowgrad_lib().rows_dense(rows, site_coords, shape5)
    return host.rows_dense(rows, site_coords, shape5)


def maxpool_arg(x: torch.Tensor, nbr: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    if x.is_cuda:
        from .rowlib import rowgrad_lib
        return rowgrad_lib().maxpool_arg(x, nbr, out)
    return host.maxpool_arg(x, nbr, out)


def maxpool_bwd(dy: torch.Tensor, arg: torch.Tensor, inv: torch.Tensor, n_in: int) -> torch.Tensor:
    if dy.is_cuda:
        from .rowlib import rowgrad_lib
        return rowgrad_lib().maxpool_bwd(dy, arg, inv, n_in)
    return host.maxpool_bwd(dy, arg, inv, n_in)


class _HostPool:
    """`host.pool_*` under the method names of `poollib.PoolLib`."""
    seg_reduce = staticmethod(host.pool_seg_reduce)
    seg_max_bwd = staticmethod(host.pool_seg_max_bwd)
    broadcast = staticmethod(host.pool_broadcast)
    broadcast_mul_bwd = staticmethod(host.pool_broadcast_mul_bwd)
    pool = staticmethod(host.pool_pool)
    pool_bwd = staticmethod(host.pool_pool_bwd)
    chconv_fwd = staticmethod(host.pool_chconv_fwd)
    chconv_wgrad = staticmethod(host.pool_chconv_wgrad)


_HOST_POOL = _HostPool()


def pool_ops(t: torch.Tensor):
    """What serves the include/pasco_pool.h operators for `t`: the `pp_*` binding on a GPU (fp32 only), `host` otherwise."""
    if t.is_cuda:
        if t.dtype != torch.float32:
            raise TypeError(f"the pooling / broadcast / channel-wise kernels serve fp32 rows on the device, got {t.dtype}")
        from .poollib import pool_lib
        return pool_lib()
    return _HOST_POOL


class _HostField:
    """`host.field_*` under the method names of `fieldlib.FieldLib`."""
    group = staticmethod(host.field_group)
    seg_rows = staticmethod(host.field_seg_rows)
    seg_max_bwd = staticmethod(host.field_seg_max_bwd)
    gather_w = staticmethod(host.field_gather_w)
    interp_map = staticmethod(host.field_interp_map)
    interp_fwd = staticmethod(host.field_interp_fwd)


_HOST_FIELD = _HostField()


def field_ops(t: torch.Tensor, rows: bool = True):
    """What serves the include/pasco_field.h operators for `t`: the `pq_*` binding on a GPU (`rows`: `t` holds feature rows, fp32
    only), `host` otherwise."""
    if t.is_cuda:
        if rows and t.dtype != torch.float32:
            raise TypeError(f"the point / voxel kernels (TensorField, slice, interpolation) serve fp32 rows on the device, got {t.dtype}")
        from .fieldlib import field_lib
        return field_lib()
    return _HOST_FIELD


def attn_cross_bwd(q, k, v, bits, any_, out, dout, need_q: bool = True, need_k: bool = True, need_v: bool = True):
    if q.is_cuda:
        from .attnlib import attn_grad_lib
        return attn_grad_lib().attn_cross_bwd(q, k, v, bits, any_, out, dout, need_q, need_k, need_v)
    return host.attn_cross_bwd(q, k, v, bits, any_, out, dout, need_q, need_k, need_v)


def target_pack(masks, unknown, coords, origin=(0, 0, 0)):
    if coords.is_cuda:
        from .matchlib import match_lib
        return match_lib().target_pack(masks, unknown, coords, origin)
    return host.target_pack(masks, unknown, coords, origin)


def pair_sums(logits, tbits, flags, flag_bit: int, t: int):
    if logits.is_cuda:
        from .matchlib import match_lib
        return match_lib().pair_sums(logits, tbits, flags, flag_bit, t)
    return host.pair_sums(logits, tbits, flags, flag_bit, t)


def mask_loss_bwd(logits, tbits, flags, tgt_of_query, coef, t: int):
    if logits.is_cuda:
        from .matchlib import match_lib
        return match_lib().mask_loss_bwd(logits, tbits, flags, tgt_of_query, coef, t)
    return host.mask_loss_bwd(logits, tbits, flags, tgt_of_query, coef, t)


from .semloss import (SemComplLossFunction, compute_sem_compl_loss, compute_sem_compl_loss_kitti360,  # noqa: E402,F401
                      sem_compl_loss)
from .norm import BatchNormRowsFunction, batch_norm_rows, group_gather  # noqa: E402,F401
from .optim import AdamW, warmup_cosine  # noqa: E402,F401
