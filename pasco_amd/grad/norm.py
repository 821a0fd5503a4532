"""Training-mode batch normalisation over feature rows, local or synchronised over the ranks of a process group
(include/pasco_norm.h).

    y = batch_norm_rows(x, weight, bias, running_mean, running_var, num_batches_tracked, momentum, eps, act="relu",
                        gather=group_gather(process_group))

The statistics travel as mergeable fp64 records.  Forward: the moments record of the local rows, ONE collective (`gather`: the
record -> the stack [R, 3, c] of every rank's record in rank order), the merge of the stack by every rank itself in rank order,
the normalisation with the activation folded in.  Backward: the sums record (sum g, sum g * xhat) of the local rows, ONE
collective, the merge, dx.  Every rank merges the same records in the same order, so all ranks hold the same statistics bit for
bit and a repeat gives the same bits.  `weight.grad` / `bias.grad` are the LOCAL sums, as in `torch.nn.SyncBatchNorm`: the
data-parallel wrapper adds them over the ranks like every other parameter gradient.

EVERY rank of the group has to make the call (a collective waits for all of them); a rank without rows (n == 0) takes part
with a count-0 record and gets `[0, c]` back.  With a `gather` nothing is read on the host.

GPU rows run the `pn_*` kernels (fp32 only), CPU rows the torch restatement `grad.host.norm_*` with the same records and the
same merge order."""
from __future__ import annotations

from typing import Callable, Optional

import torch
from torch.autograd.function import once_differentiable

from . import host

ACTS = {"none": host.ACT_NONE, "relu": host.ACT_RELU, "leaky": host.ACT_LEAKY}


class _Host:
    """The entry points of `normlib.NormLib` on the torch restatement."""
    moments = staticmethod(host.norm_moments)
    moments_merge = staticmethod(host.norm_moments_merge)
    apply = staticmethod(host.norm_apply)
    bwd_sums = staticmethod(host.norm_bwd_sums)
    sums_merge = staticmethod(host.norm_sums_merge)
    bwd_dx = staticmethod(host.norm_bwd_dx)

    @staticmethod
    def finish(rec, eps, momentum, running_mean, running_var, dtype=torch.float32):
        return host.norm_finish(rec, eps, momentum, running_mean, running_var, dtype)


def _ops(x: torch.Tensor):
    if x.is_cuda:
        from .normlib import norm_lib
        return norm_lib()
    return _Host


def group_gather(group=None) -> Callable[[torch.Tensor], torch.Tensor]:
    """The `gather` of a torch.distributed process group: a record -> the stack of every rank's record, in rank order.  One
    all-gather; device tensors are staged through the host under gloo and passed directly under RCCL (`graph.dist`)."""
    import torch.distributed as dist

    from ..graph.dist import _all_gather

    def gather(rec: torch.Tensor) -> torch.Tensor:
        rec = rec.contiguous()
        outs = [torch.empty_like(rec) for _ in range(dist.get_world_size(group))]
        _all_gather(outs, rec, group=group)
        return torch.stack(outs)

    return gather


class BatchNormRowsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, factor, eps, act, slope, gather):
        ops = _ops(x)
        xc = x.detach().contiguous()
        w = weight.detach().contiguous() if weight is not None else None
        b = bias.detach().contiguous() if bias is not None else None
        rec = ops.moments(xc)
        total = rec if gather is None else ops.moments_merge(gather(rec).contiguous())
        if x.is_cuda:
            mean_rstd = ops.finish(total, eps, factor, running_mean, running_var)
        else:
            mean_rstd = ops.finish(total, eps, factor, running_mean, running_var, x.dtype)
        y = ops.apply(xc, mean_rstd, w, b, act, slope)
        ctx.save_for_backward(xc, mean_rstd, w, b, total)
        ctx.cfg = (act, slope, gather, weight is not None, bias is not None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        xc, mean_rstd, w, b, total = ctx.saved_tensors
        act, slope, gather, has_w, has_b = ctx.cfg
        ops = _ops(xc)
        dy = dy.contiguous()
        sums = ops.bwd_sums(dy, xc, mean_rstd, w, b, act, slope)
        dx = None
        if ctx.needs_input_grad[0] or gather is not None:        # the collective is made by every rank, needed here or not
            total_sums = sums if gather is None else ops.sums_merge(gather(sums).contiguous())
            if ctx.needs_input_grad[0]:
                dx = ops.bwd_dx(dy, xc, mean_rstd, w, b, act, slope, total_sums, total)
        dw = sums[1].to(xc.dtype) if has_w and ctx.needs_input_grad[1] else None
        db = sums[0].to(xc.dtype) if has_b and ctx.needs_input_grad[2] else None
        return dx, dw, db, None, None, None, None, None, None, None


def batch_norm_rows(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                    running_mean: Optional[torch.Tensor], running_var: Optional[torch.Tensor],
                    num_batches_tracked: Optional[torch.Tensor], momentum: Optional[float], eps: float, act: str = "none",
                    slope: float = 0.01, gather: Optional[Callable[[torch.Tensor], torch.Tensor]] = None) -> torch.Tensor:
    """Training-mode batch normalisation of the rows x [n, c] over the rows of all ranks, then `act` ("none", "relu", "leaky"
    with `slope`): y = act((x - mean) * rstd * weight + bias), differentiable in x, weight and bias.

    `running_mean` / `running_var` (None: not tracked) are updated in place by the kernel with the unbiased variance over the
    TOTAL count, `num_batches_tracked` (None: not tracked) is advanced in place by `add_(1)`.  `momentum=None` takes the
    cumulative average 1 / num_batches_tracked and costs the one host read torch.nn.BatchNorm1d pays for it too.
    `gather` = None: the local rows are all there is (one row raises torch's ValueError); otherwise see `group_gather`."""
    if x.dim() != 2:
        raise ValueError(f"batch_norm_rows: rows [n, c] expected, got {tuple(x.shape)}")
    if act not in ACTS:
        raise ValueError(f"batch_norm_rows: act = {act!r}, one of {sorted(ACTS)}")
    if x.dtype != torch.float32 and (x.is_cuda or gather is not None):
        raise TypeError(f"batch_norm_rows: fp32 rows only{' when synchronised' if gather is not None else ''}, got {x.dtype}")
    if gather is None and x.shape[0] == 1:
        raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
    factor = 0.0
    if num_batches_tracked is not None:
        num_batches_tracked.add_(1)
    if running_mean is not None or running_var is not None:
        if momentum is None:
            factor = 1.0 / float(num_batches_tracked) if num_batches_tracked is not None else 0.0
        else:
            factor = float(momentum)
    return BatchNormRowsFunction.apply(x, weight, bias, running_mean, running_var, factor, float(eps), ACTS[act], float(slope),
                                       gather)
