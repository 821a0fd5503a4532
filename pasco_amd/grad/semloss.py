"""The semantic completion losses of training (the reference's `compute_sem_compl_loss` and `compute_sem_compl_loss_kitti360`):
per scale and subnet a class-weighted cross entropy and the Lovasz-softmax loss of the [N, C] logits against the dense labels,
forward and backward on the `ps_*` kernels (include/pasco_semloss.h) for device tensors and on `grad.host` for CPU tensors.

The box test `min_C <= C[:, 1:4] <= max_C` is part of the kernels: nothing is pruned and no row is copied, and the gradient
arrives at `sem_logit.F` itself.  The Lovasz order is fixed: descending error, equal errors in ascending row order."""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import host
from .semlib import PS_MAX_C, PS_MIN_C, check_classes


def _stages(F, coords, target, box, scale, weights) -> dict:
    if F.is_cuda:
        from .semlib import sem_lib
        return sem_lib().forward(F, coords, target, box, scale, weights)
    label, ce, class_count, info, err = host.sem_rows_fwd(F, coords, target, box, scale, weights)
    keys = err.to(torch.float32).view(torch.int32) if err.numel() else torch.zeros(err.shape, dtype=torch.int32)
    perm = host.sem_sort_desc(keys)
    loss_c, coef, lovasz, present = host.sem_lovasz_fwd(perm, label, err, class_count)
    return {"label": label, "ce": ce, "class_count": class_count, "info": info, "loss_c": loss_c, "coef": coef, "lovasz": lovasz,
            "present": present, "keys": keys, "perm": perm}


class SemComplLossFunction(torch.autograd.Function):
    """(F fp32 [N, C], C int32 [N, 4], target uint8 [X, Y, Z], min_C int [3], max_C int [3], scale, weights fp32 [C]) ->
    (ce [], lovasz []).  A list given as `sink` receives info int32 [4] = (rows inside the box, label indices outside the grid,
    labels in C..254, the classes present) ON THE DEVICE, so that a caller reads the words of many calls with one copy.  Saved for
    the backward: F, the labels [N], coef [N, C], the cross-entropy sums and the present count.  Once differentiable."""

    @staticmethod
    def forward(ctx, F, coords, target, min_C, max_C, scale, weights, sink=None):
        check_classes(int(F.shape[1]))
        F = F.contiguous()
        dev = F.device
        box = torch.cat([torch.as_tensor(min_C).reshape(3), torch.as_tensor(max_C).reshape(3)]).to(device=dev, dtype=torch.int32)
        coords = coords.to(torch.int32).contiguous()
        if target.dtype != torch.uint8:
            target = target.to(torch.uint8)
        weights = weights.to(device=dev, dtype=F.dtype).contiguous()
        out = _stages(F, coords, target.contiguous(), box, int(scale), weights)
        ctx.save_for_backward(F, out["label"], out["coef"], weights, out["ce"], out["present"])
        if sink is not None:
            sink.append(torch.cat([out["info"][:3], out["present"]]))
        return out["ce"][0].clone(), out["lovasz"][0].clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, g_ce, g_lov):
        F, label, coef, weights, ce, present = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 8
        g = torch.stack([g_ce.to(F.dtype), g_lov.to(F.dtype)])
        if F.is_cuda:
            from .semlib import sem_lib
            d = sem_lib().loss_bwd(F, label, coef, weights, ce, present, g)
        else:
            d = host.sem_loss_bwd(F, label, coef, weights, ce, present, g)
        return d, None, None, None, None, None, None, None


def sem_compl_loss(F, coords, target, min_C, max_C, scale, weights, sink=None):
    """One (scale, subnet) pair -> (ce, lovasz); differentiable in `F`.  See SemComplLossFunction."""
    return SemComplLossFunction.apply(F, coords, target, min_C, max_C, scale, weights, sink)


_WEIGHTS: Dict[Tuple, torch.Tensor] = {}


def class_weights(freq, exponent: float, device, dtype=torch.float32) -> torch.Tensor:
    """w = (max(f) / f) ** exponent with f = freq / sum(freq), as the reference forms it in numpy; cached per (frequencies,
    exponent, device)."""
    f = np.asarray(freq)
    key = (f.tobytes(), str(f.dtype), float(exponent), str(device), dtype)
    w = _WEIGHTS.get(key)
    if w is None:
        r = f / np.sum(f)
        w = _WEIGHTS[key] = torch.from_numpy(np.power(np.amax(r) / r, exponent)).to(device=device, dtype=dtype)
    return w


def _compute(sem_labels, sem_logits_at_scales, min_Cs, max_Cs, class_frequencies, exponent: float, skip_empty: bool):
    ces, lovs, infos, ncls = [], [], [], []
    for scale in sem_logits_at_scales:
        sem_logits = sem_logits_at_scales[scale]
        targets = sem_labels["1_{}".format(scale)]
        F0 = sem_logits[0].F
        w = class_weights(class_frequencies["1_{}".format(scale)], exponent, F0.device, F0.dtype)
        for i in range(len(targets)):
            F = sem_logits[i].F
            c = int(F.shape[1])
            if not (PS_MIN_C <= c <= PS_MAX_C):
                raise ValueError(f"semantic completion loss: {c} classes not served ({PS_MIN_C}..{PS_MAX_C})")
            ce, lov = sem_compl_loss(F, sem_logits[i].C, targets[i], min_Cs[i], max_Cs[i], int(scale), w, infos)
            ces.append(ce)
            lovs.append(lov)
            ncls.append(c)
    if not ces:
        if skip_empty:
            return 0.0, 0.0
        raise RuntimeError("semantic completion loss: no (scale, subnet) pair")
    words = torch.stack(infos).cpu().tolist()       # the one host read of the call
    for (rows, bad_index, bad_label, _), c in zip(words, ncls):
        if bad_index:
            raise IndexError(f"semantic completion loss: {bad_index} rows inside the box index outside the label grid")
        if bad_label:
            raise ValueError(f"semantic completion loss: {bad_label} labels outside 0..{c - 1} and 255")
    keep = [k for k, wd in enumerate(words) if wd[0] > 0] if skip_empty else list(range(len(words)))
    if not keep:
        return 0.0, 0.0
    return torch.stack([ces[k] for k in keep]).mean(), torch.stack([lovs[k] for k in keep]).mean()


def compute_sem_compl_loss(sem_labels, sem_logits_at_scales, min_Cs, max_Cs, class_frequencies):
    """The reference's `compute_sem_compl_loss` (SemanticKITTI): weights (max f / f) ** (1/3); a (scale, subnet) pair with no row
    inside its box is skipped; (0.0, 0.0) when all are.  -> (mean ce, mean lovasz)."""
    return _compute(sem_labels, sem_logits_at_scales, min_Cs, max_Cs, class_frequencies, 1 / 3.0, True)


def compute_sem_compl_loss_kitti360(sem_labels, sem_logits_at_scales, min_Cs, max_Cs, class_frequencies):
    """The reference's `compute_sem_compl_loss_kitti360`: weights (max f / f) ** (1/1.5); no pair is skipped (a pair with no row
    inside its box gives ce = NaN, as torch's 0/0, and lovasz = 0)."""
    return _compute(sem_labels, sem_logits_at_scales, min_Cs, max_Cs, class_frequencies, 1 / 1.5, False)
