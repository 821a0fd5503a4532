"""The panoptic matcher and the three losses the reference's `Net.step` optimises, on the `pm_*` kernels
(include/pasco_match.h): drop-ins for `HungarianMatcher` (pasco/loss/matcher_sparse.py) and `SetCriterion`
(pasco/loss/criterion_sparse.py).

The dense targets [T, X, Y, Z] become one 128-bit word and one flag byte per voxel (`pack_targets`, once per batch element);
the matcher's cost and the mask losses are both read off ONE pass over the [N, Q] logits (`pm_pair_sums`, over the matchable
rows for the matcher and the known rows for the loss); the backward is one more pass (`pm_mask_loss_bwd`).  No [N, T] target
matrix, no transposed logits, no boolean compaction and no [N, K] tensor exists in either direction.  The assignment is
`pm_assign` on the host, so scipy is not needed.  CPU tensors are served by the restatements of `pasco_amd.grad.host`.

Served: at most 128 queries and 128 targets.  Not here: the Lovasz and `ssc_*` terms and the completion loss."""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import grad as G
from .matchlib import BIT_KNOWN, BIT_MATCHABLE, PM_MAX_Q, PM_MAX_T


class PackedTargets(NamedTuple):
    tbits: torch.Tensor      # int32 [N, 4]
    flags: torch.Tensor      # uint8 [N]
    oob: torch.Tensor        # int32 [1]: rows outside the grid (the caller raises IndexError when it reads it)
    t: int


def _check_counts(q: int, t: int):
    if q > PM_MAX_Q or t > PM_MAX_T:
        raise ValueError(f"panoptic match: {q} queries and {t} targets, at most {PM_MAX_Q} queries and {PM_MAX_T} targets are served")


def pack_targets(masks: torch.Tensor, unknown: Optional[torch.Tensor], coords: torch.Tensor, origin=(0, 0, 0)) -> PackedTargets:
    """masks [T, X, Y, Z] (non-zero = inside), unknown [X, Y, Z] | None, coords int [N, 4] (column 0 ignored) -> the words."""
    t = int(masks.shape[0])
    _check_counts(1, t)
    if t == 0:
        n, dev = int(coords.shape[0]), coords.device
        return PackedTargets(torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev), 0)
    m = masks if masks.dtype == torch.uint8 else (masks != 0).to(torch.uint8)
    u = None if unknown is None else (unknown if unknown.dtype == torch.uint8 else (unknown != 0).to(torch.uint8)).contiguous()
    tbits, flags, oob = G.target_pack(m.contiguous(), u, coords.to(torch.int32).contiguous(), [int(o) for o in origin])
    return PackedTargets(tbits, flags, oob, t)


def pack_rows(tgt_rows: torch.Tensor, unknown_rows: Optional[torch.Tensor]) -> PackedTargets:
    """The words from targets that are already per row: tgt_rows [N, T] (non-zero = inside), unknown_rows bool [N] | None.
    Plain torch, for the reference's call of the matcher; `pack_targets` is the kernel."""
    n, t = tgt_rows.shape
    _check_counts(1, t)
    tgt = tgt_rows != 0
    words = torch.zeros((n, 4), dtype=torch.int64, device=tgt_rows.device)
    for k in range(t):
        words[:, k >> 5] |= tgt[:, k].long() << (k & 31)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
    known = torch.ones(n, dtype=torch.bool, device=tgt_rows.device) if unknown_rows is None else ~unknown_rows.bool()
    flags = known.to(torch.uint8) | ((known & tgt.any(dim=1)).to(torch.uint8) << 1)
    return PackedTargets(words, flags.to(torch.uint8), torch.zeros(1, dtype=torch.int32, device=tgt_rows.device), int(t))


class MaskLossFunction(torch.autograd.Function):
    """(logits fp32 [N, Q], tbits, flags, src int64 [K], tgt int64 [K], weights fp32 [K], t) -> (loss_mask [K], loss_dice [K]):
    per matched pair k, the focal loss (alpha 0.25, gamma 2) averaged over the known rows and the dice loss over the known rows,
    each times weights[k] - the reference's `loss_mask.mean(0)` and `loss_dice` of `loss_masks`.  With no known row loss_mask is
    NaN, as the reference's mean over an empty tensor is.  Saved for the backward: the logits, the words, the flags and the
    [Q, T, 3] sums; nothing of size [N, K].  Once differentiable."""

    @staticmethod
    def forward(ctx, logits, tbits, flags, src, tgt, weights, t):
        logits = logits.contiguous()
        focal_sum, dice, stats, count = G.pair_sums(logits, tbits, flags, BIT_KNOWN, t)
        w = weights.to(logits.dtype)
        cnt = count.to(logits.dtype)
        loss_mask = focal_sum[src, tgt] / cnt * w
        loss_dice = dice[src, tgt] * w
        ctx.save_for_backward(logits, tbits, flags, stats, cnt, src, tgt, w)
        ctx.t = t
        return loss_mask, loss_dice

    @staticmethod
    @once_differentiable
    def backward(ctx, g_mask, g_dice):
        logits, tbits, flags, stats, cnt, src, tgt, w = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        q = logits.shape[1]
        inter, psum, tsum = stats[src, tgt].unbind(dim=1)
        den = psum + tsum + 1
        num = 2 * inter + 1
        gd = g_dice.to(logits.dtype) * w
        coef = torch.zeros((q, 3), dtype=logits.dtype, device=logits.device)
        coef[src] = torch.stack([g_mask.to(logits.dtype) * w / cnt, -2 * gd / den, gd * num / (den * den)], dim=1)
        tgt_of_query = torch.full((q,), -1, dtype=torch.int32, device=logits.device)
        tgt_of_query[src] = tgt.to(torch.int32)
        return G.mask_loss_bwd(logits, tbits, flags, tgt_of_query, coef, ctx.t), None, None, None, None, None, None


def mask_losses(logits, packed: PackedTargets, src, tgt, weights):
    """-> (loss_mask [K], loss_dice [K]) of the matched pairs (src[k], tgt[k]); differentiable in `logits`."""
    _check_counts(int(logits.shape[1]), packed.t)
    dev = logits.device
    return MaskLossFunction.apply(logits, packed.tbits, packed.flags, src.to(dev), tgt.to(dev), weights, packed.t)


class HungarianMatcher(nn.Module):
    """The reference's matcher: C = (cost_mask * focal / count + cost_class * (-softmax(query_logits)[:, labels]) + cost_dice *
    dice) * class_weights[labels] over the matchable rows (known, in at least one target), then the linear sum assignment.  The
    mask cost is 0 when no row is matchable (the reference's branch)."""

    def __init__(self, cost_class: float = 1, cost_mask: float = 1, cost_dice: float = 1):
        super().__init__()
        self.cost_class = cost_class
        self.cost_mask = cost_mask
        self.cost_dice = cost_dice
        assert cost_class != 0 or cost_mask != 0 or cost_dice != 0, "all costs cant be 0"

    @torch.no_grad()
    def cost_packed(self, voxel_logits, query_logits, labels, class_weights, packed: PackedTargets):
        """-> (C [Q, T] in the dtype of the logits, count int32 [1]), on the device of the logits."""
        _check_counts(int(voxel_logits.shape[1]), packed.t)
        focal_sum, dice, _, count = G.pair_sums(voxel_logits.detach().contiguous(), packed.tbits, packed.flags, BIT_MATCHABLE, packed.t)
        ids = labels.long()
        cnt = count.to(focal_sum.dtype)
        cost_mask = torch.where(cnt > 0, focal_sum / cnt.clamp(min=1), torch.zeros_like(focal_sum))
        cost_class = -query_logits.detach().softmax(-1)[:, ids]
        C = self.cost_mask * cost_mask + self.cost_class * cost_class.to(focal_sum.dtype) + self.cost_dice * dice
        return C * class_weights.to(C.device)[ids][None, :].to(C.dtype), count

    @torch.no_grad()
    def match_packed(self, voxel_logits, query_logits, labels, class_weights, packed: PackedTargets):
        """voxel_logits [N, Q], query_logits [Q, C+1], labels [T], class_weights [C+1] -> (src int64 [K], tgt int64 [K]) on the CPU.
        One device-to-host copy: the cost matrix with `count` and `oob` behind it."""
        q = int(voxel_logits.shape[1])
        if packed.t == 0:
            return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
        C, count = self.cost_packed(voxel_logits, query_logits, labels, class_weights, packed)
        buf = torch.cat([C.double().reshape(-1), count.double(), packed.oob.double()]).cpu()
        if int(buf[-1]) != 0:
            raise IndexError(f"panoptic match: {int(buf[-1])} voxel rows lie outside the target grid")
        cost = buf[:-2].reshape(q, packed.t)
        if voxel_logits.is_cuda:
            from .matchlib import match_lib
            return match_lib().assign(cost)
        return G.host.assign(cost)

    @torch.no_grad()
    def forward(self, outputs, targets, class_weights, unknown_mask_dense):
        """The reference's call: outputs["voxel_logits"] and targets["masks"] are sparse tensors over the same rows ([N, Q] and
        [N, T]), `unknown_mask_dense` bool [B, X, Y, Z] is read at the rows' coordinates."""
        vox, tm = outputs["voxel_logits"], targets["masks"]
        coords = tm.C.long()
        unknown = unknown_mask_dense[coords[:, 0], coords[:, 1], coords[:, 2], coords[:, 3]]
        packed = pack_rows(tm.F, unknown)
        return self.match_packed(vox.F, outputs["query_logits"], targets["labels"], class_weights, packed)

    def __repr__(self):
        head = "Matcher " + self.__class__.__name__
        body = ["cost_class: {}".format(self.cost_class), "cost_mask: {}".format(self.cost_mask),
                "cost_dice: {}".format(self.cost_dice)]
        return "\n".join([head] + [" " * 4 + line for line in body])


class SetCriterion(nn.Module):
    """Drop-in for the reference's criterion: the same constructor, the same `forward` signature, the same keys (`loss_ce`,
    `loss_mask`, `loss_dice`, `ssc_ce_loss`, `ssc_lovasz_loss`, `indices`, `loss_aux` with `_level{i}` keys), the same weights
    from `weight_dict` and the same per-batch-element means, the same buffers (`empty_weight`, `compl_labelweights`).

    `ssc_ce_loss` and `ssc_lovasz_loss` are returned as 0.0 whatever `weight_dict` says: the reference's `Net.step` never adds
    them to the loss it optimises.  `sem_logits_pruned_1_1` and `semantic_label` are accepted and not read.  With one target dict
    the whole sparse tensor is that batch element (no rows are compacted); with more, `features_at(i)` selects them.  The
    targets are packed once per batch element and the words are reused by the matcher, the loss and every `aux_outputs` level
    whose coordinates are the same tensor object.  `criterion.matched` holds the matches of the last call: one list per level
    (the main level first), one (src, tgt) per batch element."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, class_weights, compl_labelweights, alpha=0.1):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.eos_coef = eos_coef
        self.alpha = alpha
        self.class_weights = class_weights
        self.register_buffer("empty_weight", torch.ones(self.num_classes + 1))
        self.register_buffer("compl_labelweights", compl_labelweights)
        self.matched = []

    def loss_labels(self, query_logits, labels, indice, class_weight):
        src_idx, tgt_idx = indice
        target_classes = torch.full(query_logits.shape[:1], self.num_classes, dtype=torch.int64, device=query_logits.device)
        target_classes[src_idx.to(query_logits.device)] = labels[tgt_idx.to(labels.device)].long().to(query_logits.device)
        return F.cross_entropy(query_logits, target_classes, class_weight.to(query_logits.dtype), reduction="none")

    def _packed(self, cache, voxel_logits, i, bs, targets, unknown_mask_dense, min_C):
        c_all = voxel_logits.C
        key = (id(c_all), i)
        hit = cache.get(key)
        if hit is not None and hit[0] is c_all:
            return hit[1]
        if bs == 1:
            coords = c_all
        else:
            ci = voxel_logits.coordinates_at(i)
            coords = torch.cat([torch.zeros_like(ci[:, :1]), ci], dim=1)
        origin = (0, 0, 0) if min_C is None else [int(v) for v in torch.as_tensor(min_C).reshape(3).tolist()]
        unknown = None if unknown_mask_dense is None else unknown_mask_dense[0].to(coords.device)
        if hasattr(targets[i], "pack"):       # data.targets.TargetMasks: the words straight from the label grids, no [T, X, Y, Z]
            packed = targets[i].pack(coords, unknown, origin)
        else:
            packed = pack_targets(targets[i]["masks"].to(coords.device), unknown, coords, origin)
        cache[key] = (c_all, packed)
        return packed

    def compute_losses(self, outputs, targets, unknown_mask_dense, i_infer, min_C, cache):
        bs = len(targets)
        voxel_logits, query_logits = outputs["voxel_logits"], outputs["query_logits"]
        agg = {"loss_ce": 0, "loss_mask": 0, "loss_dice": 0}
        matched = []
        for i in range(bs):
            feats = voxel_logits.F if bs == 1 else voxel_logits.features_at(i)
            class_weight = self.class_weights[i_infer].to(feats.device)
            labels = targets[i]["labels"].to(feats.device)
            pred_logit = query_logits[i]
            packed = self._packed(cache, voxel_logits, i, bs, targets, unknown_mask_dense, min_C)
            _check_counts(int(feats.shape[1]), packed.t)
            indice = self.matcher.match_packed(feats, pred_logit, labels, class_weight, packed)
            matched.append(indice)
            src, tgt = indice
            loss_ce = self.loss_labels(pred_logit, labels, indice, class_weight)
            weights = class_weight[labels[tgt.to(labels.device)].long()]
            if packed.t == 0:
                loss_mask = loss_dice = feats.new_zeros(0)
            else:
                loss_mask, loss_dice = mask_losses(feats, packed, src, tgt, weights)
            agg["loss_ce"] = agg["loss_ce"] + (loss_ce * self.weight_dict["loss_ce"]).mean()
            agg["loss_mask"] = agg["loss_mask"] + (loss_mask * self.weight_dict["loss_mask"]).mean()
            agg["loss_dice"] = agg["loss_dice"] + (loss_dice * self.weight_dict["loss_dice"]).mean()
        out = {k: v / bs for k, v in agg.items()}
        out["ssc_ce_loss"] = 0.0
        out["ssc_lovasz_loss"] = 0.0
        return out, matched

    def forward(self, sem_logits_pruned_1_1, outputs, targets, semantic_label, unknown_mask_dense, i_infer, indices, min_C=None):
        cache = {}
        losses, matched = self.compute_losses({k: v for k, v in outputs.items() if k != "aux_outputs"}, targets,
                                              unknown_mask_dense, i_infer, min_C, cache)
        self.matched = [matched]
        loss_aux = {}
        for i, aux_outputs in enumerate(outputs.get("aux_outputs", ())):
            aux, matched = self.compute_losses(aux_outputs, targets, unknown_mask_dense, i_infer, min_C, cache)
            self.matched.append(matched)
            for k, v in aux.items():
                loss_aux[k + "_level{}".format(i)] = v
        losses["indices"] = indices
        losses["loss_aux"] = loss_aux
        return losses
