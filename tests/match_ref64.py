"""The matcher's cost and the mask losses (include/pasco_match.h) in the formulation the training code they replace uses,
written from the formulas - not from csrc/match.hip and not from pasco_amd/grad/host.py - in fp64 (the reference of the tests)
and in fp32 (the yardstick the tests weigh an error against), both in torch on the CPU.

    matcher, over the rows that are known and lie in at least one target (x = logits^T [Q, M], y = targets^T [T, M]):
        focal[q][t] = (einsum(0.25 (1-p)^2 bce(x, 1), y) + einsum(0.75 p^2 bce(x, 0), 1 - y)) / M          (0 when M == 0)
        dice[q][t]  = 1 - (2 einsum(p, y) + 1) / (sum p + sum y + 1)
        C = (focal + dice - softmax(query_logits)[:, labels]) * class_weights[labels]
    loss, over the known rows, for the matched pairs k = (src[k], tgt[k]) (x, y [M, K]):
        loss_mask[k] = w[k] mean_n alpha_t bce(x, y) (1 - p_t)^2,  p_t = p y + (1-p)(1-y),  alpha_t = 0.25 y + 0.75 (1-y)
        loss_dice[k] = w[k] (1 - (2 sum p y + 1) / (sum p + sum y + 1))
        dlogits by torch autograd of sum(g_mask loss_mask) + sum(g_dice loss_dice)

The precision rule of the tests, per tensor v:   max |v - v64| <= M * max |v32 - v64|   with v32 the fp32 yardstick.
M = about twice the worst ratio measured over all cases of tests/match_cases.py and the recorded scenes, rounded up.  Measured:
    on the MI355X (csrc/match.hip), 234 tensors:
        worst 2441.576 (focal at Q1 T1 N2, logits x 3: ONE element, err 2.9e-08 = half an ulp of the value, where the fp32
        yardstick happens to land 1.2e-11 from fp64), then 272.442 (loss_dice, Q1 T1 N2), 91.359 (dice, Q1 T1 N2), 52.519
        (loss_mask, Q31 T1 N65): every ratio above 3 belongs to a tensor of one or two elements        -> PM_M[0] = 5000
        worst over the tensors of >= 64 elements: 2.758 (dlogits at Q7 T3 N70, sparse), then 2.309, 2.071 -> PM_M[1] = 6
        the recorded scenes: losses 2.569, dlogits 1.729, dquery 1.084
        the long shapes (T = 65, 70, 96: three target tiles; N = 32 768 and 32 769: 256 ranges, ranges of 160 rows):
        worst 15.114 (loss_dice at Q7 T3 N32769, first_range_unknown: 3 elements), >= 64 elements 2.789 (dlogits, Q100 T96 N257)
    on the CPU (grad/host.py), 234 tensors:
        worst 2441.576 (the same one-element tensor), then 272.442, 91.359                               -> PM_HOST_M[0] = 5000
        worst over the tensors of >= 64 elements: 2.925 (dlogits at Q7 T3 N70, sparse), then 2.298, 2.260 -> PM_HOST_M[1] = 6
        the long shapes: worst 7.337 (the same 3-element loss_dice), >= 64 elements 2.789 (dlogits, Q100 T96 N257)
The rule is ill-conditioned on a one-element tensor: a correctly rounded fp32 result can be any multiple of a yardstick that
happens to be nearly exact.  So each constant is a pair: [0] is the measured bound for every tensor, as above; [1] is a SECOND,
tighter bound that a tensor of >= WIDE = 64 elements must meet as well (`bound_for`).
A tensor that is identically zero in fp64 is compared with zero instead (FP64_FLOOR below)."""
import torch
import torch.nn.functional as F

WIDE = 64
PM_M = (5000.0, 6.0)
PM_HOST_M = (5000.0, 6.0)
# "Identically zero in fp64" has one non-structural cause: at x = +80 the fp64 formulation forms 1 - sigmoid(x) by subtraction
# and gets 0 where the value is e^-80 = 1.8e-35, so a focal term or gradient of ~1e-36 is reported as 0.  The kernels form 1 - p
# without the subtraction and return that 1e-36.  A value the fp64 formulation cannot tell from zero - below its rounding unit
# 2^-53 on operands of size 1 - therefore counts as zero.  The STRUCTURAL zeros (unmatched columns, unknown rows, refused calls)
# are asserted bit-exact by the tests themselves, not through this rule.
FP64_FLOOR = 2.0 ** -53


def matcher_terms(logits, tgt, known, dtype):
    """logits [N, Q], tgt bool [N, T], known bool [N] -> (focal [Q, T], dice [Q, T], rows counted) in `dtype`."""
    valid = tgt.any(dim=1) & known
    x = logits.to(dtype).t()[:, valid]
    y = tgt.to(dtype).t()[:, valid]
    p = x.sigmoid()
    dice = 1 - (2 * torch.einsum("nc,mc->nm", p, y) + 1) / (p.sum(-1)[:, None] + y.sum(-1)[None, :] + 1)
    m = x.shape[1]
    if m == 0:
        return torch.zeros_like(dice), dice, 0
    pos = 0.25 * (1 - p) ** 2 * F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = 0.75 * p ** 2 * F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    focal = (torch.einsum("nc,mc->nm", pos, y) + torch.einsum("nc,mc->nm", neg, 1 - y)) / m
    return focal, dice, m


def matcher_cost(logits, tgt, known, query_logits, labels, class_weights, dtype):
    """The whole cost matrix [Q, T] in `dtype` (cost_mask = cost_class = cost_dice = 1)."""
    focal, dice, _ = matcher_terms(logits, tgt, known, dtype)
    cls = -query_logits.to(dtype).softmax(-1)[:, labels.long()]
    return (focal + cls + dice) * class_weights.to(dtype)[labels.long()][None, :]


def losses(logits, tgt, known, src, tgt_idx, w, g_mask, g_dice, dtype):
    """-> (loss_mask [K], loss_dice [K], dlogits [N, Q]) in `dtype`."""
    x_all = logits.detach().clone().to(dtype).requires_grad_(True)
    x = x_all[:, src][known]
    y = tgt[:, tgt_idx].to(dtype)[known]
    p = x.sigmoid()
    ce = F.binary_cross_entropy_with_logits(x, y, reduction="none")
    p_t = p * y + (1 - p) * (1 - y)
    focal = (0.25 * y + 0.75 * (1 - y)) * (ce * (1 - p_t) ** 2)
    loss_mask = (focal * w.to(dtype)[None, :]).mean(0)
    loss_dice = (1 - (2 * (p * y).sum(0) + 1) / (p.sum(0) + y.sum(0) + 1)) * w.to(dtype)
    dl = torch.zeros_like(x_all)
    if x.numel() > 0:
        (loss_mask * g_mask.to(dtype)).sum().add((loss_dice * g_dice.to(dtype)).sum()).backward()
        dl = x_all.grad
    return loss_mask.detach(), loss_dice.detach(), dl.detach()


def bound_for(M, numel):
    """M = (the bound for every tensor, the tighter one for a tensor of >= WIDE elements) -> the bound for `numel` elements."""
    return M[1] if numel >= WIDE else M[0]


def ratio_check(label, v, v64, v32, M):
    """Assert the rule above for one tensor and print its ratio.  NaN is allowed only where the fp64 value is NaN too."""
    v, v32, v64 = v.detach().double().cpu(), v32.detach().double().cpu(), v64.detach().double().cpu()
    assert v.shape == v64.shape, f"{label}: shape {tuple(v.shape)}, expected {tuple(v64.shape)}"
    nan = torch.isnan(v64)
    assert torch.equal(torch.isnan(v), nan), f"{label}: NaN where the fp64 value is not (or the reverse)"
    v, v32, v64 = v[~nan], v32[~nan], v64[~nan]
    assert bool(torch.isfinite(v).all()), f"{label}: not finite"
    if not bool(v64.any()):
        top = float(v.abs().max()) if v.numel() else 0.0
        print(f"PM_RATIO {label} exact-zero (max |v| = {top:.3e})")
        assert top <= FP64_FLOOR, f"{label}: identically zero in fp64, got max |v| = {top:.3e}"
        return 0.0
    err, yard = float((v - v64).abs().max()), float((v32 - v64).abs().max())
    r = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    M = bound_for(M, v.numel())
    print(f"PM_RATIO {label} {r:.3f}  (err {err:.3e}, fp32 yardstick {yard:.3e}, {v.numel()} elements, bound {M:g})")
    assert err <= M * yard, f"{label}: max |v - v64| = {err:.3e} = {r:.2f} x max |v32 - v64| ({yard:.3e}), bound {M}"
    return r
