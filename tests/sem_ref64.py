"""The semantic completion losses (include/pasco_semloss.h) in the formulation the training code they replace uses, written
from the formulas - not from csrc/semloss.hip and not from pasco_amd/grad/host.py - in fp64 (the reference of the tests) and in
fp32 (the yardstick the tests weigh an error against), both in torch on the CPU.

    rows: keep = min_C <= C[:, 1:4] <= max_C;  y = target[(C[:, 1:4] - min_C) // scale] of the kept rows
    ce     = cross_entropy(F, y, weight=w, ignore_index=255, reduction="mean")
    lovasz = mean over the classes c with a row y == c of dot(sort_desc(|[y == c] - softmax(F)_c|), lovasz_grad(fg sorted))
             lovasz_grad: gts = sum fg; inter = gts - cumsum(fg); union = gts + cumsum(1 - fg); jac = 1 - inter / union;
             jac[1:] -= jac[:-1]          (float cumsums and a difference, as the training code writes it)
             rows labelled 255 stay in: they are background for every class.
    `lovasz_with_perm` takes every class's order as given instead of sorting; `closed_form` is the integer form of the header.

The precision rule of the tests, per tensor v:   max |v - v64| <= M * max |v32 - v64|   with v32 the fp32 yardstick: the
formulation above in fp32 on the CPU, never the code under test.
M = about twice the worst ratio measured over all cases of tests/sem_cases.py and the recorded scenes, rounded up.  Measured:
    on the MI355X (csrc/semloss.hip), 698 tensors:
        worst 750.061 (ce at N1 C2 ties: ONE element, err 1.4e-06 = 2 ulp of a value of 17, where the fp32 yardstick happens to
        land 1.9e-09 from fp64), then 130.420 (lovasz, N2048 C19 all_present), 51.592 (ce_num, N1 C2 ties), 27.788 (lovasz, N2049
        C32): every ratio above 3 belongs to a tensor of at most 32 elements                              -> PS_M[0] = 1500
        worst over the tensors of >= 64 elements: 2.910 (recorded scene a, the CE gradient at scale 1), then 2.853 (err at N64
        C32 single_class), 2.634, 2.611 (dlogits/lovasz at N64 C32 outside)                                -> PS_M[1] = 6
        the long shapes (N = 65 537 and 131 077 at C = 3: two and three rows per thread of k_rows_part, 33 and 65 tiles; four
        patterns): worst 23.589 (lovasz, N131077 random: one element), >= 64 elements 1.396 (err, N131077 random).  Before
        k_rows_final folded the ranges' CE partials in fp64 the CE gradient at N131077 ties stood at 6.275: over PS_M[1].
    on the CPU (grad/host.py), 696 tensors:
        worst 750.061 (the same one-element tensor), then 93.696 (lovasz, N65 C2 ignore10), 51.592         -> PS_HOST_M[0] = 1500
        worst over the tensors of >= 64 elements: 4.392 (dlogits/ce at N2047 C20 ties), then 3.190 (err at N63 C20
        single_class), 2.515                                                                               -> PS_HOST_M[1] = 9
        the long shapes: worst 80.540 (ce, N131077 random: one element), >= 64 elements 1.396 (err, N131077 random)
    the recorded scenes' fp32 losses lie within 8.9e-08 relative of this module's fp64 values (the bound is 2^-16).
The rule is ill-conditioned on a tensor of a few elements: a correctly rounded fp32 result can be any multiple of a yardstick
that happens to be nearly exact.  So each constant is a pair: [0] is the measured bound for every tensor; [1] is a SECOND, tighter
bound that a tensor of >= WIDE = 64 elements must meet as well (`bound_for`).
A tensor that is identically zero in fp64 is compared with zero instead (FP64_FLOOR below)."""
import torch
import torch.nn.functional as F

WIDE = 64
PS_M = (1500.0, 6.0)
PS_HOST_M = (1500.0, 9.0)
# At logits of +-80 the fp64 softmax gives p = 1 - 3e-69 -> exactly 1 and 1 - p = 0, where a kernel that forms 1 - p without the
# subtraction may return e^-160 (0 in fp32 as well, but the rule is kept as tests/match_ref64.py has it).
FP64_FLOOR = 2.0 ** -53
IGNORE, OUTSIDE = 255, 254


def labels_of(coords, target, min_C, max_C, scale):
    """-> (keep bool [N], y int64 [kept rows]) by the training code's gather."""
    xyz = coords[:, 1:4].long()
    keep = ((xyz >= min_C.long().reshape(1, 3)) & (xyz <= max_C.long().reshape(1, 3))).all(dim=1)
    idx = torch.div(xyz[keep] - min_C.long().reshape(1, 3), scale, rounding_mode="floor")
    return keep, target[idx[:, 0], idx[:, 1], idx[:, 2]].long()


def lovasz_grad(fg_sorted):
    gts = fg_sorted.sum()
    inter = gts - fg_sorted.cumsum(0)
    union = gts + (1 - fg_sorted).cumsum(0)
    jac = 1.0 - inter / union
    if len(fg_sorted) > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def lovasz_terms(logits, y, dtype, perms=None):
    """-> (loss_c [C] (0 for an absent class), present, errors [C, N]) in `dtype`.  perms: None (sort here, descending) or
    int64 [C, N] = every class's order."""
    x = logits.to(dtype)
    p = F.softmax(x, dim=1)
    c = x.shape[1]
    loss_c = []
    errs = []
    present = 0
    for k in range(c):
        fg = (y == k).to(dtype)
        err = (fg - p[:, k]).abs()
        errs.append(err)
        if fg.sum() == 0:
            loss_c.append(x.new_zeros(()))
            continue
        present += 1
        if perms is None:
            err_sorted, perm = torch.sort(err, 0, descending=True)
        else:
            perm = perms[k]
            err_sorted = err[perm]
        loss_c.append(torch.dot(err_sorted, lovasz_grad(fg[perm])))
    return torch.stack(loss_c), present, (torch.stack(errs) if c else x.new_zeros((0, 0)))


def lovasz_with_perm(logits, y, perms, dtype):
    """The Lovasz terms along every class's GIVEN order: perms int64 [C, N] -> (loss_c [C], present, errors [C, N])."""
    return lovasz_terms(logits, y, dtype, perms)


def losses(logits, coords, target, min_C, max_C, scale, weights, dtype, perms=None, g_ce=1.0, g_lov=1.0):
    """One (scale, subnet) pair in `dtype` -> dict: ce, lovasz, loss_c, err [C, kept], keep, y, dlogits [N, C] (the gradient of
    g_ce * ce + g_lov * lovasz, zero rows outside the box).  perms int64 [C, kept] index the KEPT rows."""
    keep, y = labels_of(coords, target, min_C, max_C, scale)
    x_all = logits.detach().clone().to(dtype).requires_grad_(True)
    x = x_all[keep]
    if (y != IGNORE).any():
        ce = F.cross_entropy(x, y, weight=weights.to(dtype), ignore_index=IGNORE, reduction="mean")
    else:
        ce = x.sum() * float("nan")
    loss_c, present, err = lovasz_terms(x, y, dtype, perms)
    lov = loss_c.sum() / present if present else x.sum() * 0.0
    dl = torch.zeros_like(x_all)
    total = (ce * g_ce if g_ce != 0.0 else 0.0) + (lov * g_lov if g_lov != 0.0 else 0.0)
    if torch.is_tensor(total) and total.requires_grad:
        total.backward()
        dl = x_all.grad
    return {"ce": ce.detach(), "lovasz": lov.detach(), "loss_c": loss_c.detach(), "err": err.detach(), "keep": keep, "y": y,
            "dlogits": dl.detach(), "present": present}


def closed_form(err, y_sorted_fg, g):
    """The header's closed form for ONE class in fp64: err_sorted [M], fg bool [M] along the sorted order, g = the foreground
    rows -> (loss, increments [M])."""
    fg = y_sorted_fg.to(torch.int64)
    cf = fg.cumsum(0)
    i1 = torch.arange(1, len(fg) + 1, dtype=torch.int64)
    u = (g + i1 - cf).double()
    inc = torch.where(fg.bool(), 1.0 / u, (g - cf).double() / ((u - 1.0) * u))
    return torch.dot(err.double(), inc), inc


def bound_for(M, numel):
    return M[1] if numel >= WIDE else M[0]


def ratio_check(label, v, v64, v32, M):
    """Assert the rule above for one tensor and print its ratio.  NaN is allowed only where the fp64 value is NaN too."""
    v, v32, v64 = (torch.as_tensor(t).detach().double().cpu() for t in (v, v32, v64))
    assert v.shape == v64.shape, f"{label}: shape {tuple(v.shape)}, expected {tuple(v64.shape)}"
    nan = torch.isnan(v64)
    assert torch.equal(torch.isnan(v), nan), f"{label}: NaN where the fp64 value is not (or the reverse)"
    v, v32, v64 = v[~nan], v32[~nan], v64[~nan]
    assert bool(torch.isfinite(v).all()), f"{label}: not finite"
    if not bool(v64.any()):
        top = float(v.abs().max()) if v.numel() else 0.0
        print(f"PS_RATIO {label} exact-zero (max |v| = {top:.3e})")
        assert top <= FP64_FLOOR, f"{label}: identically zero in fp64, got max |v| = {top:.3e}"
        return 0.0
    err, yard = float((v - v64).abs().max()), float((v32 - v64).abs().max())
    r = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    M = bound_for(M, v.numel())
    print(f"PS_RATIO {label} {r:.3f}  (err {err:.3e}, fp32 yardstick {yard:.3e}, {v.numel()} elements, bound {M:g})")
    assert err <= M * yard, f"{label}: max |v - v64| = {err:.3e} = {r:.2f} x max |v32 - v64| ({yard:.3e}), bound {M}"
    return r
