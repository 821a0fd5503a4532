"""Independent fp64 reference of the attention family (include/pasco_hip.h: attn_cross_fwd, attn_cross_split,
attn_cross_feat, attn_mask_pack, bits_or_reduce, pos_aug), written from the definition of the operation - not from
csrc/attn.hip and not from oracle/pasco_oracle.c.  Plain torch fp64 and numpy integer arithmetic.

q, k and v must be finite: NaN or Inf in them is out of scope (softmax of such a row is undefined here as it is in the
kernels), and no case of tests/attn_edge_cases.py puts one there."""
import numpy as np
import torch

from pasco_amd.me.backend import SPLIT_ACT_EXP2

RTOL, ATOL = 1e-4, 2e-5            # the project's bound for inputs of unit scale (tests/test_hip_attn.py)


# ---- split operands ------------------------------------------------------------------------------------------------------------
def unsplit(op, c, exp2=SPLIT_ACT_EXP2):
    """split operand [rows, c/32, 2, 32] f16 -> the fp32 values it stands for."""
    x = op.float()
    return ((x[:, :, 0] + x[:, :, 1]).reshape(op.shape[0], c) * float(2.0 ** -exp2))


def unsplit64(op, c, exp2=SPLIT_ACT_EXP2):
    """The same in fp64: hi + lo of two f16 values is exact there."""
    x = op.double()
    return (x[:, :, 0] + x[:, :, 1]).reshape(op.shape[0], c) * 2.0 ** -exp2


def feat_rows(x_split, aug, B, N, exp2=SPLIT_ACT_EXP2):
    """Key rows of attn_cross_feat in fp64: r = [x | aug], both carrying the operand's 2^exp2 -> [B, N, c + 16]."""
    c = x_split.shape[1] * 32
    x = unsplit64(x_split, c, exp2).reshape(B, N, c)
    return torch.cat([x, aug.double().reshape(B, N, 16) * 2.0 ** -exp2], dim=-1)


# ---- attention -----------------------------------------------------------------------------------------------------------------
def attention(q, k, v, allow=None, any_given=True, per_head=True):
    """softmax(q k^T + mask) v per (b, h) in fp64.

    q [B, H, Q, D]; k, v [B, N, H * D] (per_head) or [B, N, D] shared by the heads; allow bool [B, N, Q] or None.
    A query with no allowed key attends everywhere when `any_given` (the OR over the keys is handed to the kernel), and
    gets zeros when it is not (include/pasco_hip.h).
    -> (out [B, Q, H * D], scale [B, Q, H * D]) with scale = sum_n p_n |v_n|, the magnitude the sum was formed at."""
    B, H, Q, D = q.shape
    N = k.shape[1]
    out = torch.zeros(B, Q, H * D, dtype=torch.float64, device=q.device)
    scale = torch.zeros_like(out)
    for b in range(B):
        al = None
        if allow is not None:
            al = allow[b].t()                                            # [Q, N]
            empty = ~al.any(dim=1)                                       # [Q]
            if any_given:
                al = al | empty[:, None]
        for h in range(H):
            sl = slice(h * D, (h + 1) * D) if per_head else slice(0, D)
            kk, vv = k[b, :, sl].double(), v[b, :, sl].double()
            s = q[b, h].double() @ kk.t()                                # [Q, N]
            if al is not None:
                s = s.masked_fill(~al, float("-inf"))
            m = s.max(dim=1, keepdim=True).values
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)      # nothing allowed: every p is 0
            p = torch.exp(s - m)
            l = p.sum(dim=1, keepdim=True)
            p = p / torch.where(l > 0, l, torch.ones_like(l))
            out[b, :, h * D:(h + 1) * D] = p @ vv
            scale[b, :, h * D:(h + 1) * D] = p @ vv.abs()
    return out, scale


def bound(exp, scale):
    """|got - exp| <= 1e-4 |exp| + 2e-5 max(1, scale): the project's bound, aware of the magnitude the sum was formed at."""
    return RTOL * exp.abs() + ATOL * torch.clamp(scale, min=1.0)


def ratio(got, exp, scale):
    """max |got - exp| / bound (inf where got is not finite)."""
    got = got.double().to(exp.device)
    r = (got - exp).abs() / bound(exp, scale)
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    return float(r.max())


def feat_ref(q2, x_split, aug, B, N, allow):
    """fp64 restatement of attn_cross_feat, rounded to fp32: Y = softmax(q2 r^T + mask) r on the rows r = [x | aug]."""
    r = feat_rows(x_split, aug, B, N)
    return attention(q2, r, r, allow, per_head=False)[0].float()


# ---- mask words ----------------------------------------------------------------------------------------------------------------
def mask_pack(vals, B, N, positive_only=False):
    """vals [B * N, Q] fp32 -> (bits int32 [B * N, 4], any int32 [B, 4]): bit q of a row's 128-bit word is set where the
    value is non-zero (NaN is non-zero; -0.0 is zero), or greater than zero under `positive_only` (NaN is not; the
    smallest denormal is).  Integer arithmetic in numpy."""
    x = np.asarray(vals.detach().cpu().numpy(), dtype=np.float32)
    rows, Q = x.shape
    assert rows == B * N and 1 <= Q <= 128
    with np.errstate(invalid="ignore"):
        on = (x > 0) if positive_only else (x != 0)
    words = np.zeros((rows, 4), dtype=np.uint64)
    for qi in range(Q):
        words[:, qi >> 5] |= on[:, qi].astype(np.uint64) << np.uint64(qi & 31)
    words = words.astype(np.uint32)
    any_ = np.bitwise_or.reduce(words.reshape(B, N, 4), axis=1) if N > 0 else np.zeros((B, 4), np.uint32)
    return torch.from_numpy(words.view(np.int32).copy()), torch.from_numpy(any_.astype(np.uint32).view(np.int32).copy())


def pos_aug(coords, eps, tab_lo, exp2=SPLIT_ACT_EXP2):
    """The formula in the comment above ph_pos_aug: aug[i] = ([c == 0] per axis, eps[c - tab_lo] per axis, 0 x 10) * 2^exp2
    as f16; a coordinate outside tab_lo .. tab_lo + tab_n - 1 takes the nearer edge of the table and is reported.
    -> (aug f16 [n, 16], outside bool [n])."""
    c = coords.detach().cpu().numpy().astype(np.int64)[:, 1:4]
    e = eps.detach().cpu().numpy().astype(np.float32)
    t = c - int(tab_lo)
    outside = (t < 0) | (t >= e.shape[0])
    t = np.clip(t, 0, e.shape[0] - 1)
    pow2 = np.float32(2.0 ** exp2)
    out = np.zeros((c.shape[0], 16), dtype=np.float16)
    out[:, 0:3] = np.where(c == 0, pow2, np.float32(0)).astype(np.float16)
    out[:, 3:6] = (e[t] * pow2).astype(np.float32).astype(np.float16)
    return torch.from_numpy(out), torch.from_numpy(outside.any(axis=1))


# ---- launch geometry -----------------------------------------------------------------------------------------------------------
def geometry(kind, B, H, Q, N):
    """What the host launch code of csrc/attn.hip makes of a shape: kind = 'fwd' (ph_attn_cross_fwd, 16-key tiles, one wave
    per key range, 2048 waves aimed at), 'split' or 'feat' (ph_attn_cross_split / ph_attn_cross_feat, 32-key tiles, one
    workgroup of four query-tile waves per key range and head, 512 workgroups aimed at).

    THIS IS A RESTATEMENT OF THOSE THREE LAUNCH FORMULAS AND HAS TO BE RE-READ WHENEVER THE LAUNCH CODE CHANGES.  It serves
    to choose inputs and to assert that the case table reaches every launch class - never to form an expected value.

    -> dict(tile, ntile, splits, tpw, last_range_tiles, live_waves, idle_groups, qp)
       live_waves : split / feat: waves of a workgroup that own at least one query; fwd: waves of the last workgroup that
                    own a key range (the others leave at once)
       idle_groups: split / feat: workgroups of the grid beyond B * splits (they leave before the first barrier);
                    fwd: waves of the last workgroup without a range"""
    assert kind in ("fwd", "split", "feat")
    bh = B * H
    if kind == "fwd":
        tile = 16
        ntile = (N + tile - 1) // tile
        splits = max(1, 2048 // bh)
        splits = min(splits, ntile)
        splits = (splits + 3) // 4 * 4
        tpw = max(1, (ntile + splits - 1) // splits)
        splits = (ntile + tpw - 1) // tpw
        waves = bh * splits
        live = waves % 4 or 4
        idle = 4 - live
    else:
        tile = 32
        ntile = (N + tile - 1) // tile
        splits = max(1, 512 // bh)
        splits = min(splits, ntile)
        tpw = (ntile + splits - 1) // splits
        splits = (ntile + tpw - 1) // tpw
        live = (Q + 31) // 32
        groups = B * splits
        idle = (groups + 7) // 8 * 8 - groups
    return dict(tile=tile, ntile=ntile, splits=splits, tpw=tpw, last_range_tiles=ntile - (splits - 1) * tpw,
                live_waves=live, idle_groups=idle, qp=64 if Q <= 64 else 128)
