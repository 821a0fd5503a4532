"""fp64 gradients of the masked cross-attention (include/pasco_attngrad.h), written from the formulas of the operation - not from
csrc/attn_grad.hip and not from pasco_amd/grad/host.py - and the fp32 yardstick they are weighed against: torch autograd of the
materialised formulation on the CPU.

    P = softmax(q k^T + mask),  delta[q] = sum_d dout[q][d] out[q][d]
    dV = P^T dout,  dP = dout v^T,  dS = P (dP - delta),  dK = dS^T q,  dQ = dS k

The precision rule of the tests, per tensor g of (dq, dk, dv):   max |g - g64| <= M * max |g32 - g64|
with g32 the yardstick.  M = 4 x the worst ratio measured, rounded up (DESIGN.md 4m lists the measured values):
    on the MI355X, kernels and layer:   worst 3.018 (dk at B1 H1 Q16 N16, mask without `any`); layer 2.486   -> ATTN_GRAD_M = 13
    on the CPU, grad/host.py and layer: worst 2.271 (dq at B1 H1 Q16 N16, no mask); layer 1.127               -> ATTN_GRAD_HOST_M = 10
A tensor whose fp64 gradient is identically zero is compared for equality instead."""
import torch

from tests import attn_ref64 as ref

ATTN_GRAD_M = 13.0
ATTN_GRAD_HOST_M = 10.0
LSE_ATOL = 1e-4       # lse = log sum exp(s): s is a 48-term fp32 dot product of |q k| ~ 0.15 each (error < 48 x 2^-24 x 7 = 2e-5), the
                      # log-sum-exp of up to 4101 terms adds a few ulp of |lse| < 10 (1e-6 each): 1e-4 covers both with room


def effective_allow(allow, any_given):
    """allow bool [B, N, Q] | None -> (al bool [B, Q, N] | None, dead bool [B, Q]): the mask the kernels apply, and the queries
    that attend nowhere (only without `any`)."""
    if allow is None:
        return None, None
    al = allow.transpose(1, 2)
    empty = ~al.any(dim=2)
    if any_given:
        return al | empty[:, :, None], torch.zeros_like(empty)
    return al, empty


def grads64(q, k, v, allow, any_given, dout):
    """-> (dq [B,H,Q,D], dk [B,N,H*D], dv [B,N,H*D], out [B,Q,H*D]) in fp64 from the formulas above."""
    B, H, Q, D = q.shape
    q, k, v, dout = q.double(), k.double(), v.double(), dout.double()
    al, dead = effective_allow(allow, any_given)
    out, _ = ref.attention(q, k, v, allow, any_given)
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(k), torch.zeros_like(v)
    for b in range(B):
        for h in range(H):
            sl = slice(h * D, (h + 1) * D)
            s = q[b, h] @ k[b, :, sl].t()
            if al is not None:
                s = s.masked_fill(~al[b], float("-inf"))
            m = s.max(dim=1, keepdim=True).values
            m = torch.where(torch.isinf(m), torch.zeros_like(m), m)
            p = torch.exp(s - m)
            l = p.sum(dim=1, keepdim=True)
            p = p / torch.where(l > 0, l, torch.ones_like(l))                  # a dead row: every p is 0
            do = dout[b, :, sl]
            delta = (do * out[b, :, sl]).sum(dim=1, keepdim=True)
            ds = p * (do @ v[b, :, sl].t() - delta)
            dv[b, :, sl] = p.t() @ do
            dk[b, :, sl] = ds.t() @ q[b, h]
            dq[b, h] = ds @ k[b, :, sl]
    return dq, dk, dv, out


def grads32(q, k, v, allow, any_given, dout):
    """The yardstick: torch fp32 autograd of the materialised formulation on the CPU -> (dq, dk, dv).  A dead query (nothing
    allowed, no `any`) would be a softmax over -inf only; it is given an unmasked row and its output row is multiplied by 0."""
    B, H, Q, D = q.shape
    N = k.shape[1]
    q, k, v = (t.detach().clone().float().requires_grad_(True) for t in (q, k, v))
    al, dead = effective_allow(allow, any_given)
    s = torch.matmul(q, k.view(B, N, H, D).permute(0, 2, 3, 1))                # [B, H, Q, N]
    if al is not None:
        s = s.masked_fill(~(al | dead[:, :, None])[:, None], float("-inf"))
    o = torch.matmul(torch.softmax(s, dim=-1), v.view(B, N, H, D).transpose(1, 2))
    if al is not None:
        o = o * (~dead)[:, None, :, None].float()
    o.transpose(1, 2).reshape(B, Q, H * D).backward(dout.float())
    return q.grad, k.grad, v.grad


def ratio_check(label, g, g64, g32, M):
    """Assert the rule above for one tensor and print its ratio."""
    g, g32 = g.detach().double().cpu(), g32.detach().double().cpu()
    assert bool(torch.isfinite(g).all()), f"{label}: not finite"
    if not bool(g64.any()):
        print(f"ATTN_GRAD_RATIO {label} exact-zero")
        assert not bool(g.any()), f"{label}: the fp64 gradient is identically zero, got max |g| = {float(g.abs().max()):.3e}"
        return 0.0
    err, yard = float((g - g64).abs().max()), float((g32 - g64).abs().max())
    r = err / yard if yard > 0 else (0.0 if err == 0 else float("inf"))
    print(f"ATTN_GRAD_RATIO {label} {r:.3f}  (err {err:.3e}, fp32 autograd {yard:.3e})")
    assert err <= M * yard, f"{label}: max |g - g64| = {err:.3e} = {r:.2f} x max |g32 - g64| ({yard:.3e}), bound {M}"
    return r
