"""The masked cross-attention with a gradient: `ph_attn_cross_fwd` forward, `pa_attn_cross_bwd` (include/pasco_attngrad.h)
backward, and a layer a trainer can put in the place of the reference's `CrossAttentionLayer`
(pasco/models/transformer/blocks.py:47-92).  Neither direction forms the [B*H, Q, N] score tensor.

`AttnCrossFunction.forward` is the one launch `graph/transformer.py` makes, so the values are the same bits with and without
autograd; only the `grad_fn` is new.  The row statistics are recomputed in the backward, not saved.  Once differentiable: no
double backward.  Served: head dimension 48, at most 128 queries, no `padding_mask`, no attention dropout in training mode."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import grad as G
from ..me.autograd import wants_grad
from ..me.backend import backend_for

HEAD_DIM = 48
MAX_QUERIES = 128


class AttnCrossFunction(torch.autograd.Function):
    """out [B,Q,H*Dh] = softmax(q4 k^T + mask) v per (b, h): q4 [B,H,Q,Dh] pre-scaled, k / v [B,N,H*Dh], bits int32 [B,N,4] | None,
    any int32 [B,4] | None.  The mask carries no gradient."""

    @staticmethod
    def forward(ctx, q4, k, v, bits, any_, be):
        q4, k, v = q4.contiguous(), k.contiguous(), v.contiguous()
        out = be.attn_cross_fwd(q4, k, v, bits, any_)
        ctx.save_for_backward(q4, k, v, out)
        ctx.bits, ctx.any_ = bits, any_
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q4, k, v, out = ctx.saved_tensors
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        dq = dk = dv = None
        if need_q or need_k or need_v:
            dq, dk, dv = G.attn_cross_bwd(q4, k, v, ctx.bits, ctx.any_, out, dout.contiguous(), need_q, need_k, need_v)
        return dq, dk, dv, None, None, None


def masked_cross_attention(q4: torch.Tensor, k: torch.Tensor, v: torch.Tensor, mask_bits=None) -> torch.Tensor:
    """q4 [B,H,Q,48] (already scaled by 1/sqrt(48)), k / v [B,N,H*48], mask_bits = (bits int32 [B,N,4], any int32 [B,4] | None)
    or None -> [B,Q,H*48].  Differentiable in q4, k and v when autograd wants it; otherwise the plain launch."""
    dh, qn = int(q4.shape[-1]), int(q4.shape[-2])
    if dh != HEAD_DIM or qn > MAX_QUERIES:
        raise ValueError(f"masked_cross_attention serves head dimension {HEAD_DIM} and at most {MAX_QUERIES} queries "
                         f"(got head dimension {dh}, {qn} queries)")
    bits, any_ = (None, None) if mask_bits is None else mask_bits
    assert bits is not None or any_ is None, "mask_bits: `any` without `bits`"
    be = backend_for(q4.device)
    if wants_grad(q4, k, v):
        return AttnCrossFunction.apply(q4, k, v, bits, any_, be)
    return be.attn_cross_fwd(q4.contiguous(), k.contiguous(), v.contiguous(), bits, any_)


class CrossAttentionLayer(nn.Module):
    """Drop-in for the reference's layer: the same parameters under the same names (`multihead_attn.in_proj_weight`,
    `multihead_attn.in_proj_bias`, `multihead_attn.out_proj.weight`, `multihead_attn.out_proj.bias`, `norm.weight`, `norm.bias`),
    the same forward signature, plus the keyword `mask_bits`.  `nn.MultiheadAttention` only holds the parameters: the
    projections are `F.linear` (torch differentiates them) and the attention is `masked_cross_attention`."""

    def __init__(self, d_model, nhead, dropout=0.0):
        super().__init__()
        if d_model != nhead * HEAD_DIM:
            raise ValueError(f"CrossAttentionLayer serves head dimension {HEAD_DIM} only: d_model = {d_model} with {nhead} heads "
                             f"has head dimension {d_model / nhead:g}")
        self.multihead_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.norm = nn.LayerNorm(d_model)
        self.nhead = nhead
        self.p_dropout = float(dropout)
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, q_embed, bb_feat, attn_mask=None, padding_mask=None, pos=None, query_pos=None, *, mask_bits=None):
        """q_embed [B,Q,D], bb_feat [B,N,D] -> [B,Q,D].  The mask is either `attn_mask`, bool [B*H,Q,N] with True = masked and
        equal across the heads of a batch element (head 0 is read), or `mask_bits` = (bits [B,N,4], any [B,4] | None) as
        `ph_attn_mask_pack` makes them.  With `attn_mask`, or with `any` given, a query that is masked everywhere attends
        everywhere (what the reference's caller makes of such a row, transformer_predictor_v2.py:164)."""
        if padding_mask is not None:
            raise NotImplementedError("CrossAttentionLayer: padding_mask is not served")
        assert self.p_dropout == 0.0 or not self.training, "CrossAttentionLayer: dropout > 0 in training mode is not served"
        assert attn_mask is None or mask_bits is None, "CrossAttentionLayer: attn_mask and mask_bits are alternatives"
        mha = self.multihead_attn
        q = self.norm(q_embed)
        B, Q, D = q.shape
        H = self.nhead
        N = bb_feat.shape[1]
        w, b = mha.in_proj_weight, mha.in_proj_bias
        kv = bb_feat if pos is None else bb_feat + pos
        qq = F.linear(q if query_pos is None else q + query_pos, w[:D], b[:D])
        kk = F.linear(kv, w[D:2 * D], b[D:2 * D])
        vv = F.linear(kv, w[2 * D:], b[2 * D:])
        if attn_mask is not None:
            assert attn_mask.dtype == torch.bool and tuple(attn_mask.shape) == (B * H, Q, N), "attn_mask: bool [B*H, Q, N]"
            allow = ~attn_mask.view(B, H, Q, N)[:, 0]                                        # [B, Q, N]
            vals = allow.transpose(1, 2).reshape(B * N, Q).to(torch.float32).contiguous()
            mask_bits = backend_for(q.device).attn_mask_pack(vals, B, N)
        q4 = qq.view(B, Q, H, HEAD_DIM).transpose(1, 2) * (float(HEAD_DIM) ** -0.5)
        o = masked_cross_attention(q4, kk, vv, mask_bits)
        return q + F.linear(o, mha.out_proj.weight, mha.out_proj.bias)
