"""Cases of the attention backward (include/pasco_attngrad.h), shared by tests/test_attn_grad_cpu.py (forward on the C oracle,
backward by pasco_amd/grad/host.py) and tests/test_hip_attn_grad.py (libpascohip.so).  A `Runner` hides the difference.

Operands are tests.attn_edge_cases.Problem (unit scale), mask words are attn_ref64.mask_pack, `dout` is randn from a seeded
generator.  References (tests/attn_grad_ref64.py) are computed once per (shape, pattern) and shared; nobody writes to them.

`bwd_geometry` restates the launch arithmetic of csrc/attn_grad.hip (pa_ranges and the grid).  IT HAS TO BE RE-READ WHENEVER THAT
CODE CHANGES.  It serves to choose shapes and to assert at import that the table reaches every launch class - never to form an
expected value."""
import functools

import torch

from tests import attn_grad_ref64 as gref
from tests import attn_ref64 as ref
from tests.attn_edge_cases import DH, Problem

# (B, H, Q, N): the smallest shapes that reach each launch class
SHAPES = [
    (1, 1, 1, 1),          # one key, one query: a single partial tile, three idle waves
    (1, 1, 16, 16),        # exactly one full tile of each
    (1, 2, 17, 15),        # Q = 17: a second query tile with one query; N = 15: a partial key tile
    (1, 2, 40, 50),        # 3 query tiles: the 4-tile instantiation
    (1, 1, 100, 17),       # the decoder's 100 queries (7 tiles in the 8-tile instantiation); 2 ranges, the last with 1 key
    (1, 1, 128, 83),       # Q = 128; 6 ranges of one tile, the last partial
    (2, 8, 100, 333),      # B * H = 16; 21 ranges: 3 idle waves in the last workgroup of every (b, h)
    (2, 8, 65, 4101),      # 257 tiles in 86 ranges of 3, the last range 2 tiles, the last tile 5 keys
]
MULTI = (2, 8, 65, 4101)
PATTERNS = ("plain", "mask_any", "mask_noany")


def bwd_geometry(B, H, Q, N):
    bh = B * H
    ntile = (N + 15) // 16
    splits = 2048 // bh
    if splits >= 4:
        splits -= splits % 4
    splits = min(max(1, splits), ntile)
    tpw = max(1, (ntile + splits - 1) // splits)
    splits = (ntile + tpw - 1) // tpw
    qtiles = (Q + 15) // 16
    return dict(ntile=ntile, splits=splits, tpw=tpw, last_range_tiles=ntile - (splits - 1) * tpw, idle_waves=-splits % 4,
                qtiles=qtiles, inst=1 if qtiles <= 1 else 2 if qtiles <= 2 else 4 if qtiles <= 4 else 8)


def _check_table():
    ge = {s: bwd_geometry(*s) for s in SHAPES}
    assert any(x["ntile"] == 1 for x in ge.values()), "a single tile"
    assert any(s[3] % 16 for s in SHAPES) and any(s[3] % 16 == 0 for s in SHAPES), "a partial and a full last tile"
    assert any(x["tpw"] > 1 for x in ge.values()), "more than one tile per range"
    assert any(x["tpw"] > 1 and x["last_range_tiles"] < x["tpw"] for x in ge.values()), "a shorter last range"
    assert any(x["idle_waves"] > 0 and x["splits"] > 4 for x in ge.values()), "idle waves in the last of several workgroups"
    assert {x["inst"] for x in ge.values()} == {1, 2, 4, 8}, "every instantiation"
    qs = {s[2] for s in SHAPES}
    assert {1, 16, 17} <= qs and any(64 < q <= 128 for q in qs) and 128 in qs
    g = ge[MULTI]
    assert g["splits"] > 1 and g["tpw"] == 3 and g["last_range_tiles"] == 2


_check_table()


# ---- inputs and references ---------------------------------------------------------------------------------------------------
class Inputs:
    def __init__(self, shape, pattern, seed=None):
        B, H, Q, N = shape
        self.shape, self.pattern = shape, pattern
        p = Problem(B, H, Q, N, seed=7000 + 13 * N + Q if seed is None else seed)
        self.q, self.k, self.v = p.q.contiguous(), p.k.contiguous(), p.v.contiguous()
        self.dout = torch.randn(B, Q, H * DH, generator=p.g)
        self.allow = None if pattern == "plain" else p.random_allow(0.3)       # one query allowed nowhere (query 3 % Q)
        self.any_given = pattern != "mask_noany"
        self.p = p

    def words(self):
        """-> (bits int32 [B, N, 4] | None, any int32 [B, 4] | None) on the CPU."""
        if self.allow is None:
            return None, None
        B, H, Q, N = self.shape
        bits, any_ = ref.mask_pack(self.allow.reshape(B * N, Q).float(), B, N)
        return bits.view(B, N, 4).contiguous(), (any_.contiguous() if self.any_given else None)

    @functools.cached_property
    def g64(self):
        return gref.grads64(self.q, self.k, self.v, self.allow, self.any_given, self.dout)

    @functools.cached_property
    def g32(self):
        return gref.grads32(self.q, self.k, self.v, self.allow, self.any_given, self.dout)


@functools.lru_cache(maxsize=None)
def inputs(shape, pattern):
    return Inputs(shape, pattern)


class Runner:
    """fwd(q, k, v, bits, any) -> out and bwd(q, k, v, bits, any, out, dout, need_q, need_k, need_v) -> (dq, dk, dv) on `dev`."""

    def __init__(self, dev, fwd, bwd, M, name):
        self.dev, self.fwd, self.bwd, self.M, self.name = dev, fwd, bwd, M, name

    def grads(self, x: Inputs, bits="default", any_="default", need=(True, True, True)):
        d = self.dev
        b0, a0 = x.words()
        bits = b0 if isinstance(bits, str) else bits
        any_ = a0 if isinstance(any_, str) else any_
        mv = lambda t: None if t is None else t.to(d).contiguous()
        q, k, v, dout, bits, any_ = (mv(t) for t in (x.q, x.k, x.v, x.dout, bits, any_))
        out = self.fwd(q, k, v, bits, any_)
        return self.bwd(q, k, v, bits, any_, out, dout, *need)


def check_precision(r: Runner, shape, pattern):
    x = inputs(shape, pattern)
    got = r.grads(x)
    worst = 0.0
    for name, g, g64, g32 in zip(("dq", "dk", "dv"), got, x.g64[:3], x.g32):
        worst = max(worst, gref.ratio_check(f"{r.name} B{shape[0]} H{shape[1]} Q{shape[2]} N{shape[3]} {pattern} {name}", g, g64, g32,
                                            r.M))
    if pattern == "mask_noany":          # the query allowed nowhere: an exact zero dq row
        assert not bool(got[0][:, :, 3 % shape[2]].any()), "dq row of a query with no allowed key"
    return worst


def check_dead_query_equals_its_removal():
    """The reference itself: with `any` == NULL, dk and dv are those of the problem without the dead query."""
    shape = (1, 2, 17, 15)
    x = inputs(shape, "mask_noany")
    dead = 3 % shape[2]
    keep = [i for i in range(shape[2]) if i != dead]
    dq2, dk2, dv2, _ = gref.grads64(x.q[:, :, keep], x.k, x.v, x.allow[:, :, keep], False, x.dout[:, keep])
    assert torch.equal(dk2, x.g64[1]) and torch.equal(dv2, x.g64[2]) and torch.equal(dq2, x.g64[0][:, :, keep])
    assert not bool(x.g64[0][:, :, dead].any())


def check_unattended_keys(r: Runner):
    """Keys allowed for no query, every query allowed somewhere (nothing is forced): their dk and dv rows are exact zeros."""
    shape = (2, 8, 100, 333)
    B, H, Q, N = shape
    x = Inputs(shape, "mask_any", seed=91)
    x.allow = torch.rand(B, N, Q, generator=x.p.g) < 0.3
    x.allow[:, 0] = True                                     # every query has key 0
    off = [5, 16, 17, 31, 100, 320, 321, N - 1]              # whole-tile neighbours, tile edges, the last key
    x.allow[:, off] = False
    dq, dk, dv = r.grads(x)
    for name, g, g64, g32 in zip(("dq", "dk", "dv"), (dq, dk, dv), x.g64[:3], x.g32):
        gref.ratio_check(f"{r.name} unattended_keys {name}", g, g64, g32, r.M)
    assert not bool(dk[:, off].any()) and not bool(dv[:, off].any())
    assert bool(dk[:, 6].any()) and bool(dv[:, 6].any())


def check_garbage_bits(r: Runner):
    """Stray ones at bit positions >= Q, in the key words and in `any`, change no bit of any gradient."""
    shape = (2, 8, 100, 333)
    B, H, Q, N = shape
    x = inputs(shape, "mask_any")
    bits, any_ = x.words()
    high = torch.zeros(4, dtype=torch.int64)
    for pos in range(Q, 128):
        high[pos >> 5] |= 1 << (pos & 31)
    high = high.to(torch.int32)
    g = torch.Generator().manual_seed(5)
    junk = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, N, 4), generator=g, dtype=torch.int64).to(torch.int32)
    clean = r.grads(x)
    dirty = r.grads(x, bits=bits | (junk & high), any_=any_ | high)
    for name, a, b in zip(("dq", "dk", "dv"), clean, dirty):
        assert torch.equal(a, b), name
    dirty = r.grads(x, bits=bits | (junk & high), any_=None)               # and with any == NULL
    clean = r.grads(x, any_=None)
    for name, a, b in zip(("dq", "dk", "dv"), clean, dirty):
        assert torch.equal(a, b), name


def check_masked_range_start(r: Runner):
    """Key ranges whose first tiles are entirely masked (the m = -inf start of the statistics pass): range 0 (keys 0 .. 47) has
    its first two tiles masked, an interior range all three, for every query."""
    B, H, Q, N = MULTI
    ge = bwd_geometry(*MULTI)
    span = ge["tpw"] * 16
    x = Inputs(MULTI, "mask_any", seed=92)
    x.allow = torch.rand(B, N, Q, generator=x.p.g) < 0.3
    x.allow[:, :32] = False
    x.allow[:, 40 * span:41 * span] = False
    x.allow[:, 41 * span:41 * span + 16] = False
    x.allow[:, N - 1] = True                                 # nobody is forced
    got = r.grads(x)
    for name, g, g64, g32 in zip(("dq", "dk", "dv"), got, x.g64[:3], x.g32):
        gref.ratio_check(f"{r.name} masked_range_start {name}", g, g64, g32, r.M)
    assert not bool(got[1][:, :32].any()) and not bool(got[2][:, 40 * span:41 * span].any())


# ---- autograd and the layer --------------------------------------------------------------------------------------------------
def check_autograd_route(be, dev, M):
    """Through masked_cross_attention an input that requires grad gets a grad_fn; without one, or under no_grad, there is none;
    the values are the bits of be.attn_cross_fwd in every mode."""
    from pasco_amd.grad.attention import masked_cross_attention
    x = inputs((1, 2, 17, 15), "mask_any")
    bits, any_ = (t.to(dev) for t in x.words())
    q, k, v = (t.to(dev) for t in (x.q, x.k, x.v))
    plain = be.attn_cross_fwd(q, k, v, bits, any_)
    out = masked_cross_attention(q, k, v, (bits, any_))
    assert out.grad_fn is None and torch.equal(out, plain)
    for which in range(3):
        ts = [t.clone().requires_grad_(i == which) for i, t in enumerate((q, k, v))]
        out = masked_cross_attention(*ts, (bits, any_))
        assert out.grad_fn is not None and torch.equal(out.detach(), plain)
        with torch.no_grad():
            out2 = masked_cross_attention(*ts, (bits, any_))
        assert out2.grad_fn is None and torch.equal(out2, plain)
        out.backward(x.dout.to(dev))
        for i, t in enumerate(ts):
            assert (t.grad is not None) == (i == which)
    # all three at once: the gradients are the library's
    ts = [t.clone().requires_grad_(True) for t in (q, k, v)]
    masked_cross_attention(*ts, (bits, any_)).backward(x.dout.to(dev))
    for name, t, g64, g32 in zip(("dq", "dk", "dv"), ts, x.g64[:3], x.g32):
        gref.ratio_check(f"autograd {name}", t.grad, g64, g32, M)
    with_bad = q[..., :32].contiguous()
    try:
        masked_cross_attention(with_bad, k[..., :64].contiguous(), v[..., :64].contiguous())
    except ValueError as e:
        assert "48" in str(e)
    else:
        raise AssertionError("head dimension 32 was accepted")


class RefLayer(torch.nn.Module):
    """The reference's layer restated on nn.MultiheadAttention: norm, MHA with attn_mask, residual (blocks.py:73-92)."""

    def __init__(self, d_model, nhead):
        super().__init__()
        self.multihead_attn = torch.nn.MultiheadAttention(d_model, nhead, dropout=0.0, batch_first=True)
        self.norm = torch.nn.LayerNorm(d_model)

    def forward(self, q_embed, bb_feat, attn_mask=None, pos=None, query_pos=None):
        q = self.norm(q_embed)
        kv = bb_feat if pos is None else bb_feat + pos
        y = self.multihead_attn(query=q if query_pos is None else q + query_pos, key=kv, value=kv, attn_mask=attn_mask)[0]
        return q + y


LAYER = dict(d_model=384, nhead=8, B=2, Q=100, N=333)


@functools.lru_cache(maxsize=None)
def layer_problem():
    """Inputs, the reference module's state, and its fp64 / fp32 results on the CPU."""
    c = LAYER
    g = torch.Generator().manual_seed(4242)
    D, H, B, Q, N = c["d_model"], c["nhead"], c["B"], c["Q"], c["N"]
    m = RefLayer(D, H)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[0] + p.shape[1])) ** 0.5)
            else:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    t = dict(q_embed=torch.randn(B, Q, D, generator=g), bb_feat=torch.randn(B, N, D, generator=g),
             pos=0.5 * torch.randn(B, N, D, generator=g), query_pos=0.5 * torch.randn(B, Q, D, generator=g),
             w_out=torch.randn(B, Q, D, generator=g))
    mask = torch.rand(B, Q, N, generator=g) < 0.7                            # True = masked
    mask[:, 3] = True                                                          # a query masked everywhere ...
    mask[mask.sum(-1) == N] = False                                            # ... and the caller's fix (predictor_v2.py:164)
    attn_mask = mask[:, None].expand(B, H, Q, N).reshape(B * H, Q, N).contiguous()
    res = {}
    for dt in (torch.float64, torch.float32):
        mm = RefLayer(D, H).to(dt)
        mm.load_state_dict({k: v.to(dt) for k, v in m.state_dict().items()})
        qe, bf = (t[n].to(dt).clone().requires_grad_(True) for n in ("q_embed", "bb_feat"))
        out = mm(qe, bf, attn_mask, t["pos"].to(dt), t["query_pos"].to(dt))
        (out * t["w_out"].to(dt)).sum().backward()
        res[dt] = dict(out=out.detach(), q_embed=qe.grad, bb_feat=bf.grad, **{k: p.grad for k, p in mm.named_parameters()})
    return m.state_dict(), t, attn_mask, res


def check_layer(dev, M, label):
    from pasco_amd.grad.attention import CrossAttentionLayer
    from pasco_amd.me.backend import backend_for
    c = LAYER
    state, t, attn_mask, res = layer_problem()
    layer = CrossAttentionLayer(c["d_model"], c["nhead"]).to(dev)
    assert sorted(layer.state_dict()) == sorted(state) == sorted(
        ["multihead_attn.in_proj_weight", "multihead_attn.in_proj_bias", "multihead_attn.out_proj.weight",
         "multihead_attn.out_proj.bias", "norm.weight", "norm.bias"])
    layer.load_state_dict(state, strict=True)
    layer.train()
    qe, bf = (t[n].to(dev).clone().requires_grad_(True) for n in ("q_embed", "bb_feat"))
    pos, qpos, am = t["pos"].to(dev), t["query_pos"].to(dev), attn_mask.to(dev)
    out = layer(qe, bf, am, None, pos, qpos)
    assert out.grad_fn is not None
    (out * t["w_out"].to(dev)).sum().backward()
    got = dict(out=out.detach(), q_embed=qe.grad, bb_feat=bf.grad, **{k: p.grad for k, p in layer.named_parameters()})
    r64, r32 = res[torch.float64], res[torch.float32]
    assert len(got) == 9
    for name in got:
        gref.ratio_check(f"{label} layer {name}", got[name], r64[name], r32[name], M)
    # the same mask as words: identical bits
    B, Q, N = c["B"], c["Q"], c["N"]
    allow = ~attn_mask.view(B, c["nhead"], Q, N)[:, 0]
    words = backend_for(torch.device(dev)).attn_mask_pack(allow.transpose(1, 2).reshape(B * N, Q).float().contiguous().to(dev), B, N)
    with torch.no_grad():
        out2 = layer(qe, bf, None, None, pos, qpos, mask_bits=words)
    assert torch.equal(out2, out.detach())
    # what is not served says so
    for bad, exc in ((lambda: layer(qe, bf, am, torch.zeros(B, N, dtype=torch.bool, device=dev), pos, qpos), NotImplementedError),
                     (lambda: CrossAttentionLayer(256, 8), ValueError)):
        try:
            bad()
        except exc as e:
            assert exc is NotImplementedError or "48" in str(e)
        else:
            raise AssertionError("an unserved configuration was accepted")
    drop = CrossAttentionLayer(c["d_model"], c["nhead"], dropout=0.1).to(dev)
    drop.train()
    try:
        drop(qe, bf, am, None, pos, qpos)
    except AssertionError as e:
        assert "dropout" in str(e)
    else:
        raise AssertionError("dropout > 0 in training mode was accepted")
