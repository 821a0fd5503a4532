"""Edge cases of the attention family (csrc/attn.hip: k_attn_cross, k_attn_split, k_attn_feat, k_attn_merge, k_mask_pack,
k_bits_or_reduce, k_pos_aug), each a function of (be, dev): `be` is the C oracle on the CPU (tests/test_attn_edges_cpu.py) or
libpascohip.so on the GPU (tests/test_hip_attn_edges.py).  Every case runs the three attention entry points on one shape and
holds each to the fp64 reference of tests/attn_ref64.py:

    |got - exp| <= 1e-4 |exp| + 2e-5 max(1, scale),   scale = sum_n p_n |v_n| from the reference

(for inputs of unit scale: the assertion of tests/test_hip_attn.py).  Each comparison prints `max |got - exp| / bound`.
Integer results - mask words, position columns, status bits, bit-equality of two calls - are compared for equality.  Every
launch gets a scratch buffer of exactly attn_workspace_bytes followed by a canary that must survive.

q, k and v hold no NaN and no Inf: that is out of scope, the reference is undefined there too.

The table at the bottom asserts at import, through attn_ref64.geometry (a restatement of the launch arithmetic, used for
nothing else), that every launch class and every mask pattern is reached by a case that also runs on the CPU."""
import torch

from pasco_amd.me.backend import SPLIT_ACT_EXP2, F16RangeError, StatusError, _ptr
from tests import attn_ref64 as ref

DH, C, E = 48, 64, 80
GUARD = 1 << 16
CASES = []


def case(geoms, tags=(), gpu_only=False, name=None):
    """Register a case: `geoms` = the (B, H, Q, N) shapes it runs all kernels at, `tags` = the patterns it applies."""
    def deco(f):
        f.geoms, f.tags, f.gpu_only = tuple(geoms), frozenset(tags), gpu_only
        if name is not None:
            f.__name__ = name
        CASES.append(f)
        return f
    return deco


# ---- launches with an exactly-sized scratch and a canary -----------------------------------------------------------------------
def _scratch(be, dev, N, B, H, Q, dh, short=0):
    need = int(be.fn["attn_workspace_bytes"](N, B, H, Q, dh))
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device=dev)
    ws[need:] = 0x5A
    return ws, need - short


def _canary(ws, need, what):
    if ws.is_cuda:
        torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), f"{what} wrote past its declared workspace"


def run_fwd(be, dev, q, k, v, bits=None, any_=None, short=0, out=None):
    B, H, Q, dh = q.shape
    N = k.shape[1]
    ws, need = _scratch(be, dev, N, B, H, Q, dh, short)
    out = torch.empty((B, Q, H * dh), device=dev) if out is None else out
    rc = be.fn["attn_cross_fwd"](_ptr(q), _ptr(k), _ptr(v), _ptr(bits), _ptr(any_), _ptr(out), N, B, H, Q, dh, _ptr(ws), need,
                                 be.stream(dev))
    _canary(ws, need + short, "attn_cross_fwd")
    return out, rc


def run_split(be, dev, q, ks, vs, N, bits=None, any_=None, short=0, out=None):
    B, H, Q, dh = q.shape
    ws, need = _scratch(be, dev, N, B, H, Q, dh, short)
    out = torch.empty((B, Q, H * dh), device=dev) if out is None else out
    rc = be.fn["attn_cross_split"](_ptr(q), _ptr(ks), _ptr(vs), SPLIT_ACT_EXP2, _ptr(bits), _ptr(any_), _ptr(out), N, B, H, Q,
                                   dh, _ptr(ws), need, be.status_ptr(dev), be.stream(dev))
    _canary(ws, need + short, "attn_cross_split")
    return out, rc


def run_feat(be, dev, q2, xs, aug, N, bits=None, any_=None, short=0, out=None):
    B, H, Q, d = q2.shape
    ws, need = _scratch(be, dev, N, B, H, Q, d, short)
    out = torch.empty((B, Q, H * d), device=dev) if out is None else out
    rc = be.fn["attn_cross_feat"](_ptr(q2), _ptr(xs), _ptr(aug), d - 16, SPLIT_ACT_EXP2, _ptr(bits), _ptr(any_), _ptr(out), N, B,
                                  H, Q, _ptr(ws), need, be.status_ptr(dev), be.stream(dev))
    _canary(ws, need + short, "attn_cross_feat")
    return out, rc


# ---- inputs --------------------------------------------------------------------------------------------------------------------
_EPS = {}


def angle_eps(dev):
    """The angle model of the sine table, as the transformer hands it to pos_aug."""
    from pasco_amd.graph.transformer import PositionEmbeddingSineSparse
    if dev.type not in _EPS:
        pe = PositionEmbeddingSineSparse(128, normalize=True)
        _EPS[dev.type] = (pe.angle_model(dev)[0].contiguous(), pe.TABLE_LO)
    return _EPS[dev.type]


class Problem:
    """Operands of one shape on the CPU, of unit scale (the recipe of tests/test_hip_attn.py); cases edit them before run()."""

    def __init__(self, B, H, Q, N, seed):
        g = self.g = torch.Generator().manual_seed(seed)
        self.B, self.H, self.Q, self.N = B, H, Q, N
        self.q = torch.randn(B, H, Q, DH, generator=g) * DH ** -0.5
        self.k = torch.randn(B, N, H * DH, generator=g) * 1.7
        self.v = torch.randn(B, N, H * DH, generator=g)
        self.x = torch.randn(B * N, C, generator=g) * torch.rand(B * N, 1, generator=g) * 3
        self.coords = torch.randint(-2, 260, (B * N, 4), generator=g, dtype=torch.int32)
        nz = max(1, N // 7)
        self.coords[:nz, 1:] = torch.randint(0, 3, (nz, 3), generator=g, dtype=torch.int32)
        self.q2 = torch.randn(B, H, Q, E, generator=g) * DH ** -0.5
        self.q2[..., C + 6:] = 0                                     # unused position columns
        self.q2[..., C + 3:C + 6] *= 2.0 ** -14

    def random_allow(self, share=0.3):
        """The recipe of tests/test_hip_attn.py: `share` allowed, one query allowed nowhere, one masked on half a batch."""
        allow = torch.rand(self.B, self.N, self.Q, generator=self.g) < share
        allow[:, :, 3 % self.Q] = False
        if self.N > 40:
            allow[0, : self.N // 2, self.Q - 1] = False
        return allow


def pack(be, dev, allow):
    B, N, Q = allow.shape
    return be.attn_mask_pack(allow.reshape(B * N, Q).float().contiguous().to(dev), B, N)


def clear_status(be, dev):
    try:
        be.check_status(dev)
    except StatusError:
        pass


def run(be, dev, label, p, allow=None, any_given=True, bits=None, any_=None, kernels=("fwd", "split", "feat")):
    """All kernels on problem `p` against fp64 -> {kernel: output}.  The mask is `allow` packed by the backend, or the given
    words (`allow` then states what they mean)."""
    B, H, Q, N = p.B, p.H, p.Q, p.N
    clear_status(be, dev)
    if allow is not None and bits is None:
        bits, any_ = pack(be, dev, allow)
    if not any_given:
        any_ = None
    al = None if allow is None else allow.to(dev)
    outs, ratios = {}, {}
    q = p.q.to(dev).contiguous()
    if H * DH % 32 == 0 and ("fwd" in kernels or "split" in kernels):
        ks = be.split_rows(p.k.reshape(B * N, -1).contiguous().to(dev))
        vs = be.split_rows(p.v.reshape(B * N, -1).contiguous().to(dev))
        k2, v2 = ref.unsplit(ks, H * DH).view(B, N, -1).contiguous(), ref.unsplit(vs, H * DH).view(B, N, -1).contiguous()
        exp, scale = ref.attention(q, ref.unsplit64(ks, H * DH).view(B, N, -1), ref.unsplit64(vs, H * DH).view(B, N, -1), al,
                                   any_given)
        if "split" in kernels:
            outs["split"], rc = run_split(be, dev, q, ks, vs, N, bits, any_)
            assert rc == 0, rc
            ratios["split"] = ref.ratio(outs["split"], exp, scale)
    else:
        k2, v2 = p.k.to(dev).contiguous(), p.v.to(dev).contiguous()
        exp, scale = ref.attention(q, k2, v2, al, any_given)
    if "fwd" in kernels:
        outs["fwd"], rc = run_fwd(be, dev, q, k2, v2, bits, any_)
        assert rc == 0, rc
        ratios["fwd"] = ref.ratio(outs["fwd"], exp, scale)
    if "feat" in kernels:
        eps, lo = angle_eps(dev)
        xs = be.split_rows(p.x.to(dev).contiguous())
        aug = be.pos_aug(p.coords.to(dev).contiguous(), eps, lo)
        q2 = p.q2.to(dev).contiguous()
        r = ref.feat_rows(xs, aug, B, N)
        expf, scalef = ref.attention(q2, r, r, al, any_given, per_head=False)
        outs["feat"], rc = run_feat(be, dev, q2, xs, aug, N, bits, any_)
        assert rc == 0, rc
        ratios["feat"] = ref.ratio(outs["feat"], expf, scalef)
    be.check_status(dev)                                             # no flag on finite inputs inside the f16 range
    for kname, r in ratios.items():
        print(f"ATTN_RATIO {label} B{B} H{H} Q{Q} N{N} {kname} {r:.4f}")
    bad = {kname: r for kname, r in ratios.items() if not r <= 1.0}
    assert not bad, f"{label}: max |got - exp| / bound above 1: {bad}"
    return outs


# ---- launch geometry -----------------------------------------------------------------------------------------------------------
# (B, H, Q, N): chosen with attn_ref64.geometry; the class every row is there for is asserted in _check_table()
GEOMS = [
    (8, 8, 33, 1792),      # split / feat: 7 tiles per range, 8 ranges, no idle workgroup; fwd: 4 tiles per wave
    (8, 8, 65, 1280),      # 5 tiles per range (the ring wraps, 2 tiles into the second turn); 3 live waves; fwd: 3 per wave
    (8, 8, 96, 927),       # 4 tiles per range (the ring wraps once), last range 1 tile; N % 32 = 31, N % 16 = 15
    (8, 8, 97, 705),       # 3 tiles per range, last range 2; N % 32 = 1 = N % 16; 4 live waves, the last with one query
    (8, 8, 64, 480),       # 2 tiles per range (shorter than the ring), last range 1; N % 32 = 0
    (3, 6, 17, 1759),      # H = 6 (288-column rows); 2 per range, last 1; 84 groups: 4 idle workgroups
    (2, 4, 15, 4817),      # 3 per range over 51 ranges, last 1; fwd: one tile per wave, 151 * 2 waves
    (65, 8, 5, 200),       # B * H = 520 > 512: one range of 7 tiles per head; 65 groups: 7 idle workgroups
    (257, 8, 5, 40),       # B * H = 2056 > 2048 (fwd); workspace 10272 records x 64 x 52 x 4 B = 136.7 MB (feat: 220.9 MB)
    (1, 2, 1, 1), (2, 4, 15, 2), (3, 6, 16, 15), (1, 8, 17, 16), (2, 6, 32, 17), (3, 2, 63, 31), (1, 4, 64, 32),
    (2, 8, 127, 33), (3, 4, 128, 63), (8, 2, 33, 64), (1, 6, 96, 65),
]


def _geom_case(B, H, Q, N):
    @case([(B, H, Q, N)], name=f"geom_B{B}_H{H}_Q{Q}_N{N}")
    def f(be, dev):
        p = Problem(B, H, Q, N, seed=1000 + N + Q)
        run(be, dev, "plain", p)
        run(be, dev, "random_mask", p, p.random_allow())


for _g in GEOMS:
    _geom_case(*_g)

# ---- mask patterns -------------------------------------------------------------------------------------------------------------
# split / feat: 47 tiles in 16 ranges of 3 (range r starts at key 96 r); fwd: 94 tiles in 47 ranges of 2 (range r at key 32 r)
MG = (3, 8, 70, 1501)
MG_INTERIOR = 480          # first key of range 5 (split / feat) and of range 15 (fwd)
MG_LAST = 1488             # first key of the last 16-key tile, inside the last 32-key tile (1472 ..): both partial


@case([MG], tags=["one_key"])
def one_key_per_query(be, dev):
    """Exactly one allowed key: every other range hands the merge (m = -inf, l = 0).  Key 0, key N - 1 and the first key of
    an interior range, by query."""
    B, H, Q, N = MG
    p = Problem(*MG, seed=11)
    allow = torch.zeros(B, N, Q, dtype=torch.bool)
    for qi in range(Q):
        allow[:, (0, N - 1, MG_INTERIOR)[qi % 3], qi] = True
    outs = run(be, dev, "one_key", p, allow)
    # softmax over one key: the output is that key's value row - exactly, whatever the arithmetic
    v2 = ref.unsplit(be.split_rows(p.v.reshape(B * N, -1).contiguous().to(dev)), H * DH).view(B, N, -1)
    for qi in (0, 1, 2, Q - 1):
        want = v2[:, (0, N - 1, MG_INTERIOR)[qi % 3]]
        for kname in ("fwd", "split"):
            assert torch.allclose(outs[kname][:, qi], want, rtol=1e-6, atol=0), (kname, qi)


@case([MG], tags=["first_tile"])
def first_tile_only(be, dev):
    """Allowed keys all inside the first 16: every later tile and range is trailing -inf."""
    B, H, Q, N = MG
    p = Problem(*MG, seed=12)
    allow = torch.zeros(B, N, Q, dtype=torch.bool)
    allow[:, :16] = torch.rand(B, 16, Q, generator=p.g) < 0.5
    allow[:, 5] = True
    run(be, dev, "first_tile", p, allow)


@case([MG], tags=["odd_tiles"])
def odd_tiles_only(be, dev):
    """Allowed keys only in 32-key tiles of odd index: the running maximum leaves -inf, meets an empty tile, moves again."""
    B, H, Q, N = MG
    p = Problem(*MG, seed=13)
    odd = ((torch.arange(N) // 32) % 2 == 1)
    allow = (torch.rand(B, N, Q, generator=p.g) < 0.5) & odd[None, :, None]
    run(be, dev, "odd_tiles", p, allow)


@case([MG], tags=["last_tile"])
def last_partial_tile_only(be, dev):
    B, H, Q, N = MG
    p = Problem(*MG, seed=14)
    allow = torch.zeros(B, N, Q, dtype=torch.bool)
    allow[:, MG_LAST:] = torch.rand(B, N - MG_LAST, Q, generator=p.g) < 0.6
    allow[:, N - 1] = True
    run(be, dev, "last_tile", p, allow)


@case([MG], tags=["empty_batch_any"])
def empty_batch_with_any(be, dev):
    """Batch element 1 allows nothing, its neighbours are ordinary; `any` given: element 1 attends everywhere."""
    p = Problem(*MG, seed=15)
    allow = p.random_allow()
    allow[1] = False
    run(be, dev, "empty_batch_any", p, allow)


@case([MG], tags=["empty_batch_null_any"])
def empty_batch_without_any(be, dev):
    """The same with any = NULL: a query with no allowed key gets zeros (include/pasco_hip.h), from all three kernels and
    the oracle - exactly zero, not a small number."""
    p = Problem(*MG, seed=15)
    allow = p.random_allow()
    allow[1] = False
    outs = run(be, dev, "empty_batch_null_any", p, allow, any_given=False)
    for kname, o in outs.items():
        assert not bool(o[1].any()), kname                          # the whole element
        assert not bool(o[:, 3].any()), kname                       # and the query allowed nowhere, in every element
        assert bool(o[0, 4].any()), kname


@case([MG], tags=["garbage_bits"])
def garbage_bits_beyond_q(be, dev):
    """Stray bits at positions >= Q of the 128-bit words (keys and `any`) change no output bit."""
    B, H, Q, N = MG
    p = Problem(*MG, seed=16)
    allow = p.random_allow()
    bits, any_ = pack(be, dev, allow)
    clean = run(be, dev, "garbage_bits/clean", p, allow, bits=bits, any_=any_)
    high = torch.zeros(4, dtype=torch.int64)
    for pos in range(Q, 128):
        high[pos >> 5] |= 1 << (pos & 31)
    high = high.to(torch.int32).to(dev)                                # wraps to the int32 bit pattern
    junk = torch.randint(-2 ** 31, 2 ** 31 - 1, (B, N, 4), generator=p.g, dtype=torch.int64).to(torch.int32).to(dev)
    dirty = run(be, dev, "garbage_bits/dirty", p, allow, bits=bits | (junk & high), any_=any_ | high)
    for kname in clean:
        assert torch.equal(clean[kname], dirty[kname]), kname


@case([MG], tags=["all_allowed"])
def all_allowed_equals_unmasked(be, dev):
    """Every bit set: bit-equal to the unmasked call of the same kernel."""
    B, H, Q, N = MG
    p = Problem(*MG, seed=17)
    plain = run(be, dev, "all_allowed/plain", p)
    full = run(be, dev, "all_allowed/bits", p, torch.ones(B, N, Q, dtype=torch.bool))
    for kname in plain:
        assert torch.equal(plain[kname], full[kname]), kname


# ---- number patterns -----------------------------------------------------------------------------------------------------------
NG = (3, 8, 40, 1501)      # the ranges of MG


def _both(be, dev, label, p):
    run(be, dev, label, p)
    run(be, dev, label + "/masked", p, p.random_allow())


@case([NG], tags=["uniform"])
def uniform_softmax(be, dev):
    """K = 0 (feat: Q2 = 0): every score is 0, the output is the mean of V over the allowed keys."""
    p = Problem(*NG, seed=21)
    p.k.zero_()
    p.q2.zero_()
    _both(be, dev, "uniform", p)


def _peaked(order):
    """Scores 60 c a[n] (+ noise of ~0.3), c in [0.7, 1] by query: a = a ramp over the keys with the row maximum at the last
    key, at the first key, or -1 everywhere but at the two keys on either side of range boundaries."""
    B, H, Q, N = NG
    p = Problem(*NG, seed=22)
    g = p.g
    if order == "last":
        a = torch.linspace(-1, 1, N)
    elif order == "first":
        a = torch.linspace(1, -1, N)
    else:
        a = torch.full((N,), -1.0)
        for r in (1, 5, 10, 15):
            a[96 * r - 1] = a[96 * r] = 1.0                            # last key of a split / feat range, first of the next
        a[32 * 7 - 1] = a[32 * 7] = 1.0                                # and of a fwd range
    c = 0.7 + 0.3 * torch.rand(B, H, Q, 1, generator=g)
    u = torch.nn.functional.normalize(torch.randn(H, DH, generator=g), dim=-1)
    p.q = 30.0 * c * u[None, :, None, :]
    p.k = (2.0 * a[None, :, None, None] * u[None, None] + 0.01 * torch.randn(B, N, H, DH, generator=g)).reshape(B, N, H * DH)
    w = torch.nn.functional.normalize(torch.randn(C, generator=g), dim=-1)
    p.x = (2.0 * a[None, :, None] * w + 0.01 * torch.randn(B, N, C, generator=g)).reshape(B * N, C)
    p.q2[..., :C] = 30.0 * c * w
    return p


@case([NG], tags=["peaked_last"])
def peaked_maximum_last(be, dev):
    """|s| up to 60, the largest key last: the running maximum rises at every tile and every range."""
    _both(be, dev, "peaked_last", _peaked("last"))


@case([NG], tags=["peaked_first"])
def peaked_maximum_first(be, dev):
    """|s| up to 60, the largest key first: the maximum is reached at once, everything later is far below it."""
    _both(be, dev, "peaked_first", _peaked("first"))


@case([NG], tags=["peaked_boundary"])
def peaked_maxima_at_range_boundaries(be, dev):
    _both(be, dev, "peaked_boundary", _peaked("boundary"))


@case([NG], tags=["mixed_magnitude"])
def mixed_magnitude_columns(be, dev):
    """V columns of 1e3 and of 1e-3 in the same row, entries of full fp32 precision (more than the 11 significant bits of
    one f16 plane: the lo plane matters; at 1e-3 it is a denormal f16).  The feature kernel's rows are K and V at once:
    its Q2 columns shrink by what the key columns grow."""
    B, H, Q, N = NG
    p = Problem(*NG, seed=23)
    p.v = torch.rand(B, N, H * DH, generator=p.g) * 2 - 1               # |v| <= 1: 1e3 * 2^5 stays inside the f16 range
    p.v[..., 0::4] *= 1e3
    p.v[..., 1::4] *= 1e-3
    xs = torch.rand(B * N, C, generator=p.g) * 2 - 1
    xs[:, :8] *= 1e3
    xs[:, 8:16] *= 1e-3
    p.x = xs
    p.q2[..., :8] *= 1e-3
    _both(be, dev, "mixed_magnitude", p)


FG = (2, 4, 33, 300)


@case([FG], tags=["f16_range"])
def split_query_f16_range_flag(be, dev):
    """One query value with |q * 2^8| > 65504: the split kernel raises status bit 0 and check_status raises F16RangeError
    (the C oracle forms no f16 query and documents that it never raises).  The same input at 65504 / 2^8 raises nothing
    and matches fp64."""
    B, H, Q, N = FG
    p = Problem(*FG, seed=24)
    p.k[..., 1 * DH + 7] *= 2.0 ** -8                                   # the key column that meets the large query value
    p.q[0, 1, 5, 7] = 65504.0 / 256.0                                   # 255.875: the largest value inside
    run(be, dev, "f16_range/under", p)
    p.q[0, 1, 5, 7] = 256.0
    q = p.q.to(dev).contiguous()
    ks = be.split_rows(p.k.reshape(B * N, -1).contiguous().to(dev))
    vs = be.split_rows(p.v.reshape(B * N, -1).contiguous().to(dev))
    clear_status(be, dev)
    _, rc = run_split(be, dev, q, ks, vs, N)
    assert rc == 0
    if be.device_type == "cpu":
        be.check_status(dev)
        return
    try:
        be.check_status(dev)
    except F16RangeError as e:
        assert e.bits == 1
    else:
        raise AssertionError("no F16RangeError for |q * 2^8| > 65504")


# ---- helpers -------------------------------------------------------------------------------------------------------------------
SPECIALS = (0.0, -0.0, 1e-45, -1e-45, float("inf"), float("-inf"), float("nan"))


@case([], tags=["mask_pack"])
def mask_pack_bit_for_bit(be, dev):
    """attn_mask_pack and bits_or_reduce against integer arithmetic: both rules, zeros of both signs, denormals, infinities
    and NaN (non-zero; not positive), bits >= Q clear, a batch element of all-zero rows next to one that is not."""
    g = torch.Generator().manual_seed(31)
    for B in (1, 3):
        for N in (1, 2, 63, 64, 65, 777):
            for Q in (1, 31, 32, 33, 64, 65, 100, 127, 128):
                for positive_only in (False, True):
                    vals = torch.randn(B * N, Q, generator=g)
                    vals[torch.rand(B * N, Q, generator=g) < 0.5] = 0.0
                    sp = torch.tensor(SPECIALS)[torch.randint(0, len(SPECIALS), (B * N, Q), generator=g)]
                    pick = torch.rand(B * N, Q, generator=g) < 0.3
                    vals[pick] = sp[pick]
                    vals[0, : min(Q, len(SPECIALS))] = torch.tensor(SPECIALS)[:Q]
                    if B == 3:
                        vals[N:2 * N] = torch.tensor([0.0, -0.0])[torch.randint(0, 2, (N, Q), generator=g)]
                    bits_e, any_e = ref.mask_pack(vals, B, N, positive_only)
                    bits, any_ = be.attn_mask_pack(vals.to(dev), B, N, positive_only=positive_only)
                    what = (B, N, Q, positive_only)
                    assert torch.equal(bits.cpu().reshape(B * N, 4), bits_e), what
                    assert torch.equal(any_.cpu(), any_e), what
                    assert torch.equal(be.bits_or_reduce(bits).cpu(), any_e), what
                    for pos in range(Q, 128):
                        assert not bool(((bits_e[:, pos >> 5] >> (pos & 31)) & 1).any()), what
                    if B == 3:
                        assert not bool(any_.cpu()[1].any()), what
                    nobits, noany = be.attn_mask_pack(vals.to(dev), B, N, positive_only=positive_only, want_any=False)
                    assert noany is None and torch.equal(nobits.cpu(), bits.cpu()), what


@case([], tags=["pos_aug"])
def pos_aug_bit_for_bit(be, dev):
    """pos_aug against the formula above ph_pos_aug: the table's two ends, one outside on each side (clamped to the nearer
    end, status bit 2 raised - for those rows only), the value 0 and its neighbours."""
    g = torch.Generator().manual_seed(32)
    tab_lo, tab_n = -5, 37
    eps = (torch.randn(tab_n, generator=g) * 1e-3).contiguous()
    eps[0 - tab_lo] = 0.0
    hi = tab_lo + tab_n - 1
    inside = torch.tensor([tab_lo, hi, -1, 0, 1, 2, 17], dtype=torch.int32)
    idx = torch.randint(0, len(inside), (500, 4), generator=g)
    coords = inside[idx].contiguous()
    coords[:7, 1] = inside
    coords[:7, 2] = inside.flip(0)
    for exp2 in (SPLIT_ACT_EXP2, 0, -3):
        clear_status(be, dev)
        aug = be.pos_aug(coords.to(dev), eps.to(dev), tab_lo, exp2=exp2)
        aug_e, outside = ref.pos_aug(coords, eps, tab_lo, exp2)
        assert not bool(outside.any())
        assert torch.equal(aug.cpu().view(torch.int16), aug_e.view(torch.int16)), exp2
        be.check_status(dev)                                            # nothing outside: no flag
    for bad_value in (tab_lo - 1, hi + 1, -100000, 100000):
        for axis in (1, 2, 3):
            bad = coords.clone()
            bad[123, axis] = bad_value
            clear_status(be, dev)
            aug = be.pos_aug(bad.to(dev), eps.to(dev), tab_lo)
            aug_e, outside = ref.pos_aug(bad, eps, tab_lo)
            assert outside.nonzero().flatten().tolist() == [123]
            assert torch.equal(aug.cpu().view(torch.int16), aug_e.view(torch.int16)), (bad_value, axis)
            try:
                be.check_status(dev)
            except StatusError as e:
                assert e.bits == 4, e.bits
            else:
                raise AssertionError(f"no status bit 2 for coordinate {bad_value} on axis {axis}")


@case([], tags=["ws_short"])
def workspace_one_byte_short_is_refused(be, dev):
    """A scratch buffer one byte short of attn_workspace_bytes: a non-zero return and nothing launched (the output keeps
    what it held).  A host-side check."""
    B, H, Q, N = 2, 4, 20, 100
    p = Problem(B, H, Q, N, seed=33)
    q, k, v = p.q.to(dev), p.k.to(dev), p.v.to(dev)
    ks, vs = be.split_rows(k.reshape(B * N, -1).contiguous()), be.split_rows(v.reshape(B * N, -1).contiguous())
    eps, lo = angle_eps(dev)
    xs, aug = be.split_rows(p.x.to(dev)), be.pos_aug(p.coords.to(dev), eps, lo)
    q2 = p.q2.to(dev)
    for name, call, width in (("fwd", lambda o: run_fwd(be, dev, q, k, v, short=1, out=o), H * DH),
                              ("split", lambda o: run_split(be, dev, q, ks, vs, N, short=1, out=o), H * DH),
                              ("feat", lambda o: run_feat(be, dev, q2, xs, aug, N, short=1, out=o), H * E)):
        out = torch.full((B, Q, width), 7.0, device=dev)
        _, rc = call(out)
        assert rc != 0, name
        assert bool((out == 7.0).all()), name


# ---- the table reaches every class ---------------------------------------------------------------------------------------------
MASK_TAGS = ("one_key", "first_tile", "odd_tiles", "last_tile", "empty_batch_any", "empty_batch_null_any", "garbage_bits",
             "all_allowed")
NUMBER_TAGS = ("uniform", "peaked_last", "peaked_first", "peaked_boundary", "mixed_magnitude", "f16_range")
HELPER_TAGS = ("mask_pack", "pos_aug", "ws_short")


def classes_of(B, H, Q, N):
    """The launch classes shape (B, H, Q, N) belongs to."""
    out = {f"H={H}", f"B={B}"}
    for tile in (16, 32):
        out.add(f"N%{tile}={N % tile}")
        if N < tile:
            out.add(f"N<{tile}")
    out.add(f"N={N}")
    for kind in ("split", "feat"):
        if kind == "split" and H * DH % 32 != 0:
            continue
        ge = ref.geometry(kind, B, H, Q, N)
        tpw, last = ge["tpw"], ge["last_range_tiles"]
        out.add(f"{kind}:tpw={tpw}" if tpw < 7 else f"{kind}:tpw>=7")
        if last < tpw:
            out.add(f"{kind}:tpw={tpw},last_short")
        if tpw >= 3 and last < 3:
            out.add(f"{kind}:last_range_shorter_than_ring_only")
        out.add(f"{kind}:live_waves={ge['live_waves']}")
        out.add(f"{kind}:Q={Q}")
        out.add(f"{kind}:idle_groups" + ("=0" if ge["idle_groups"] == 0 else ">0"))
        if B * H > 512:
            assert ge["splits"] == 1
            out.add(f"{kind}:one_range,BH>512")
    ge = ref.geometry("fwd", B, H, Q, N)
    out.add(f"fwd:tpw={ge['tpw']}" if ge["tpw"] < 3 else "fwd:tpw>=3")
    out.add(f"fwd:Q={Q}")
    out.add(f"fwd:qp={ge['qp']}")
    if ge["idle_groups"]:
        out.add("fwd:waves%4!=0")
    if Q % 16:
        out.add("fwd:partial_query_tile")
    if B * H > 2048:
        out.add("fwd:BH>2048")
    return out


REQUIRED = (
    [f"{k}:tpw={t}" for k in ("split", "feat") for t in (1, 2, 3, 4, 5)] + [f"{k}:tpw>=7" for k in ("split", "feat")]
    + [f"{k}:tpw={t},last_short" for k in ("split", "feat") for t in (2, 3, 4)]
    + [f"{k}:last_range_shorter_than_ring_only" for k in ("split", "feat")]
    + [f"{k}:live_waves={w}" for k in ("split", "feat") for w in (1, 2, 3, 4)]
    + [f"{k}:Q={q}" for k in ("split", "feat") for q in (1, 32, 33, 64, 65, 96, 97, 127, 128)]
    + [f"{k}:idle_groups{s}" for k in ("split", "feat") for s in ("=0", ">0")]
    + [f"{k}:one_range,BH>512" for k in ("split", "feat")]
    + ["fwd:tpw=1", "fwd:tpw=2", "fwd:tpw>=3", "fwd:waves%4!=0", "fwd:BH>2048", "fwd:qp=64", "fwd:qp=128",
       "fwd:partial_query_tile"]
    + [f"fwd:Q={q}" for q in (1, 15, 16, 17, 63, 64, 65, 128)]
    + [f"H={h}" for h in (2, 4, 6, 8)] + [f"B={b}" for b in (1, 2, 3, 8)]
    + [f"N%{t}={r}" for t in (16, 32) for r in (0, 1, t - 1)] + ["N<16", "N<32", "N=1", "N=2"]
)


def _check_table(cases):
    on_cpu = [c for c in cases if not c.gpu_only]
    assert 5 * (len(cases) - len(on_cpu)) <= len(cases), "more than one case in five is gpu_only"
    reached, tags = set(), set()
    for c in on_cpu:
        tags |= c.tags
        for shape in c.geoms:
            reached |= classes_of(*shape)
    missing = [r for r in REQUIRED if r not in reached]
    assert not missing, f"launch classes no CPU-run case reaches: {missing}"
    missing = [t for t in MASK_TAGS + NUMBER_TAGS + HELPER_TAGS if t not in tags]
    assert not missing, f"patterns no CPU-run case applies: {missing}"
    for c in cases:                                # a mask pattern counts at >= 4 ranges of >= 2 tiles, for every kernel
        if c.tags & set(MASK_TAGS):
            for shape in c.geoms:
                for kind in ("fwd", "split", "feat"):
                    ge = ref.geometry(kind, *shape)
                    assert ge["splits"] >= 4 and ge["tpw"] >= 2, (c.__name__, kind, ge)
    # what the mask cases assume about MG
    sp, fw = ref.geometry("split", *MG), ref.geometry("fwd", *MG)
    assert MG_INTERIOR % (sp["tpw"] * 32) == 0 and 0 < MG_INTERIOR // (sp["tpw"] * 32) < sp["splits"] - 1
    assert MG_INTERIOR % (fw["tpw"] * 16) == 0 and 0 < MG_INTERIOR // (fw["tpw"] * 16) < fw["splits"] - 1
    assert MG_LAST == (fw["ntile"] - 1) * 16 >= (sp["ntile"] - 1) * 32 and MG[3] % 32 and MG[3] % 16
    assert ref.geometry("split", *NG)["tpw"] == 3 and fw["tpw"] == 2                 # the boundary keys of _peaked


_check_table(CASES)
