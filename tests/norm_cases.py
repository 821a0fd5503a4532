"""Test helper: the case table and the shared checks of batch normalisation over rows (tests/test_norm_cpu.py on the host
restatement, tests/test_hip_norm.py on the pn_* kernels).  Every check takes the device; the references are tests/norm_ref64.py.

Inputs are randn * s + mu with non-dyadic s and mu (no channel is constant, so no denominator of the bound is zero); one case
has mu = 1000, s = 1, where a variance formed as sum x^2 - n * mean^2 in fp32 loses every digit."""
import functools

import pytest
import torch

from pasco_amd.grad import host
from pasco_amd.grad.norm import batch_norm_rows
from tests.norm_ref64 import NORM_M, norm_twin, ratios

T = host.NORM_TILE_ROWS
ROWS = (2, 63, 65, T - 1, T, T + 1, 3 * T + 5)
CHANNELS = (1, 3, 20, 32, 65, 283)          # 283: the point MLP's width; 65: one lane past a wave; c % 4 != 0: the scalar path
ACT_NAMES = ("none", "relu", "leaky")
# every (n, c), the activation cycling so that each n and each c meets all three
CASES = [(n, c, ACT_NAMES[(i + j) % 3]) for i, n in enumerate(ROWS) for j, c in enumerate(CHANNELS)]
SLOPE, EPS, MOMENTUM = 0.07, 1e-5, 0.1
MU, S = 0.37, 1.3

# ---- past the first trip of the loops ----------------------------------------------------------------------------------------
# The tables above stop at 4 tiles and two multiples of 4 among the channel counts.  These reach what a scene runs: records
# beyond one wave and beyond one pass of the merge kernels, and the vector geometry at the net's widths.
LONG_ROWS = (9 * T + 1, 32 * T, 32 * T + 1, 65 * T + 3)
VECTOR_C = (4, 8, 16, 64, 128, 256, 260)     # c % 4 == 0: L = 1, 2, 4, 16, 32, 64 and, at 260, a second block of channel units
SCALAR_C = (2, 6, 10, 18)                    # c % 4 != 0: L = 2, 8, 16, 32
# c > 64 is left out at the longest n: the classes it would reach are reached at 32 T + 1 already
LONG_CASES = [(n, c, ACT_NAMES[(i + j) % 3]) for i, n in enumerate(LONG_ROWS) for j, c in enumerate(VECTOR_C + SCALAR_C)
              if not (n == LONG_ROWS[-1] and c > 64)]
MERGE_R = (8, 9, 31, 32, 33, 64, 65, 97)     # records handed to the merge kernels
MERGE_C = (3, 20)                            # one partial block of MERGE_CH channels; a full one and a partial one
CHUNK_CYCLE = (0, 1, 3, T, T + 2)            # the rows of record i are CHUNK_CYCLE[i % 5]: unequal counts, empty records
MISALIGNED_C = (32, 256)
VIRTUAL_RANKS_C = (65, 128)

BLOCK, MERGE_CH, MERGE_K, WAVE_RECORDS = 256, 8, 32, 8      # csrc/norm.hip: threads, channels and records per pass / per wave


# !! `row_geometry` and `merge_geometry` restate the launch arithmetic of pasco_amd/csrc/norm.hip.  They are used to CHOOSE shapes
# !! and to assert, at import, that the tables above reach every launch class - never to form an expected value: those come
# !! from tests/norm_ref64.py and from the host restatement alone.
def row_geometry(n, c, aligned=True):
    V = 4 if (c % 4 == 0 and aligned) else 1
    cu, L = c // V, 1
    while L < cu and L < 64:
        L *= 2
    tiles = -(-n // T)
    return dict(V=V, L=L, R=BLOCK // L, grid_y=-(-cu // L), tiles=tiles, passes=-(-tiles // MERGE_K))


def merge_geometry(counts, c):
    """counts: the rows of every record in order -> which waves and passes hold a non-empty / an empty record."""
    slots = [(i // MERGE_K, (i % MERGE_K) // WAVE_RECORDS, n > 0) for i, n in enumerate(counts)]
    return dict(passes=-(-len(counts) // MERGE_K), full_last_pass=len(counts) % MERGE_K == 0,
                rows_in_upper_waves=any(w > 0 and has for _, w, has in slots),
                empty_in_upper_waves=any(w > 0 and not has for _, w, has in slots),
                rows_in_later_pass=any(p > 0 and has for p, _, has in slots),
                empty_in_later_pass=any(p > 0 and not has for p, _, has in slots),
                rows_in_upper_waves_of_later_pass=any(p > 0 and w > 0 and has for p, w, has in slots),
                channel_blocks=-(-c // MERGE_CH), partial_block=c % MERGE_CH != 0)


def merge_counts(r):
    return [CHUNK_CYCLE[i % len(CHUNK_CYCLE)] for i in range(r)]


def _check_norm_tables():
    assert (BLOCK, MERGE_K) == (256, BLOCK // MERGE_CH) and WAVE_RECORDS == 64 // MERGE_CH
    old = [row_geometry(n, c) for n, c, _ in CASES]
    assert max(g["tiles"] for g in old) <= WAVE_RECORDS, "the short table stays inside the first wave's records"
    new = [row_geometry(n, c) for n, c, _ in LONG_CASES]
    for L in (1, 2, 4, 16, 32, 64):
        assert any(g["V"] == 4 and g["L"] == L for g in new), f"the vector path at L = {L}"
    assert any(g["V"] == 4 and g["L"] == 8 for g in old), "the vector path at L = 8 (the short table)"
    assert any(g["V"] == 4 and g["grid_y"] == 2 for g in new), "the vector path with a second block of channel units"
    for L in (2, 8, 16, 32):
        assert any(g["V"] == 1 and g["L"] == L for g in new), f"the scalar path at L = {L}"
    for c in VECTOR_C + SCALAR_C:
        mine = [row_geometry(n, k) for n, k, _ in LONG_CASES if k == c]
        assert any(WAVE_RECORDS < g["tiles"] < MERGE_K for g in mine), f"c = {c}: tile records in waves 1 - 3, one pass"
        assert any(g["tiles"] == MERGE_K for g in mine), f"c = {c}: exactly one full pass"
        assert any(g["tiles"] == MERGE_K + 1 for g in mine), f"c = {c}: one record in the second pass"
        if c <= 64:
            assert any(g["passes"] == 3 for g in mine), f"c = {c}: three passes"
    for n in LONG_ROWS:
        assert sorted({a for k, _, a in LONG_CASES if k == n}) == sorted(ACT_NAMES), f"n = {n} meets every activation"
    g = row_geometry(T + 1, 256, aligned=False)
    assert 256 in MISALIGNED_C and (g["V"], g["L"], g["grid_y"]) == (1, 64, 4), "misaligned rows at c = 256: scalar, four blocks"
    assert row_geometry(3 * T + 5, 128)["L"] == 32 and 128 in VIRTUAL_RANKS_C, "the virtual ranks at L = 32 on the vector path"
    ms = {(r, c): merge_geometry(merge_counts(r), c) for r in MERGE_R for c in MERGE_C}
    v = list(ms.values())
    assert any(m["passes"] == 1 and m["rows_in_upper_waves"] and not m["full_last_pass"] for m in v), "one pass, records in wave 1"
    assert any(m["passes"] == 1 and m["full_last_pass"] for m in v), "exactly one full pass"
    assert any(m["passes"] == 1 and m["empty_in_upper_waves"] for m in v), "an empty record inside waves 1 - 3"
    assert any(m["passes"] == 2 and m["rows_in_later_pass"] and not m["rows_in_upper_waves_of_later_pass"] for m in v), \
        "a second pass of one wave"
    assert any(m["passes"] == 2 and m["full_last_pass"] for m in v), "two full passes"
    assert any(m["passes"] == 2 and m["empty_in_later_pass"] for m in v), "an empty record inside the second pass"
    assert any(m["passes"] >= 3 and m["rows_in_upper_waves_of_later_pass"] for m in v), "three passes and more"
    assert ms[(8, 3)]["passes"] == 1 and not ms[(8, 3)]["rows_in_upper_waves"] and ms[(9, 3)]["rows_in_upper_waves"], \
        "r = 8 ends with wave 0, r = 9 is the first with a record in wave 1"
    assert any(m["channel_blocks"] == 1 and m["partial_block"] for m in v), "one partial block of MERGE_CH channels"
    assert any(m["channel_blocks"] == 3 and m["partial_block"] for m in v), "full blocks of MERGE_CH channels and a partial one"


_check_norm_tables()

_LONG_WORST = {}


def note_long(device, worst: float):
    """The running worst ratio over the cases of this section, per device, printed with every one of them."""
    kind = torch.device(device).type
    _LONG_WORST[kind] = max(_LONG_WORST.get(kind, 0.0), worst)
    print(f"[norm] long cases on {kind} so far: worst {_LONG_WORST[kind]:.3f}")


def ops_of(device):
    """The entry points under test: the binding on a GPU, the restatement on the CPU."""
    from pasco_amd.grad.norm import _ops
    return _ops(torch.empty(0, device=device))


def tile_rows_of(device) -> int:
    if torch.device(device).type == "cuda":
        from pasco_amd.grad.normlib import PN_TILE_ROWS
        return PN_TILE_ROWS
    return host.NORM_TILE_ROWS


@functools.lru_cache(maxsize=None)
def _inputs_cpu(n, c, mu, s):
    g = torch.Generator().manual_seed(1000 * n + c)
    x = torch.randn(n, c, generator=g) * s + mu
    dy = torch.randn(n, c, generator=g) * 0.71 + 0.05
    w = torch.randn(c, generator=g) * 0.37 + 1.13
    b = torch.randn(c, generator=g) * 0.29 + 0.11
    rm = torch.randn(c, generator=g) * 0.3
    rv = torch.rand(c, generator=g) + 0.5
    return x, dy, w, b, rm, rv


def inputs(n, c, device, mu=MU, s=S):
    """-> x, dy [n, c], weight, bias, running_mean, running_var [c]: fresh copies on `device` (the cached originals stay as
    they are)."""
    return tuple(t.clone().to(device) for t in _inputs_cpu(n, c, mu, s))


def run_op(chunks_x, chunks_dy, w, b, rm, rv, act, momentum=MOMENTUM, nbt=None, gathers=None):
    """`batch_norm_rows` forward and backward per chunk (one chunk without `gathers`: the local operator) -> (the quantities of
    tests/norm_ref64.py with y / dx concatenated and dw / db ADDED over the chunks, the per-chunk running statistics)."""
    ys, dxs, dws, dbs, stats = [], [], [], [], []
    for i, (x, dy) in enumerate(zip(chunks_x, chunks_dy)):
        xi = x.detach().requires_grad_(True)                 # not a copy: a test may hand in rows at a chosen address
        wi = w.clone().requires_grad_(True) if w is not None else None
        bi = b.clone().requires_grad_(True) if b is not None else None
        rmi, rvi = (rm.clone() if rm is not None else None), (rv.clone() if rv is not None else None)
        gather = None if gathers is None else gathers[i]
        y = batch_norm_rows(xi, wi, bi, rmi, rvi, nbt, momentum, EPS, act=act, slope=SLOPE, gather=gather)
        y.backward(dy)
        ys.append(y.detach()), dxs.append(xi.grad), stats.append((rmi, rvi))
        dws.append(wi.grad if wi is not None else None), dbs.append(bi.grad if bi is not None else None)
    add = lambda ts: None if ts[0] is None else torch.stack([t.double() for t in ts]).sum(0)
    got = {"y": torch.cat(ys), "dx": torch.cat(dxs), "dw": add(dws), "db": add(dbs), "running_mean": stats[0][0],
           "running_var": stats[0][1]}
    return got, stats


def twins(chunks_x, chunks_dy, w, b, rm, rv, act, factor=MOMENTUM):
    v32 = norm_twin(chunks_x, chunks_dy, w, b, rm, rv, factor, EPS, act, SLOPE, torch.float32)
    v64 = norm_twin(chunks_x, chunks_dy, w, b, rm, rv, factor, EPS, act, SLOPE, torch.float64)
    return v32, v64


def assert_bound(r: dict, what: str):
    print(f"[norm] {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"  (worst {max(r.values()):.3f})")
    bad = {k: v for k, v in r.items() if not v <= NORM_M}
    assert not bad, f"{what}: ratio over NORM_M = {NORM_M}: {bad}"


# ---- accuracy ----------------------------------------------------------------------------------------------------------------
def check_case(device, n, c, act, mu=MU, s=S):
    x, dy, w, b, rm, rv = inputs(n, c, device, mu, s)
    got, _ = run_op([x], [dy], w, b, rm, rv, act)
    r = ratios(got, *twins([x], [dy], w, b, rm, rv, act))
    assert_bound(r, f"n = {n}, c = {c}, {act}, mu = {mu}")
    return r


def check_large_mean(device):
    """mu = 1000, s = 1: sum x^2 - n * mean^2 in fp32 has an error of the size of the variance itself (1e6 * 2^-24 * n terms);
    M2 about the tile mean has none of it."""
    return check_case(device, 3 * T + 5, 20, "relu", mu=1000.0, s=1.0)


# ---- exact properties --------------------------------------------------------------------------------------------------------
def check_repeat_bits(device):
    for n, c, act in ((3 * T + 5, 283, "leaky"), (T + 1, 32, "relu")):
        x, dy, w, b, rm, rv = inputs(n, c, device)
        a, _ = run_op([x], [dy], w, b, rm, rv, act)
        z, _ = run_op([x], [dy], w, b, rm, rv, act)
        for k in a:
            assert torch.equal(a[k], z[k]), f"{k} differs between two runs (n = {n}, c = {c})"


def _moment_ratio(rec, x):
    """The mean and the biased variance of a record against fp64, relative to torch's fp32 error on the same rows."""
    m64, v64 = x.double().mean(0), x.double().var(0, unbiased=False)
    out = {}
    for name, v, ref, v32 in (("mean", rec[1], m64, x.mean(0)), ("var", rec[2] / rec[0], v64, x.var(0, unbiased=False))):
        out[name] = float((v - ref).abs().max()) / float((v32.double() - ref).abs().max())
    return out


def check_split_merge(device):
    """The partials of pn_moments ARE moments records of its tiles and its combine IS pn_moments_merge (one left fold in ascending
    order): the merge of the per-tile records equals the record of the whole bit for bit.  Chunks of several tiles, or a permuted
    order, change the association of the fold - floating-point addition is not associative - so those are held to the accuracy
    bound instead."""
    ops, tile = ops_of(device), tile_rows_of(device)
    for c in (20, 283):
        n = 3 * tile + 5
        x = inputs(n, c, device)[0]
        whole = ops.moments(x)
        assert float(whole[0].min()) == float(whole[0].max()) == n
        recs = [ops.moments(x[r0:r0 + tile].contiguous()) for r0 in range(0, n, tile)]
        assert torch.equal(ops.moments_merge(torch.stack(recs)), whole), f"c = {c}: per-tile records"
        # with empty records in between: skipped
        empty = ops.moments(x[:0].contiguous())
        assert torch.equal(ops.moments_merge(torch.stack([empty, recs[0], empty, *recs[1:], empty])), whole)
        # chunks of several tiles at tile boundaries, and the per-tile records in another order
        two = torch.stack([ops.moments(x[:2 * tile].contiguous()), ops.moments(x[2 * tile:].contiguous())])
        assert_bound(_moment_ratio(ops.moments_merge(two), x), f"c = {c}: two chunks at a tile boundary")
        perm = torch.stack([recs[i] for i in (2, 0, 3, 1)])
        assert_bound(_moment_ratio(ops.moments_merge(perm), x), f"c = {c}: permuted per-tile records")
        assert_bound(_moment_ratio(whole, x), f"c = {c}: the whole")


def check_split_merge_long(device, n):
    """The same identity where the fold leaves the first wave's records and the first pass: whole == merge of the per-tile
    records, bit for bit, with and without empty records in between."""
    ops, tile = ops_of(device), tile_rows_of(device)
    for c in (20, 283):
        x = inputs(n, c, device)[0]
        whole = ops.moments(x)
        assert float(whole[0].min()) == float(whole[0].max()) == n
        recs = [ops.moments(x[r0:r0 + tile].contiguous()) for r0 in range(0, n, tile)]
        assert len(recs) == row_geometry(n, c)["tiles"] > WAVE_RECORDS
        assert torch.equal(ops.moments_merge(torch.stack(recs)), whole), f"n = {n}, c = {c}: per-tile records"
        empty = ops.moments(x[:0].contiguous())
        spread = [t for i, rec in enumerate(recs) for t in ((empty, rec) if i % 7 == 3 else (rec,))]
        assert len(spread) > len(recs)
        assert torch.equal(ops.moments_merge(torch.stack(spread)), whole), f"n = {n}, c = {c}: with empty records in between"
        r = _moment_ratio(whole, x)
        assert_bound(r, f"n = {n}, c = {c}: the whole")
        note_long(device, max(r.values()))


def check_merge_records(device, r, c):
    """`r` records of unequal and empty row chunks (CHUNK_CYCLE) of one x through the two merge entry points.  Both sides of the
    family evaluate w = n_b / (n + n_b), mean + d * w and (m2 + q) + (d * d) * (n * w) in fp64 in ascending order with
    contraction off, so the result equals the host restatement's bit for bit; the merged moments are also held to the accuracy
    bound against fp64 over the concatenated rows."""
    ops = ops_of(device)
    counts = merge_counts(r)
    n = sum(counts)
    x, dy, w, b, _, _ = inputs(n, c, device)
    cuts = [sum(counts[:i]) for i in range(r + 1)]
    xs = [x[a:z].contiguous() for a, z in zip(cuts[:-1], cuts[1:])]
    dys = [dy[a:z].contiguous() for a, z in zip(cuts[:-1], cuts[1:])]
    recs = torch.stack([ops.moments(t) for t in xs])
    assert recs[:, 0, 0].tolist() == [float(k) for k in counts]
    got = ops.moments_merge(recs)
    want = host.norm_moments_merge(recs.cpu())
    assert torch.equal(got.cpu().view(torch.int64), want.view(torch.int64)), \
        f"r = {r}, c = {c}: moments_merge differs from the restatement in {int((got.cpu() != want).sum())} of {want.numel()} values"
    ratio = _moment_ratio(got, x)
    assert_bound(ratio, f"r = {r}, c = {c}: merged records of unequal chunks")
    note_long(device, max(ratio.values()))
    mean_rstd = ops.finish(got, EPS, 0.0, None, None)
    sums = torch.stack([ops.bwd_sums(d, t, mean_rstd, w, b, host.ACT_LEAKY, SLOPE) for t, d in zip(xs, dys)])
    got = ops.sums_merge(sums)
    want = host.norm_sums_merge(sums.cpu())
    assert torch.equal(got.cpu().view(torch.int64), want.view(torch.int64)), \
        f"r = {r}, c = {c}: sums_merge differs from the restatement in {int((got.cpu() != want).sum())} of {want.numel()} values"


# ---- edges -------------------------------------------------------------------------------------------------------------------
def check_empty(device):
    ops = ops_of(device)
    c = 20
    x, dy, w, b, rm, rv = inputs(0, c, device)
    rec = ops.moments(x)
    assert tuple(rec.shape) == (3, c) and rec.dtype == torch.float64 and not bool(rec.any())
    rm0, rv0 = rm.clone(), rv.clone()
    mr = ops.finish(rec, EPS, MOMENTUM, rm, rv)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0), "count 0 leaves the running statistics untouched"
    sums = ops.bwd_sums(dy, x, mr, w, b, host.ACT_RELU, SLOPE)
    assert tuple(sums.shape) == (2, c) and not bool(sums.any())
    assert not bool(ops.moments_merge(torch.zeros((0, 3, c), dtype=torch.float64, device=device)).any())
    assert not bool(ops.sums_merge(torch.zeros((0, 2, c), dtype=torch.float64, device=device)).any())


def check_count_one(device):
    """A total count of 1 (only reachable with a gather): the unbiased variance divides by 1."""
    ops = ops_of(device)
    x, _, _, _, rm, rv = inputs(1, 3, device)
    rm0, rv0 = rm.clone(), rv.clone()
    rec = ops.moments(x)
    assert torch.equal(rec, torch.stack([torch.ones(3, device=device), x[0], torch.zeros(3, device=device)]).double())
    ops.finish(rec, EPS, MOMENTUM, rm, rv)
    assert torch.equal(rv, ((1.0 - MOMENTUM) * rv0.double()).float()), "M2 / max(count - 1, 1) = 0 / 1"
    assert torch.equal(rm, ((1.0 - MOMENTUM) * rm0.double() + MOMENTUM * x[0].double()).float())


def check_relu_zero_gets_no_gradient(device):
    n, c = T + 1, 20
    x, dy, _, _, rm, rv = inputs(n, c, device)
    w, b = torch.zeros(c, device=device), torch.zeros(c, device=device)
    got, _ = run_op([x], [dy], w, b, rm, rv, "relu")
    assert not bool(got["y"].any()) and not bool(got["dx"].any()) and not bool(got["dw"].any()) and not bool(got["db"].any())
    # leaky: the slope where z <= 0, so with z == 0 everywhere g = slope * dy
    got, _ = run_op([x], [dy], w, b, rm, rv, "leaky")
    want = (dy * SLOPE).double().sum(0)
    assert torch.allclose(got["db"], want, rtol=1e-6, atol=0) and not bool(got["dx"].any())      # dx: weight == 0


def check_leaky_slope(device):
    """weight = 1, bias = -10 (z < 0 everywhere): the gradient is the slope's, exactly as the twin's."""
    n, c = 65, 3
    x, dy, _, _, rm, rv = inputs(n, c, device)
    w, b = torch.ones(c, device=device), torch.full((c,), -10.0, device=device)
    got, _ = run_op([x], [dy], w, b, rm, rv, "leaky")
    v32, v64 = twins([x], [dy], w, b, rm, rv, "leaky")
    assert bool((got["y"] < 0).all())
    assert torch.allclose(got["db"], (dy * SLOPE).double().sum(0), rtol=1e-6, atol=0)
    assert_bound(ratios(got, v32, v64), "leaky, z < 0 everywhere")


def check_optional_tensors(device):
    n, c = T + 1, 65
    x, dy, w, b, rm, rv = inputs(n, c, device)
    got, _ = run_op([x], [dy], None, None, rm, rv, "relu")                       # no affine
    assert got["dw"] is None and got["db"] is None
    assert_bound(ratios(got, *twins([x], [dy], None, None, rm, rv, "relu")), "weight and bias NULL")
    got, stats = run_op([x], [dy], w, b, None, None, "leaky")                    # track_running_stats=False
    assert stats[0] == (None, None)
    assert_bound(ratios(got, *twins([x], [dy], w, b, None, None, "leaky")), "running statistics NULL")


def check_cumulative_average(device):
    """momentum=None: the factor is 1 / num_batches_tracked after this call's increment."""
    n, c = 63, 32
    x, dy, w, b, rm, rv = inputs(n, c, device)
    nbt = torch.tensor(3, dtype=torch.long, device=device)
    keep = nbt
    got, _ = run_op([x], [dy], w, b, rm, rv, "none", momentum=None, nbt=nbt)
    assert nbt is keep and int(nbt) == 4
    assert_bound(ratios(got, *twins([x], [dy], w, b, rm, rv, "none", factor=0.25)), "momentum=None")


def check_counter_in_place(device):
    x, dy, w, b, rm, rv = inputs(65, 3, device)
    nbt = torch.tensor(7, dtype=torch.long, device=device)
    ptr, version = nbt.data_ptr(), nbt._version
    batch_norm_rows(x, w, b, rm, rv, nbt, MOMENTUM, EPS)
    assert nbt.data_ptr() == ptr and int(nbt) == 8 and nbt._version == version + 1


def check_one_row_raises(device):
    x, dy, w, b, rm, rv = inputs(1, 3, device)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
        batch_norm_rows(x, w, b, rm, rv, None, MOMENTUM, EPS)


def check_non_fp32_synchronised(device):
    x, dy, w, b, rm, rv = inputs(5, 3, device)
    with pytest.raises(TypeError):
        batch_norm_rows(x.double(), w, b, rm, rv, None, MOMENTUM, EPS, gather=lambda r: r[None])


# ---- virtual ranks -----------------------------------------------------------------------------------------------------------
def check_virtual_ranks(device, act="relu", c=65):
    """3 T + 5 rows in chunks of 0, 1, T + 3 and the rest, one chunk per virtual rank: every rank's records are computed ahead
    with the entry points, and each rank's `gather` returns those stacks - what an all-gather would have delivered."""
    ops, tile = ops_of(device), tile_rows_of(device)
    n = 3 * tile + 5
    x, dy, w, b, rm, rv = inputs(n, c, device)
    cuts = [0, 0, 1, tile + 4, n]
    xs = [x[a:z].contiguous() for a, z in zip(cuts[:-1], cuts[1:])]
    dys = [dy[a:z].contiguous() for a, z in zip(cuts[:-1], cuts[1:])]
    assert [t.shape[0] for t in xs] == [0, 1, tile + 3, n - tile - 4]
    recs = torch.stack([ops.moments(t) for t in xs])
    total = ops.moments_merge(recs)
    mean_rstd = ops.finish(total, EPS, 0.0, None, None)
    act_id = {"none": host.ACT_NONE, "relu": host.ACT_RELU, "leaky": host.ACT_LEAKY}[act]
    sums = torch.stack([ops.bwd_sums(d, t, mean_rstd, w, b, act_id, SLOPE) for t, d in zip(xs, dys)])
    calls = []

    def gather_of(i):
        def gather(rec):
            calls.append((i, tuple(rec.shape)))
            stack = recs if rec.shape[0] == 3 else sums
            assert torch.equal(rec, stack[i]), f"rank {i}: its own record is not what it computed ahead"
            return stack
        return gather

    got, stats = run_op(xs, dys, w, b, rm, rv, act, gathers=[gather_of(i) for i in range(4)])
    assert calls == [(i, s) for i in range(4) for s in ((3, c), (2, c))], "one collective per forward, one per backward"
    assert got["y"].shape == (n, c)
    r = ratios(got, *twins(xs, dys, w, b, rm, rv, act))
    assert_bound(r, f"virtual ranks, {act}, c = {c}")
    for rmi, rvi in stats[1:]:
        assert torch.equal(rmi, stats[0][0]) and torch.equal(rvi, stats[0][1]), "the ranks' running statistics differ"
    return r


def check_misaligned(device, c=32):
    """c % 4 == 0 with x and dy 4 bytes past a 16-byte boundary: the kernels fall back to 4-byte accesses (at c = 256 with 64
    lanes along a row and four blocks of channels)."""
    from tests.grad_cases import misaligned
    assert c in MISALIGNED_C
    n = T + 1
    x, dy, w, b, rm, rv = inputs(n, c, device)
    xm, dym = misaligned(x), misaligned(dy)
    got, _ = run_op([xm], [dym], w, b, rm, rv, "relu")
    r = ratios(got, *twins([x], [dy], w, b, rm, rv, "relu"))
    assert_bound(r, f"misaligned rows, c = {c}")
    return r


def check_long_case(device, n, c, act):
    """One of LONG_CASES through `check_case`, its worst ratio noted."""
    assert (n, c, act) in LONG_CASES
    r = check_case(device, n, c, act)
    note_long(device, max(r.values()))
