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


def check_misaligned(device):
    """c % 4 == 0 with x and dy 4 bytes past a 16-byte boundary: the kernels fall back to 4-byte accesses."""
    from tests.grad_cases import misaligned
    n, c = T + 1, 32
    x, dy, w, b, rm, rv = inputs(n, c, device)
    xm, dym = misaligned(x), misaligned(dy)
    got, _ = run_op([xm], [dym], w, b, rm, rv, "relu")
    assert_bound(ratios(got, *twins([x], [dy], w, b, rm, rv, "relu")), "misaligned rows")
