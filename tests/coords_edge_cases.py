"""Edge cases of the sparse-structure layer (include/pasco_hip.h: coordinate map, kernel maps, stable compactions, row lists,
row movement, dense <-> sparse conversion, max pooling, coordinate generation), each a function of (be, dev): `be` is the C
oracle on the CPU (tests/test_coords_edges_cpu.py) or libpascohip.so on the GPU (tests/test_hip_coords_edges.py).  Every
result is held to tests/coords_ref.py: integers bit for bit, floats bit for bit (these kernels move values; scatter_add_rows
adds once per element)."""
import functools

import numpy as np
import pytest
import torch

from pasco_amd.me.backend import _ptr
from pasco_amd.me.core import kernel_offsets
from tests import coords_ref as ref

I32 = torch.int32
# block boundaries of the compactions: a tile is 2048 rows, and the scan of the tile counters carries across chunks of 256
SIZES = (1, 2047, 2048, 2049, 524287, 524288, 524289, 5_000_011)
SPECIAL = (0x7FC01234, -0x3F5432, 0x7F800000, -0x800000, -0x80000000)    # NaN, -NaN (payloads), +inf, -inf, -0.0 as int32


def same(got, exp, what=""):
    """Bit-exact equality (floats compared by their bit patterns) with the first mismatch in the message."""
    got = got.cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, tuple(got.shape), tuple(exp.shape))
    if got.dtype == torch.float32:
        got, exp = got.view(I32), exp.view(I32)
    bad = torch.nonzero((got != exp).reshape(-1)).flatten()
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {got.numel()} differ, first at flat index {int(bad[0])}: "
                              f"got {int(got.reshape(-1)[bad[0]])}, expected {int(exp.reshape(-1)[bad[0]])}")


def with_specials(shape, g, share=0.2):
    """randn values, a `share` of them replaced by NaNs with payloads, infinities and -0.0."""
    x = torch.randn(shape, generator=g)
    bits = x.view(I32).reshape(-1)
    pick = torch.rand(bits.numel(), generator=g) < share
    bits[pick] = torch.tensor(SPECIAL, dtype=I32)[torch.randint(0, len(SPECIAL), (int(pick.sum()),), generator=g)]
    return x


def insert(be, dev, coords, cap=None, dedup=True):
    """ph_map_insert into a table of `cap` slots (the backend's capacity when None) with a status word of its own
    -> (tkeys, tvals, uniq_rows, row2uniq, status)."""
    c = coords.to(device=dev, dtype=I32).contiguous()
    n = c.shape[0]
    cap = be.table_capacity(n) if cap is None else cap
    tkeys = torch.empty(cap, dtype=torch.int64, device=dev)
    tvals = torch.empty(cap, dtype=I32, device=dev)
    r2u = torch.empty(max(n, 1), dtype=I32, device=dev)
    uq = torch.empty(max(n, 1), dtype=I32, device=dev)
    nu = torch.zeros(1, dtype=I32, device=dev)
    status = torch.zeros(1, dtype=I32, device=dev)
    ws = torch.empty(int(be.fn["workspace_bytes"](n)), dtype=torch.uint8, device=dev)
    rc = be.fn["map_insert"](_ptr(c), n, _ptr(tkeys), _ptr(tvals), cap, _ptr(r2u) if dedup else None,
                             _ptr(uq) if dedup else None, _ptr(nu) if dedup else None, _ptr(ws), ws.numel(), _ptr(status),
                             be.stream(dev))
    be._check(rc, "map_insert")
    if not dedup:
        return tkeys, tvals, None, None, int(status.item())
    return tkeys, tvals, uq[: int(nu.item())], r2u[:n], int(status.item())


def check_insert(be, dev, coords, cap=None, what=""):
    """Insert, compare unique rows and row2uniq with the reference -> (tkeys, tvals, uniq coords, status)."""
    tk, tv, uq, r2u, status = insert(be, dev, coords, cap)
    uq_e, r2u_e = ref.map_insert(coords)
    same(uq, uq_e, what + " uniq_rows")
    same(r2u, r2u_e, what + " row2uniq")
    return tk, tv, coords[uq_e.long()], status


def rows_in(g, n, lo, hi, batches):
    """n random rows (b from `batches`, x, y, z in [lo, hi))."""
    b = torch.tensor(batches)[torch.randint(0, len(batches), (n,), generator=g)]
    return torch.cat([b[:, None], torch.randint(lo, hi, (n, 3), generator=g)], 1).int()


def distinct(c):
    return torch.unique(c, dim=0)


# ---- the key's range ------------------------------------------------------------------------------------------------------------
def corners():
    return torch.tensor([[b, x, y, z] for b in (0, ref.B_MAX) for x in (ref.LO, ref.HI) for y in (ref.LO, ref.HI)
                         for z in (ref.LO, ref.HI)], dtype=I32)


def key_range(be, dev):
    """All 16 corners of the key's box (the all-ones key among them) with duplicates, their inward neighbours, ordinary
    rows and rows beyond the box: every row is stored and found, or flagged (status bit 1), left out of the map and
    answered with -1.  Nothing aliases, and no neighbour is found across the edge of the range."""
    g = torch.Generator().manual_seed(1)
    cor = corners()
    inward = cor.clone()
    inward[:, 1:] += torch.where(cor[:, 1:] == ref.HI, -1, 1).int()
    beyond = torch.tensor([[1024, 1, 2, 3], [-1, 1, 2, 3], [0, ref.HI + 1, 2, 3], [0, 1, ref.LO - 1, 3], [7, 1, 2, 1 << 18],
                           list(ref.ALL_ONES)], dtype=I32)
    ordinary = torch.cat([rows_in(g, 3000, -300, 300, list(range(1024))), torch.tensor([[0, 1, 2, 3]], dtype=I32)])
    coords = torch.cat([cor, cor, cor, inward, inward, beyond, beyond, ordinary])
    coords = coords[torch.randperm(coords.shape[0], generator=g)].contiguous()
    tk, tv, uc, status = check_insert(be, dev, coords, what="corners")
    assert status & 2, "rows beyond the key's range were not flagged"
    bad = ~ref.packable(coords)
    assert int(bad.sum()) == 2 * beyond.shape[0] + 3                 # + the all-ones corner, three times
    q = torch.cat([coords, cor, inward, beyond, cor + torch.tensor([1, 0, 0, 0], dtype=I32), cor - torch.tensor([1, 0, 0, 0],
                                                                                                         dtype=I32)])
    got = be.map_find(q.to(dev).contiguous(), tk, tv)
    same(got, ref.map_find(coords, q), "map_find")
    assert bool((got.cpu()[: coords.shape[0]][bad] == -1).all())
    offs = [(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 1, 1), (-1, -1, -1)]
    out = distinct(torch.cat([cor, inward]))
    same(be.nbr_build(out.to(dev), tk, tv, offs), ref.nbr_table(out, uc, offs), "nbr_build at the edges")
    _, _, _, status = check_insert(be, dev, coords[~bad].contiguous(), what="inside the range")
    assert status == 0, "a coordinate inside the key's range was flagged"


# ---- hash probing ---------------------------------------------------------------------------------------------------------------
def colliding(cap, slot, count, seed):
    """`count` distinct packable rows whose probe starts at `slot` of a `cap`-slot table (found by sampling)."""
    rng = np.random.default_rng(seed)
    found = np.zeros((0, 4), np.int64)
    while found.shape[0] < count:
        c = np.concatenate([rng.integers(0, 1024, (1 << 20, 1)), rng.integers(ref.LO, ref.HI, (1 << 20, 3))], 1)
        found = np.unique(np.concatenate([found, c[ref.home_slot(c, cap) == slot]]), axis=0)
    return torch.from_numpy(found[rng.permutation(found.shape[0])[:count]]).int()


def hash_probing(be, dev):
    """Chains of >= 64 keys on one home slot that wrap from cap - 1 to 0, tables at exactly cap = 2n and the smallest table
    (n = 1, cap = 2); misses that probe through such chains end with -1."""
    g = torch.Generator().manual_seed(2)
    for n, cap in ((64, 128), (4096, 8192)):
        chain = colliding(cap, cap - 1, 128, seed=cap)               # 64 inserted, 64 misses probing the whole chain
        inside = colliding(cap, 5, 16, seed=cap + 1)                 # misses starting inside the wrapped part of the chain
        keys = distinct(torch.cat([chain, inside, rows_in(g, 2 * n, -5000, 5000, [0, 3, 1023])]))
        keys = keys[torch.randperm(keys.shape[0], generator=g)]
        is_probe = (keys[:, None, :] == torch.cat([chain[64:], inside])[None]).all(-1).any(-1)
        ins = torch.cat([chain[:64], keys[~is_probe & ~(keys[:, None, :] == chain[None]).all(-1).any(-1)][: n - 64]])
        ins = ins[torch.randperm(n, generator=g)].contiguous()
        assert ins.shape[0] == n and (ref.home_slot(chain, cap) == cap - 1).all()
        misses = torch.cat([chain[64:], inside])
        tk, tv, _, _ = check_insert(be, dev, ins, cap=cap, what=f"cap {cap} = 2n")
        q = torch.cat([ins, misses]).contiguous()
        same(be.map_find(q.to(dev), tk, tv), ref.map_find(ins, q), f"map_find cap {cap}")
        # the same table without dedup (rows keep their index), and duplicates in a chain at cap = 2n
        tk, tv, *_ = insert(be, dev, ins, cap=cap, dedup=False)
        same(be.map_find(q.to(dev), tk, tv), torch.cat([torch.arange(n), torch.full((misses.shape[0],), -1)]).int(),
             f"map_find cap {cap} (unique rows)")
        dup = chain[:32].repeat(2, 1)
        dup = dup[torch.randperm(64, generator=g)].contiguous()
        tk, tv, _, _ = check_insert(be, dev, dup, cap=128 if n == 64 else cap, what="duplicates in one chain")
    one = torch.tensor([[3, -7, 11, 2]], dtype=I32)
    misses = torch.cat([colliding(2, 0, 8, seed=5), colliding(2, 1, 8, seed=6)])
    tk, tv, _, _ = check_insert(be, dev, one, cap=2, what="n = 1, cap = 2")
    q = torch.cat([one, misses]).contiguous()
    same(be.map_find(q.to(dev), tk, tv), ref.map_find(one, q), "map_find cap 2")


def first_occurrence_under_contention(be, dev):
    """> 10^6 rows over 5 coordinates, interleaved so that every workgroup races on every key: the unique rows are the
    first occurrences, in input order."""
    keys = torch.tensor([[0, 0, 0, 0], [1023, ref.HI, ref.HI, ref.HI - 1], [5, -7, 3, ref.LO], [5, -7, 3, ref.LO + 1],
                         [0, 1, 0, 0]], dtype=I32)
    n = (1 << 20) + 37
    g = torch.Generator().manual_seed(3)
    interleaved = (torch.arange(n) * 3 + 2) % 5
    late = torch.randint(0, 4, (n,), generator=g)
    late[n - 5] = late[n - 1] = 4                                    # the last key appears only at the very end
    for name, pattern in (("interleaved", interleaved), ("random, one key late", late)):
        _, _, uc, _ = check_insert(be, dev, keys[pattern].contiguous(), what=name)
        assert uc.shape[0] == 5


# ---- block boundaries of the compactions ----------------------------------------------------------------------------------------
def masks(n, seed):
    g = torch.Generator().manual_seed(seed)
    yield "zeros", torch.zeros(n, dtype=torch.uint8)
    yield "ones", torch.ones(n, dtype=torch.uint8)
    yield "alternating", (torch.arange(n) % 2).to(torch.uint8)
    yield "random", (torch.randint(0, 4, (n,), generator=g) * 85).to(torch.uint8)      # any non-zero byte keeps
    last = torch.zeros(n, dtype=torch.uint8)
    last[-1] = 7
    yield "last only", last


def compactions(be, dev, n):
    """mask_compact and mask_compact_rank across tile and scan-chunk boundaries."""
    for name, m in masks(n, n):
        keep_e, rank_e = ref.compact(m)
        md = m.to(dev)
        same(be.mask_compact(md), keep_e, f"mask_compact n={n} {name}")
        keep = torch.empty(max(n, 1), dtype=I32, device=dev)
        rank = torch.empty(n, dtype=I32, device=dev)
        cnt = torch.empty(1, dtype=I32, device=dev)
        ws = torch.empty(int(be.fn["workspace_bytes"](n)), dtype=torch.uint8, device=dev)
        be._check(be.fn["mask_compact_rank"](_ptr(md), n, _ptr(keep), _ptr(rank), _ptr(cnt), _ptr(ws), ws.numel(),
                                             be.stream(dev)), "mask_compact_rank")
        same(keep[: int(cnt.item())], keep_e, f"mask_compact_rank n={n} {name} rows")
        same(rank, rank_e, f"mask_compact_rank n={n} {name} rank_of")


def map_insert_blocks(be, dev, n):
    """First-occurrence dedup across the same boundaries (about half the rows repeat an earlier one)."""
    g = torch.Generator().manual_seed(n)
    pool = rows_in(g, n // 2 + 1, -3000, 3000, list(range(8)))
    coords = pool[torch.randint(0, pool.shape[0], (n,), generator=g)].contiguous()
    check_insert(be, dev, coords, what=f"map_insert n={n}")


def kmap_blocks(be, dev, n, kvol):
    """ph_kmap_compact: kvol segments of n rows, each segment its own scan; one segment empty, one full where kvol allows."""
    g = torch.Generator().manual_seed(n + kvol)
    dens = (torch.arange(kvol, dtype=torch.float32) + 0.5) / kvol
    hit = torch.rand(kvol, n, generator=g) < dens[:, None]
    if kvol > 2:
        hit[0], hit[1] = False, True
    nbr = torch.where(hit, torch.randint(0, 1 << 30, (kvol, n), generator=g, dtype=I32), torch.tensor(-1, dtype=I32))
    pin, pout, cnt = be.kmap_compact(nbr.to(dev))
    ks, js, pi, po, cnt_e = ref.kmap_coo(nbr)
    same(cnt, cnt_e, f"kmap_compact n={n} kvol={kvol} counts")
    same(pin.cpu()[ks, js], pi, f"kmap_compact n={n} kvol={kvol} pairs_in")
    same(pout.cpu()[ks, js], po, f"kmap_compact n={n} kvol={kvol} pairs_out")


def to_sparse_grid(be, dev):
    """to_sparse_coords on a [3, 256, 256, 32] grid (6.3 M sites, 24 scan chunks) under the compaction masks; dropped sites
    hold 0 or -0.0, kept ones any non-zero channel - NaN alone included."""
    n = 3 * 256 * 256 * 32
    g = torch.Generator().manual_seed(4)
    for name, m in masks(n, 4):
        keep = m != 0
        v = torch.randn(n, 2, generator=g)
        v[torch.rand(n, 2, generator=g) < 0.4] = 0.0
        v[keep & (v == 0).all(1), 1] = 1.5
        v[keep & (torch.arange(n) % 7 == 0)] = torch.tensor([0.0, float("nan")])
        v[~keep] = 0.0
        v[~keep & (torch.arange(n) % 3 == 0)] = -0.0
        dense = v.reshape(3, 256, 256, 32, 2).permute(0, 4, 1, 2, 3).contiguous()
        coords, feats = be.to_sparse(dense.to(dev))
        exp = ref.to_sparse_coords(dense)
        assert exp.shape[0] == int(keep.sum())
        same(coords, exp, f"to_sparse {name} coords")
        same(feats, ref.dense_gather(dense, exp), f"to_sparse {name} feats")


# ---- kernel maps ----------------------------------------------------------------------------------------------------------------
def nbr_batches(be, dev):
    """Several batches holding the same xyz (each a different subset): no neighbour across batches; negative coordinates."""
    g = torch.Generator().manual_seed(5)
    xyz = distinct(torch.randint(-40, 40, (4000, 3), generator=g, dtype=I32))
    coords = torch.cat([torch.cat([torch.full((xyz.shape[0], 1), b, dtype=I32), xyz], 1)[torch.rand(xyz.shape[0], generator=g) < 0.7]
                        for b in (0, 1, 7, 1023)])
    coords = coords[torch.randperm(coords.shape[0], generator=g)].contiguous()
    tk, tv, uc, _ = check_insert(be, dev, coords, what="batches")
    out = torch.cat([torch.cat([torch.full((xyz.shape[0], 1), b, dtype=I32), xyz], 1) for b in (0, 1, 2, 7, 1023)])
    for offs in (kernel_offsets(3, 1), kernel_offsets(2, 1), kernel_offsets(4, 1)):
        same(be.nbr_build(out.to(dev), tk, tv, offs), ref.nbr_table(out, uc, offs), f"nbr_build batches kvol={len(offs)}")


def nbr_strides(be, dev):
    """Tensor strides 2, 4, 8 (offsets scaled), strided and transposed kernel maps, kvol = 64, negative coordinates."""
    g = torch.Generator().manual_seed(6)
    for ts in (2, 4, 8):
        base = distinct(rows_in(g, 3000, -20, 20, [0, 3]))
        coords = base.clone()
        coords[:, 1:] *= ts
        coords = coords[torch.randperm(coords.shape[0], generator=g)].contiguous()
        tk, tv, uc, _ = check_insert(be, dev, coords, what=f"ts={ts}")
        out = distinct(ref.coords_floor(coords, 2 * ts))
        kids = ref.coords_expand(coords, ts // 2)
        for name, o, offs in (("k3", coords, kernel_offsets(3, ts)), ("k2 down", out, kernel_offsets(2, ts)),
                              ("k4", coords, kernel_offsets(4, ts)),
                              ("k2 transposed", kids, kernel_offsets(2, ts // 2, transposed=True)),
                              ("k3 dilated", coords, kernel_offsets(3, ts, 2))):
            same(be.nbr_build(o.to(dev), tk, tv, offs), ref.nbr_table(o, uc, offs), f"nbr_build ts={ts} {name}")


def nbr_same_map(be, dev):
    """nbr_build_same (half the probes, mirrored writes) against the dict reference: dilation 1, 2, 3 and a (3, 1, 3) kernel."""
    g = torch.Generator().manual_seed(7)
    for ks, dil in ((3, 1), (3, 2), (3, 3), ((3, 1, 3), 1), ((3, 1, 3), 2), (1, 1)):
        c = distinct(rows_in(g, 6000, -12, 12, [0, 1, 2]))
        c = c[torch.randperm(c.shape[0], generator=g)].contiguous()
        tk, tv, *_ = insert(be, dev, c, dedup=False)
        offs = kernel_offsets(ks, 1, dil)
        same(be.nbr_build(c.to(dev), tk, tv, offs, same_map=True), ref.nbr_table(c, c, offs), f"nbr_build_same {ks} dil {dil}")


def rowlist_pack(be, dev, pin, pout, cnt, n_out, cap, tcap):
    kvol = pin.shape[0]
    fill = 0x5A5A5A5A                                   # entries the pack must write
    rl_in = torch.full((cap,), fill, dtype=I32, device=dev)
    rl_out = torch.full((cap,), fill, dtype=I32, device=dev)
    tile_k = torch.full((tcap,), fill, dtype=I32, device=dev)
    status = torch.zeros(1, dtype=I32, device=dev)
    be._check(be.fn["rowlist_pack"](_ptr(pin), _ptr(pout), _ptr(cnt), kvol, n_out, _ptr(rl_in), _ptr(rl_out), _ptr(tile_k), cap,
                                    tcap, _ptr(status), be.stream(dev)), "rowlist_pack")
    return rl_in, rl_out, tile_k, int(status.item())


def check_rowlist(be, dev, nbr, what, one_pair):
    kvol, n_out = nbr.shape
    pin, pout, cnt = be.kmap_compact(nbr.to(dev))
    ks, js, pi, po, cnt_e = ref.kmap_coo(nbr)
    pi_m = torch.full((kvol, max(n_out, 1)), -1, dtype=I32)
    po_m = pi_m.clone()
    pi_m[ks, js], po_m[ks, js] = pi, po
    cap = ref.rowlist_min_cap(n_out, kvol)
    for tcap in (cap // 128, cap // 128 + 3):
        got = rowlist_pack(be, dev, pin, pout, cnt, n_out, cap, tcap)
        for a, b, name in zip(got[:3], ref.rowlist_pack(pi_m, po_m, cnt_e, cap, tcap), ("rl_in", "rl_out", "tile_k")):
            same(a, b, f"rowlist {what} cap={cap} tcap={tcap} {name}")
        assert bool(got[3] & 32) == (not one_pair), f"rowlist {what}: status {got[3]}"


def rowlists(be, dev):
    """ph_rowlist_pack at the smallest capacity its check accepts; status bit 32 exactly when the map breaks
    one-pair-per-row."""
    g = torch.Generator().manual_seed(8)
    par = distinct(rows_in(g, 700, -30, 30, [0, 2]))
    par[:, 1:] *= 2
    kids = ref.coords_expand(par, 1)
    nbr = ref.nbr_table(kids, par, kernel_offsets(2, 1, transposed=True))   # generative: one parent per child
    assert bool(((nbr >= 0).sum(0) == 1).all())
    check_rowlist(be, dev, nbr, "generative", True)
    fewer = nbr.clone()
    fewer[:, ::7] = -1
    check_rowlist(be, dev, fewer, "rows without a pair", False)
    more = nbr.clone()
    counts = (nbr >= 0).sum(1)
    k = int(torch.nonzero((128 - counts % 128) % 128 >= 3).flatten()[0])   # 3 more pairs fit in k's padding
    free = torch.nonzero(nbr[k] < 0).flatten()[:3]
    more[k, free] = 0
    check_rowlist(be, dev, more, "rows with two pairs", False)
    for kvol in (1, 27, 64):
        for n_out in (1, 127, 128, 129, 1000):
            nbr = torch.full((kvol, n_out), -1, dtype=I32)
            nbr[torch.randint(0, kvol, (n_out,), generator=g), torch.arange(n_out)] = torch.randint(0, 5000, (n_out,), generator=g,
                                                                                                    dtype=I32)
            check_rowlist(be, dev, nbr, f"kvol={kvol} n_out={n_out}", True)


# ---- rows, dense conversion and pooling -----------------------------------------------------------------------------------------
def gather_rows(be, dev):
    """gather_rows with -1 rows, c in {1, 3, 4, 5, 64}, aligned (the float4 path when c % 4 == 0) and unaligned source or
    destination views; NaN payloads, infinities and -0.0 copied bit for bit; nothing written around the destination."""
    g = torch.Generator().manual_seed(9)
    n, m = 777, 1500
    fill = torch.tensor([0x7FBADBAD], dtype=I32).view(torch.float32)
    for c in (1, 3, 4, 5, 64):
        rows = torch.randint(-n // 2, n, (m,), generator=g).clamp(min=-1).int()
        rows[:2] = torch.tensor([0, n - 1])
        flat = with_specials((n * c + 1,), g)
        for src_off in (0, 1):
            src = flat[src_off:src_off + n * c].view(n, c).to(dev)
            exp = ref.gather_rows(src.cpu(), rows)
            for dst_off in (4, 1):
                buf = fill.repeat(m * c + 8).to(dev)
                out = buf[dst_off:dst_off + m * c].view(m, c)
                be.gather_rows(src, rows.to(dev), out=out)
                same(out, exp, f"gather_rows c={c} src+{src_off} dst+{dst_off}")
                rest = torch.cat([buf[:dst_off], buf[dst_off + m * c:]]).cpu()
                same(rest, fill.repeat(rest.numel()), f"gather_rows c={c}: written outside the destination")


def scatter_add(be, dev):
    g = torch.Generator().manual_seed(10)
    for c in (1, 5, 64):
        n_dst, n_src = 3000, 2000
        rows = torch.randperm(n_dst, generator=g)[:n_src].int()
        rows[torch.rand(n_src, generator=g) < 0.2] = -1
        src = torch.randn(n_src, c, generator=g)
        dst = torch.randn(n_dst, c, generator=g)
        dst[::13] = float("inf")
        dst[5::17] = -0.0
        src[5::17] = -0.0
        got = be.scatter_add_rows(src.to(dev), rows.to(dev), dst.clone().to(dev))
        same(got, ref.scatter_add_rows(src, rows, dst), f"scatter_add_rows c={c}")


def dense_conversion(be, dev):
    """to_dense with ts 1, 2, 4 (floor division of coordinates below the box's minimum), the [-dim, 0) wrap, batches and rows
    out of the box; then to_sparse and dense_gather.  Values carried bit for bit.

    to_sparse keeps a site when any channel is != 0 (include/pasco_hip.h): a site whose only non-zero channel is NaN is
    kept, a site of -0.0 dropped.  MinkowskiEngine is not available to the tests, so this rule is checked against the
    header's statement, not against upstream's implementation."""
    g = torch.Generator().manual_seed(11)
    B, X, Y, Z = 2, 9, 7, 5
    dim = torch.tensor([X, Y, Z])
    min3 = (-10, 3, -4)
    for ts in (1, 2, 4):
        sites = torch.nonzero(torch.rand(B, X, Y, Z, generator=g) < 0.6).int()
        wrap = torch.rand(sites.shape[0], 3, generator=g) < 0.25
        s = torch.where(wrap, sites[:, 1:] - dim, sites[:, 1:])                 # [-dim, 0) lands on the same site
        out_s = torch.tensor([[0, -X - 1, 0, 0], [1, 0, Y, 0], [0, 0, 0, -Z - 3], [1, X + 4, -Y - 1, 2]], dtype=I32)
        out_b = torch.tensor([[-1, 1, 1, 1], [B, 2, 2, 2], [1023, 0, 0, 0]], dtype=I32)
        site_rows = torch.cat([torch.cat([sites[:, :1], s], 1), out_s, out_b])
        r = torch.randint(0, ts, (site_rows.shape[0], 3), generator=g, dtype=I32)
        coords = site_rows.clone()
        coords[:, 1:] = torch.tensor(min3, dtype=I32) + site_rows[:, 1:] * ts + r
        perm = torch.randperm(coords.shape[0], generator=g)
        coords = coords[perm].int().contiguous()
        feats = with_specials((coords.shape[0], 3), g)
        feats[0] = torch.tensor([0.0, float("nan"), 0.0])
        feats[1] = -0.0
        dense = be.to_dense(feats.to(dev), coords.to(dev), min3, ts, (B, X, Y, Z))
        exp = ref.to_dense(feats, coords, min3, ts, (B, X, Y, Z))
        same(dense, exp, f"to_dense ts={ts}")
        sc, sf = be.to_sparse(dense)
        sc_e = ref.to_sparse_coords(exp)
        same(sc, sc_e, f"to_sparse ts={ts} coords")
        same(sf, ref.dense_gather(exp, sc_e), f"to_sparse ts={ts} feats")
        q = torch.cat([sc_e, torch.tensor([[0, -1, 0, 0], [0, X, 0, 0], [B, 0, 0, 0], [-1, 0, 0, 0], [1, 0, Y, Z - 1]], dtype=I32),
                       rows_in(g, 300, -2, 10, [0, 1])])
        same(be.dense_gather(dense, q.to(dev)), ref.dense_gather(exp, q), f"dense_gather ts={ts}")


def maxpool(be, dev):
    """maxpool_fwd with all-negative rows, rows without any neighbour and c not a multiple of 4."""
    g = torch.Generator().manual_seed(12)
    n_in, n_out = 500, 700
    for c, kvol in ((3, 8), (5, 27), (7, 64), (64, 8)):
        x = torch.randn(n_in, c, generator=g)
        x[x == 0] = 0.5
        x[::4] = -(x[::4].abs() + 0.01)
        nbr = torch.randint(0, n_in, (kvol, n_out), generator=g, dtype=I32)
        nbr[torch.rand(kvol, n_out, generator=g) < 0.5] = -1
        nbr[:, ::9] = -1
        sel = nbr[:, 1::9]
        nbr[:, 1::9] = torch.where(sel >= 0, sel // 4 * 4, sel)        # only all-negative input rows
        same(be.maxpool_fwd(x.to(dev), nbr.to(dev)), ref.maxpool(x, nbr), f"maxpool c={c} kvol={kvol}")


def coords_generation(be, dev):
    """coords_floor / coords_expand with Python integer division, negative coordinates and the edges of the key's range."""
    g = torch.Generator().manual_seed(13)
    c = torch.cat([rows_in(g, 2000, -50, 50, [0, 1, 1023]),
                   torch.tensor([[0, ref.LO, ref.LO + 1, -1], [1, ref.HI, ref.HI - 7, 0], [2, -8, -9, 7]], dtype=I32)])
    for ts in (1, 2, 3, 4, 8):
        same(be.coords_floor(c.to(dev), ts), ref.coords_floor(c, ts), f"coords_floor ts={ts}")
        same(be.coords_expand(c.to(dev), ts), ref.coords_expand(c, ts), f"coords_expand ts={ts}")


def unique_rows_sorted(be, dev):
    """pasco_amd.graph.unet.unique_rows_sorted equals torch.unique(dim=0, return_inverse=True) for batches up to 1023 and
    coordinates at the edges of the key's range; rows it cannot pack raise."""
    from pasco_amd.graph.unet import unique_rows_sorted as urs
    g = torch.Generator().manual_seed(14)
    for k in (3, 4):
        r = rows_in(g, 5000, -60, 60, [0, 1, 511, 512, 600, 1023])
        r = torch.cat([r, corners(), corners(), torch.tensor([[600, 0, 0, 0], [0, 0, 0, 0]], dtype=I32)])[:, 4 - k:]
        r = r[torch.randperm(r.shape[0], generator=g)].contiguous()
        u0, i0 = torch.unique(r, dim=0, return_inverse=True)
        u1, i1 = urs(r.to(dev))
        same(u1, u0, f"unique_rows_sorted [N, {k}] rows")
        same(i1, i0, f"unique_rows_sorted [N, {k}] inverse")
    for bad in ([1024, 0, 0, 0], [-1, 0, 0, 0], [0, ref.HI + 1, 0, 0], [0, 0, ref.LO - 1, 0], [0, 0, 0, 1 << 20]):
        with pytest.raises(ValueError):
            urs(torch.tensor([[0, 0, 0, 0], bad], dtype=I32).to(dev))


def _case(fn, **kw):
    f = functools.partial(fn, **kw)
    return pytest.param(f, id="-".join([fn.__name__] + [f"{k}{v}" for k, v in kw.items()]))


CASES = ([_case(key_range), _case(hash_probing), _case(first_occurrence_under_contention)]
         + [_case(compactions, n=n) for n in SIZES] + [_case(map_insert_blocks, n=n) for n in SIZES]
         + [_case(kmap_blocks, n=n, kvol=k) for n in SIZES for k in (1, 8)]
         + [_case(kmap_blocks, n=n, kvol=k) for n in (1, 2049, 524287, 524289) for k in (27, 64)]
         + [_case(to_sparse_grid), _case(nbr_batches), _case(nbr_strides), _case(nbr_same_map), _case(rowlists),
            _case(gather_rows), _case(scatter_add), _case(dense_conversion), _case(maxpool), _case(coords_generation),
            _case(unique_rows_sorted)])
