"""Plain torch / numpy restatement of the sparse-structure layer of include/pasco_hip.h - coordinate map, lookups, kernel
maps, stable compactions, row lists, row movement, dense <-> sparse conversion, max pooling and coordinate generation -
written from the header's contracts with a lexicographic sort, `torch.nonzero` and boolean masks.  The checker of
csrc/coords.hip and csrc/rows.hip (and of the C oracle, which restates the same layer): nothing here calls either.

No expected answer goes through a 64-bit key.  `pack` and `home_slot` (the key packing and the hash mixer, in numpy
uint64) exist only to CONSTRUCT inputs - keys that share one home slot of a table, chains that wrap past its last slot.
"""
import numpy as np
import torch

LO, HI = -(1 << 17), (1 << 17) - 1        # coordinate range of the key
B_MAX = 1023                               # largest batch index of the key
ALL_ONES = (B_MAX, HI, HI, HI)             # the one coordinate in that box whose key is the table's empty marker


# ---- coordinate map -------------------------------------------------------------------------------------------------------------
def groups(rows):
    """Numbering of the distinct rows of [N, 4] (through one lexicographic sort) -> (id of every row, number of ids)."""
    r = torch.as_tensor(rows).long().reshape(-1, 4).numpy()
    if r.shape[0] == 0:
        return torch.zeros(0, dtype=torch.int64), 0
    order = np.lexsort(r.T[::-1])
    s = r[order]
    new = np.ones(s.shape[0], dtype=bool)
    new[1:] = (s[1:] != s[:-1]).any(axis=1)
    gid = np.cumsum(new) - 1
    inv = np.empty(s.shape[0], dtype=np.int64)
    inv[order] = gid
    return torch.from_numpy(inv), int(gid[-1]) + 1


def packable(c):
    """[N, 4] (b, x, y, z) -> bool [N]: what a map can hold (include/pasco_hip.h ph_map_insert)."""
    c = torch.as_tensor(c).long().reshape(-1, 4)
    ok = (c[:, 0] >= 0) & (c[:, 0] <= B_MAX) & ((c[:, 1:] >= LO) & (c[:, 1:] <= HI)).all(dim=1)
    return ok & ~(c == torch.tensor(ALL_ONES)).all(dim=1)


def map_insert(coords):
    """First-occurrence dedup: -> (uniq_rows int32 [U], row2uniq int32 [N]).  Unique rows keep their input order; a row
    that cannot be packed is no unique row and its row2uniq is -1."""
    c = torch.as_tensor(coords).long().reshape(-1, 4)
    n = c.shape[0]
    row2uniq = torch.full((n,), -1, dtype=torch.int64)
    idx = torch.nonzero(packable(c)).flatten()
    if idx.numel() == 0:
        return torch.zeros(0, dtype=torch.int32), row2uniq.int()
    inv, ng = groups(c[idx])
    first = torch.full((ng,), n, dtype=torch.int64).scatter_reduce(0, inv, idx, "amin")
    order = torch.argsort(first)
    rank = torch.empty_like(order)
    rank[order] = torch.arange(order.numel())
    row2uniq[idx] = rank[inv]
    return first[order].int(), row2uniq.int()


def lookup(keys, vals, queries):
    """vals[j] of the row j of `keys` equal to each query, -1 where there is none or the query cannot be packed (a dict
    lookup, vectorised through one numbering of keys and queries).  The rows of `keys` must be distinct."""
    k = torch.as_tensor(keys).long().reshape(-1, 4)
    q = torch.as_tensor(queries).long().reshape(-1, 4)
    vals = torch.as_tensor(vals).long()
    out = torch.full((q.shape[0],), -1, dtype=torch.int64)
    if k.shape[0] == 0 or q.shape[0] == 0:
        return out.int()
    inv, ng = groups(torch.cat([k, q]))
    assert int(torch.unique(inv[: k.shape[0]]).numel()) == k.shape[0], "lookup keys must be distinct"
    table = torch.full((ng,), -1, dtype=torch.int64)
    table[inv[: k.shape[0]]] = vals
    out = table[inv[k.shape[0]:]]
    out[~packable(q)] = -1
    return out.int()


def map_find(coords, queries):
    """Unique row of every query in the map built from `coords` (map_insert), -1 when absent."""
    c = torch.as_tensor(coords).long().reshape(-1, 4)
    uniq_rows, _ = map_insert(c)
    return lookup(c[uniq_rows.long()], torch.arange(uniq_rows.numel()), queries)


def nbr_table(out_coords, in_coords, offsets):
    """nbr[k][o] = row of in_coords (distinct) at out_coords[o] + offsets[k], within the same batch; -1 when absent."""
    o = torch.as_tensor(out_coords).long().reshape(-1, 4)
    off = torch.as_tensor(offsets, dtype=torch.int64).reshape(-1, 3)
    q = o[None, :, :].repeat(off.shape[0], 1, 1)
    q[:, :, 1:] += off[:, None, :]
    n_in = int(torch.as_tensor(in_coords).reshape(-1, 4).shape[0])
    return lookup(in_coords, torch.arange(n_in), q.reshape(-1, 4)).reshape(off.shape[0], -1)


# ---- compactions ----------------------------------------------------------------------------------------------------------------
def compact(mask):
    """-> (keep_rows int32 [n_keep], rank_of int32 [N]): the kept positions in order, every position's rank or -1."""
    m = torch.as_tensor(mask).reshape(-1) != 0
    keep = torch.nonzero(m).flatten()
    rank_of = torch.full((m.numel(),), -1, dtype=torch.int64)
    rank_of[keep] = torch.arange(keep.numel())
    return keep.int(), rank_of.int()


def kmap_coo(nbr):
    """COO kernel map, per offset k the (in_row, out_row) pairs in ascending out_row -> (ks, js, pairs_in, pairs_out,
    counts): pair js[i] of offset ks[i] is (pairs_in[i], pairs_out[i])."""
    nbr = torch.as_tensor(nbr)
    k, o = torch.nonzero(nbr >= 0, as_tuple=True)        # row-major: ascending o within every k
    counts = torch.bincount(k, minlength=nbr.shape[0])
    starts = torch.cumsum(counts, 0) - counts
    j = torch.arange(k.numel()) - starts[k]
    return k, j, nbr[k, o].int(), o.int(), counts.int()


def rowlist_min_cap(n_out, kvol):
    """The smallest list capacity ph_rowlist_pack accepts: a multiple of 128 >= n_out + (127 kvol rounded down to 128)."""
    need = n_out + kvol * 127 - (kvol * 127) % 128
    return (need + 127) // 128 * 128


def rowlist_pack(pairs_in, pairs_out, counts, cap, tcap):
    """Padded row lists of a COO map (include/pasco_hip.h ph_rowlist_pack): offset k's pairs at [off_k, off_k +
    counts[k]), off_k = sum_{j<k} roundup128(counts[j]), -1 padding; tile t -> its offset, -1 past the last tile.
    pairs_in / pairs_out [K, >= max count].  -> (rl_in, rl_out, tile_k)."""
    rl_in = torch.full((cap,), -1, dtype=torch.int32)
    rl_out = torch.full((cap,), -1, dtype=torch.int32)
    tile_k = torch.full((tcap,), -1, dtype=torch.int32)
    pos = 0
    for k, c in enumerate(torch.as_tensor(counts).tolist()):
        rl_in[pos:pos + c] = pairs_in[k, :c]
        rl_out[pos:pos + c] = pairs_out[k, :c]
        padded = (c + 127) // 128 * 128
        tile_k[pos // 128:(pos + padded) // 128] = k
        pos += padded
    assert pos <= cap, "the lists do not fit"
    return rl_in, rl_out, tile_k


# ---- rows -----------------------------------------------------------------------------------------------------------------------
def gather_rows(src, rows):
    """out[j] = src[rows[j]], +0.0 for rows[j] < 0.  Bit patterns are copied, NaN payloads included."""
    src = torch.as_tensor(src)
    rows = torch.as_tensor(rows).long()
    out = torch.zeros((rows.numel(), src.shape[1]), dtype=src.dtype)
    ok = rows >= 0
    out[ok] = src[rows[ok]]
    return out


def scatter_add_rows(src, rows, dst):
    """dst[rows[i]] += src[i] for rows[i] >= 0; the targets are distinct, so one fp32 add per element."""
    out = torch.as_tensor(dst).clone()
    rows = torch.as_tensor(rows).long()
    ok = rows >= 0
    assert int(torch.unique(rows[ok]).numel()) == int(ok.sum()), "the reference takes distinct targets"
    out[rows[ok]] += torch.as_tensor(src)[ok]
    return out


# ---- dense <-> sparse -----------------------------------------------------------------------------------------------------------
def to_dense(feats, coords, min3, ts, dims4):
    """dense [B, C, X, Y, Z]: site floor((p - min) / ts) per axis; an index in [-dim, 0) wraps python-style, anything
    further out (or a batch outside 0 .. B-1) is skipped.  The rows that land must land on distinct sites."""
    f = torch.as_tensor(feats)
    c = torch.as_tensor(coords).long()
    B, X, Y, Z = dims4
    dense = torch.zeros((B, f.shape[1], X, Y, Z), dtype=f.dtype)
    s = torch.div(c[:, 1:] - torch.tensor(min3), ts, rounding_mode="floor")
    dim = torch.tensor([X, Y, Z])
    s = torch.where(s < 0, s + dim, s)
    ok = (c[:, 0] >= 0) & (c[:, 0] < B) & ((s >= 0) & (s < dim)).all(dim=1)
    b, s, fv = c[ok, 0], s[ok], f[ok]
    lin = ((b * X + s[:, 0]) * Y + s[:, 1]) * Z + s[:, 2]
    assert int(torch.unique(lin).numel()) == lin.numel(), "the reference takes distinct sites"
    dense.permute(0, 2, 3, 4, 1)[b, s[:, 0], s[:, 1], s[:, 2]] = fv
    return dense


def to_sparse_coords(dense):
    """Sites (b, x, y, z) with any channel != 0, in lexicographic order: NaN counts as non-zero, -0.0 does not."""
    return torch.nonzero((torch.as_tensor(dense) != 0).any(dim=1)).int()


def dense_gather(dense, site_coords):
    """feats[i] = dense[b, :, x, y, z] of site i, +0.0 for a site outside the grid."""
    d = torch.as_tensor(dense)
    s = torch.as_tensor(site_coords).long().reshape(-1, 4)
    B, C, X, Y, Z = d.shape
    ok = ((s >= 0) & (s < torch.tensor([B, X, Y, Z]))).all(dim=1)
    out = torch.zeros((s.shape[0], C), dtype=d.dtype)
    q = s[ok]
    out[ok] = d.permute(0, 2, 3, 4, 1)[q[:, 0], q[:, 1], q[:, 2], q[:, 3]]
    return out


# ---- pooling and coordinate generation ------------------------------------------------------------------------------------------
def maxpool(x, nbr):
    """out[o] = max over the neighbours of o, 0 for a row without any (for x without NaN or -0.0)."""
    x = torch.as_tensor(x)
    nbr = torch.as_tensor(nbr).long()
    g = torch.where((nbr >= 0)[:, :, None], x[nbr.clamp(min=0)], torch.tensor(float("-inf")))
    out = g.amax(dim=0)
    out[~(nbr >= 0).any(dim=0)] = 0.0
    return out


def coords_floor(coords, ts):
    """(b, x, y, z) -> (b, (x // ts) ts, ...) with Python's floor division."""
    return torch.tensor([[r[0]] + [v // ts * ts for v in r[1:]] for r in torch.as_tensor(coords).tolist()],
                        dtype=torch.int32).reshape(-1, 4)


def coords_expand(coords, ts):
    """Every row -> its 8 children c + {0, 1}^3 ts, x fastest."""
    return torch.tensor([[r[0], r[1] + (k & 1) * ts, r[2] + (k >> 1 & 1) * ts, r[3] + (k >> 2 & 1) * ts]
                         for r in torch.as_tensor(coords).tolist() for k in range(8)], dtype=torch.int32).reshape(-1, 4)


# ---- input construction only ----------------------------------------------------------------------------------------------------
def pack(c):
    """numpy uint64 keys of int rows [N, 4] (10 bits batch, 18 bits per axis biased by 2^17)."""
    c = np.asarray(c, dtype=np.int64).reshape(-1, 4)
    u = [(c[:, i] + (0 if i == 0 else 1 << 17)).astype(np.uint64) for i in range(4)]
    return ((u[0] & np.uint64(0x3FF)) << np.uint64(54)) | ((u[1] & np.uint64(0x3FFFF)) << np.uint64(36)) | \
        ((u[2] & np.uint64(0x3FFFF)) << np.uint64(18)) | (u[3] & np.uint64(0x3FFFF))


def mix(k):
    """The table's 64-bit hash mixer."""
    k = np.asarray(k, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xFF51AFD7ED558CCD)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xC4CEB9FE1A85EC53)
        k ^= k >> np.uint64(33)
    return k


def home_slot(c, cap):
    """Slot where the probe of each row starts in a table of `cap` slots."""
    return (mix(pack(c)) & np.uint64(cap - 1)).astype(np.int64)
