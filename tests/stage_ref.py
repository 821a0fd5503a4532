"""Independent references of the kernels at the two ends of the step (include/pasco_hip.h): the input stage (points_bounds,
points_mark, mask_compact_rank, points_link, cells_max), semantic and panoptic ensembling (sem_ensemble, ens_resample,
ens_merge, ens_finish, project_canonical), panoptic post-processing (panop_queries, panop_argmax, panop_write), keep_mask
and sine_pe.  Written from the definition of each operation in the reference model's Python (ensembler, panoptic_inference,
the cylinder-feature scatter_max and the augmenter's merge, the canonical transform) - not from the kernels, not from
oracle/pasco_oracle.c, and without calling either.

Computed floats (softmax rows, their mean and maxima, the sigmoid, the two panoptic ratios, sin / cos) are formed in fp64 and
held to  |got - exp| <= K * 2^-24 * scale  (scale = the magnitude the value was formed at).  Decisions and bit-defined results
are restated in the arithmetic the header defines: numpy float32, one rounded operation at a time (numpy never contracts a
product into a sum), and integers."""
import numpy as np
import torch

U24 = 2.0 ** -24
# Twice the worst |got - exp| / (2^-24 scale) of the plain fp32 torch formulation on the CPU over the whole case table
# (measured 3.104, in the softmax rows of sem_ensemble; tests/test_stage_edges_cpu.py::test_torch_formulation_fits prints the
# figure of every kernel).
K = 6.208

NAN_BITS = 0x7FC00000
F32 = np.float32


def f32(t):
    return np.ascontiguousarray(t.detach().cpu().numpy(), dtype=F32)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32))


def ti32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))


# ---- the float bound -------------------------------------------------------------------------------------------------------------
def units(got, exp, scale=1.0):
    """max |got - exp| / (2^-24 scale) over the elements; inf when got is not finite where exp is, or not NaN where exp is."""
    got = got.detach().cpu().double()
    exp = exp.detach().cpu().double()
    assert got.shape == exp.shape, (tuple(got.shape), tuple(exp.shape))
    if got.numel() == 0:
        return 0.0
    scale = torch.as_tensor(scale, dtype=torch.float64).expand_as(exp)
    nan_e = torch.isnan(exp)
    diff = (got - exp).abs()
    r = torch.where(diff == 0, torch.zeros_like(diff), diff / (U24 * scale))
    r = torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))
    r = torch.where(nan_e, torch.where(torch.isnan(got), torch.zeros_like(r), torch.full_like(r, float("inf"))), r)
    return float(r.max())


TORCH_WORST = {}      # kernel -> worst units of the plain fp32 torch formulation (what K is twice of)


class Rec:
    """Collects the worst units per kernel of one case, prints `STAGE_RATIO <case> <kernel> <worst / K>` and asserts <= 1."""

    def __init__(self, case):
        self.case, self.worst = case, {}

    def add(self, kernel, got, exp, scale=1.0, torch32=None):
        self.worst[kernel] = max(self.worst.get(kernel, 0.0), units(got, exp, scale))
        if torch32 is not None:
            TORCH_WORST[kernel] = max(TORCH_WORST.get(kernel, 0.0), units(torch32, exp, scale))

    def done(self):
        for kernel, x in sorted(self.worst.items()):
            print(f"STAGE_RATIO {self.case} {kernel} {x / K:.4f}")
        bad = {k: x / K for k, x in self.worst.items() if not x <= K}
        assert not bad, (self.case, bad)


# ---- semantic ensembling (Ensembler.ensemble_sem_compl + the confidence maps) -------------------------------------------------------
def sem_ensemble(logits, rows):
    """-> (outs: m + 1 fp64 [n_sites, c], confs: m + 1 fp64 [n_sites]): softmax of the sampled row, or the one-hot of class 0
    where nothing lands; then the mean over the subnets; the row maxima."""
    outs = []
    for x, r in zip(logits, rows):
        r = r.cpu().long()
        p = torch.softmax(x.cpu().double(), dim=1)[r.clamp(min=0)]
        one_hot = torch.zeros(x.shape[1], dtype=torch.float64)
        one_hot[0] = 1.0
        outs.append(torch.where((r < 0)[:, None], one_hot[None], p))
    outs.append(torch.stack(outs).mean(0))
    return outs, [o.max(dim=1).values for o in outs]


def sem_ensemble_torch32(logits, rows):
    outs = []
    for x, r in zip(logits, rows):
        r = r.cpu().long()
        p = torch.softmax(x.cpu().float(), dim=1)[r.clamp(min=0)]
        p = p.clone()
        p[r < 0] = 0.0
        p[r < 0, 0] = 1.0
        outs.append(p)
    outs.append(torch.stack(outs).mean(0))
    return outs, [o.max(dim=1).values for o in outs]


# ---- panoptic ensembling rows ------------------------------------------------------------------------------------------------------
def ens_resample(logits, rows, sel):
    """sigmoid in fp64 of the voxel row every union site samples (zeros where it samples none) -> fp64 [U, q]."""
    r = rows.cpu().long()[sel.cpu().long()]
    out = torch.sigmoid(logits.cpu().double())[r.clamp(min=0)] if logits.shape[0] else torch.zeros(r.shape[0], logits.shape[1],
                                                                                                  dtype=torch.float64)
    return torch.where((r < 0)[:, None], torch.zeros_like(out), out)


def ens_resample_torch32(logits, rows, sel):
    r = rows.cpu().long()[sel.cpu().long()]
    out = torch.sigmoid(logits.cpu().float())[r.clamp(min=0)]
    return torch.where((r < 0)[:, None], torch.zeros_like(out), out)


def ens_merge(anchor, m, perm, i):
    """(anchor * i + m[:, perm]) / (i + 1): three rounded fp32 operations."""
    a, b = f32(anchor), f32(m)[:, perm.cpu().numpy().astype(np.int64)]
    fi = F32(i)
    den = F32(fi + F32(1))
    t = (a * fi).astype(F32)
    w = (t + b).astype(F32)
    return t32((w / den).astype(F32))


def ens_finish(anchor, keep, sem, sel):
    """anchor's kept columns times 0 where class 0 is the first maximum of the site's semantic row, times 1 elsewhere;
    flag = the written row has a non-zero entry."""
    s = f32(sem)[sel.cpu().numpy().astype(np.int64)]
    nz = (np.argmax(s, axis=1) != 0).astype(F32)                       # np.argmax: first maximum
    out = (f32(anchor)[:, keep.cpu().numpy().astype(np.int64)] * nz[:, None]).astype(F32)
    return t32(out), torch.from_numpy((out != 0).any(axis=1).astype(np.uint8))


def project_canonical(T, size, resolution, min_bound):
    """Voxel index of T applied to every site's centre: centre = site * res + res / 2 + min_bound in float64, cast to fp32;
    ((T0 x + T1 y) + T2 z) + T3 in fp32; (v - min_bound - res / 2) / res in fp32; round half to even."""
    X, Y, Z = size
    T = f32(T)
    mb = np.asarray(min_bound, dtype=F32)
    res = float(resolution)
    g = np.stack(np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    p = ((g * res + res / 2) + mb.astype(np.float64)[None]).astype(F32)
    resf, halff = F32(res), F32(res / 2)
    out = np.zeros((g.shape[0], 4), dtype=np.int32)
    for r in range(3):
        t0 = (T[r, 0] * p[:, 0]).astype(F32)
        t1 = (T[r, 1] * p[:, 1]).astype(F32)
        v = (t0 + t1).astype(F32)
        t2 = (T[r, 2] * p[:, 2]).astype(F32)
        v = (v + t2).astype(F32)
        v = (v + T[r, 3]).astype(F32)
        v = (v - mb[r]).astype(F32)
        v = (v - halff).astype(F32)
        v = (v / resf).astype(F32)
        out[:, 1 + r] = np.rint(v).astype(np.int32)
    return torch.from_numpy(out)


# ---- panoptic post-processing (panoptic_inference) ------------------------------------------------------------------------------------
QMAX = 128


def panop_queries(qp, thr):
    """-> (qtab int32 [4, 128], K, written bool [4, 128]): label = first maximum of the fp32 row, kept = label not 0, not the
    dustbin, probability > thr.  Rows 0, 2, 3 hold -1 / 0 / 0.0 at and beyond q; row 1 is written for the K kept only."""
    x = f32(qp)
    q, c1 = x.shape
    label = np.argmax(x, axis=1)
    prob = x[np.arange(q), label]
    keep = (label != 0) & (label != c1 - 1) & (prob > F32(thr))
    qtab = np.zeros((4, QMAX), dtype=np.int32)
    qtab[0] = -1
    qtab[0, :q] = np.where(keep, np.cumsum(keep) - 1, -1)
    K = int(keep.sum())
    qtab[1, :K] = np.nonzero(keep)[0]
    qtab[2, :q] = label
    qtab[3, :q] = prob.view(np.int32)
    written = np.ones((4, QMAX), dtype=bool)
    written[1, K:] = False
    return torch.from_numpy(qtab), K, torch.from_numpy(written)


def panop_argmax(masks, qtab, occ_thr):
    """-> dict(winner int32 [n], own uint8 [n], areas int64 [2, 128] (the counts to ADD), conf / vunc fp64 [n] with their
    scales): the winner is the first maximum of the fp32 products p * m over the kept queries."""
    qt = qtab.cpu().numpy()
    m_all = f32(masks)
    n, q = m_all.shape
    kq = np.nonzero(qt[0, :q] >= 0)[0]
    K = kq.size
    areas = np.zeros((2, QMAX), dtype=np.int64)
    if K == 0:
        z = torch.zeros(n, dtype=torch.float64)
        return dict(winner=torch.full((n,), -1, dtype=torch.int32), own=torch.zeros(n, dtype=torch.uint8), areas=torch.from_numpy(areas),
                    conf=z, vunc=z.clone(), conf_scale=torch.ones(n, dtype=torch.float64), vunc_scale=torch.ones(n, dtype=torch.float64))
    p = qt[3, kq].view(F32)
    m = m_all[:, kq]
    v = (m * p[None]).astype(F32)
    w = np.argmax(v, axis=1)
    bm = m[np.arange(n), w]
    occ = F32(occ_thr)
    own = bm >= occ
    areas[0, :K] = np.bincount(w[own], minlength=K)
    areas[1, :K] = (m >= occ).sum(axis=0)
    m64, p64 = m.astype(np.float64), p.astype(np.float64)
    sm = m64.sum(axis=1) + float(F32(1e-8))
    v64 = m64 * p64[None]
    sc = v64.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        vunc = v64.max(axis=1) / sc                                      # 0 / 0 = NaN where every kept product is 0
    return dict(winner=ti32(w), own=torch.from_numpy(own.astype(np.uint8)), areas=torch.from_numpy(areas),
                conf=torch.from_numpy(bm.astype(np.float64) / sm), vunc=torch.from_numpy(vunc), conf_scale=torch.from_numpy(sm),
                vunc_scale=torch.from_numpy(np.where(sc > 0, sc, 1.0)))


def panop_argmax_torch32(masks, qtab):
    """conf and vunc the way _panoptic_inference_torch forms them, fp32 on the CPU."""
    qt = qtab.cpu()
    q = masks.shape[1]
    keep = qt[0, :q] >= 0
    m = masks.cpu().float()[:, keep]
    p = qt[3, :q].view(torch.float32)[keep]
    combined = p.view(1, -1) * m
    w = combined.argmax(dim=1)
    norm = m / (m.sum(1, keepdim=True) + 1e-8)
    return norm.gather(1, w[:, None]).squeeze(1), (combined / combined.sum(1, keepdim=True)).max(1)[0]


def panop_write(winner, own, conf, vunc, areas, qtab, K, overlap_thr, thing_mask):
    """The sequential walk over the kept queries and the per-voxel writes -> dict(panoptic, semantic int32 [n], ins_unc,
    vox_conf, vox_unc fp32 [n] (moved bits), seg int32 [5, 128], n_seg)."""
    qt, ar = qtab.cpu().numpy(), areas.cpu().numpy()
    seg_of, full, cls_of, prob_of = np.zeros(QMAX, np.int32), np.zeros(QMAX, bool), np.zeros(QMAX, np.int32), np.zeros(QMAX, np.int32)
    seg = np.zeros((5, QMAX), dtype=np.int32)
    stuff, current = {}, 0
    for k in range(K):
        qid = int(qt[1, k])
        cls = int(qt[2, qid])
        cls_of[k], prob_of[k] = cls, qt[3, qid]
        ma, oa = int(ar[0, k]), int(ar[1, k])
        if not (ma > 0 and oa > 0) or ma / oa < float(overlap_thr):
            continue
        isthing = bool((int(thing_mask) >> cls) & 1)
        if not isthing:
            if cls in stuff:
                seg_of[k] = stuff[cls]
                continue
            stuff[cls] = current + 1
        current += 1
        seg_of[k], full[k] = current, True
        seg[:4, current - 1] = (current, int(isthing), cls, qid)
    seg[4, 0] = current
    w = winner.cpu().numpy().astype(np.int64)
    mine = (own.cpu().numpy() != 0) & (w >= 0)
    wk = np.where(mine, w, 0)
    hit, fl = mine & (seg_of[wk] != 0), mine & full[wk]
    zero = np.zeros(w.shape, np.int32)
    bits = lambda t: t.detach().cpu().contiguous().view(torch.int32).numpy()
    fbits = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).view(torch.float32)
    return dict(panoptic=ti32(np.where(hit, seg_of[wk], zero)), semantic=ti32(np.where(fl, cls_of[wk], zero)),
                ins_unc=fbits(np.where(fl, prob_of[wk], zero)), vox_conf=fbits(np.where(fl, bits(conf), zero)),
                vox_unc=fbits(np.where(fl, bits(vunc), zero)), seg=torch.from_numpy(seg), n_seg=current)


# ---- input stage ---------------------------------------------------------------------------------------------------------------
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def points_bounds(xyz):
    """min and max per axis of the coordinates clamped to int32; the sentinels (INT_MAX x 3, INT_MIN x 3) for no point."""
    a = np.clip(xyz.cpu().numpy().astype(np.int64).reshape(-1, 3), I32_MIN, I32_MAX)
    if a.shape[0] == 0:
        return ti32([I32_MAX] * 3 + [I32_MIN] * 3)
    return ti32(np.concatenate([a.min(0), a.max(0)]))


def sites_of(xyz, lo, dims):
    """Site id ((x - lo) dimy + (y - lo)) dimz + (z - lo) of every point, -1 outside the box."""
    a = xyz.cpu().numpy().astype(np.int64).reshape(-1, 3) - np.asarray(lo, np.int64)[None]
    d = np.asarray(dims, np.int64)
    inside = ((a >= 0) & (a < d[None])).all(axis=1)
    return np.where(inside, (a[:, 0] * d[1] + a[:, 1]) * d[2] + a[:, 2], -1)


def points_mark(xyz, lo, dims):
    """-> (flags uint8 [sites], status): 1 at the site of every point inside the box; bit 3 when a point lies outside."""
    s = sites_of(xyz, lo, dims)
    flags = np.zeros(int(np.prod(dims)), dtype=np.uint8)
    flags[s[s >= 0]] = 1
    return torch.from_numpy(flags), 8 if (s < 0).any() else 0


def compact_rank(mask):
    m = mask.cpu().numpy() != 0
    keep = np.nonzero(m)[0]
    rank = np.where(m, np.cumsum(m) - 1, -1)
    return ti32(keep), ti32(rank)


def subnet_of(n, starts):
    """Subnet of every point: the points of subnet b are starts[b] .. starts[b + 1] - 1 (empty subnets have equal starts)."""
    b = np.zeros(n, dtype=np.int64)
    for s in list(starts)[1:-1]:
        b += np.arange(n) >= int(s)
    return b


def cells_max(h, xyz, starts, lo, dims):
    """-> (coords int32 [v, 4], feats fp32 [v, m c], status): the merged rows are the occupied sites in ascending site order;
    channels [b c, (b + 1) c) of a row hold subnet b's maximum BY VALUE over its points in the voxel: a NaN among them gives
    the quiet NaN 0x7FC00000, a zero maximum is +0.0 when a +0.0 is among the points and -0.0 otherwise, an empty cell is +0.0.
    Status bit 3 when some row compares equal to zero in every channel (-0.0 is zero, NaN is not)."""
    x = f32(h)
    n, c = x.shape
    m = len(starts) - 1
    s = sites_of(xyz, lo, dims)
    inside = s >= 0
    occupied = np.unique(s[inside])
    v = occupied.size
    row = np.searchsorted(occupied, np.where(inside, s, occupied[0] if v else 0))
    cell = row * m + subnet_of(n, starts)
    idx = np.nonzero(inside)[0]
    order = idx[np.argsort(cell[idx], kind="stable")]
    out = np.zeros((v * m, c), dtype=F32)
    if order.size:
        cs = cell[order]
        first = np.nonzero(np.concatenate([[True], cs[1:] != cs[:-1]]))[0]
        vals = x[order]
        with np.errstate(invalid="ignore"):
            mx = np.maximum.reduceat(vals, first, axis=0)                                   # propagates NaN
            pos0 = np.logical_or.reduceat((vals == 0) & ~np.signbit(vals), first, axis=0)
            mx = np.where(mx == 0, np.where(pos0, F32(0.0), F32(-0.0)), mx)
        mx = np.where(np.isnan(mx), np.array([NAN_BITS], np.int32).view(F32)[0], mx).astype(F32)
        out[cs[first]] = mx
    out = out.reshape(v, m * c)
    d = np.asarray(dims, np.int64)
    coords = np.stack([np.zeros(v, np.int64), occupied // (d[1] * d[2]) + lo[0], occupied // d[2] % d[1] + lo[1], occupied % d[2] + lo[2]], 1)
    with np.errstate(invalid="ignore"):
        status = 8 if v and (~(out != 0).any(axis=1)).any() else 0
    return ti32(coords), torch.from_numpy(out), status


def chains(head, nxt, cells):
    """The point sets of the chains head / next describe -> list of sorted lists, one per cell (walks at most n links)."""
    hd, nx = head.cpu().numpy(), nxt.cpu().numpy()
    out = []
    for cell in range(cells):
        pts, p = [], int(hd[cell])
        while p >= 0:
            pts.append(p)
            assert len(pts) <= nx.size, "a chain loops"
            p = int(nx[p])
        out.append(sorted(pts))
    return out


# ---- keep masks and the sine encoding ------------------------------------------------------------------------------------------------
def keep_mask(srcs, kind, coords, lo, hi, fallback_rows, n):
    k = np.zeros(n, dtype=bool) if srcs else np.ones(n, dtype=bool)
    for s in srcs:
        a = s.cpu().numpy()
        k |= (a >= 0) if kind == 1 else (a != 0)
    if fallback_rows > 0 and not k.any():
        k = np.arange(n) < fallback_rows
    if lo is not None:
        c = coords.cpu().numpy()[:, 1:4]
        k &= ((c >= lo.cpu().numpy()[None]) & (c <= hi.cpu().numpy()[None])).all(axis=1)
    return torch.from_numpy(k.astype(np.uint8))


def sine_pe(coords, cstride, coff, dim_t, scale):
    """fp64 sin / cos of the fp32-formed argument: c = float(coord); c = c / (c + 1e-6f) * scale; ang = c / dim_t[i]."""
    cs = coords.cpu().numpy().reshape(-1, cstride)[:, coff:coff + 3].astype(F32)
    dt = f32(dim_t)
    f = dt.size
    c = ((cs / (cs + F32(1e-6)).astype(F32)).astype(F32) * F32(scale)).astype(F32)        # [n, 3]
    ang = (c[:, :, None] / dt[None, None, :]).astype(F32).astype(np.float64)              # [n, 3, f]
    out = np.concatenate([np.sin(ang[:, :, 0::2]), np.cos(ang[:, :, 1::2])], axis=2)       # [n, 3, f]
    return torch.from_numpy(out.reshape(cs.shape[0], 3 * f))


def sine_pe_torch32(coords, cstride, coff, dim_t, scale):
    cs = coords.cpu().reshape(-1, cstride)[:, coff:coff + 3].float()
    c = cs / (cs + 1e-6) * scale
    ang = c[:, :, None] / dim_t.cpu().float()[None, None, :]
    return torch.cat([ang[:, :, 0::2].sin(), ang[:, :, 1::2].cos()], dim=2).reshape(cs.shape[0], -1)


# ---- launch geometry -----------------------------------------------------------------------------------------------------------
def sweeps(kernel, rows):
    """What the host launch code makes of a row count: kernel = 'ens' (ens_grid of csrc/rows.hip: four rows per workgroup, at
    most 16 384 workgroups), 'argmax' (ph_panop_argmax: four rows per workgroup, at most 4096), 'bounds' (ph_points_bounds: 256
    points per workgroup, at most 256), 'cells' (ph_cells_max: four rows per workgroup, no cap: the class is the fill of the
    one / last workgroup).

    A RESTATEMENT OF THOSE LAUNCH FORMULAS, TO BE RE-READ WHENEVER THE LAUNCH CODE CHANGES.  It serves to choose row counts and
    to assert that the case table reaches every class - never to form an expected value.
    -> 'under' (less than one full sweep / workgroup), 'exact' (exactly one), 'over' (more than one)."""
    per, cap = {"ens": (4, 16384), "argmax": (4, 4096), "bounds": (256, 256), "cells": (4, 1)}[kernel]
    full = per * cap
    return "under" if rows < full else ("exact" if rows == full else "over")
