"""Edge cases of the kernels at the two ends of the step - input stage (csrc/input.hip), semantic / panoptic ensembling and
keep_mask / sine_pe (csrc/rows.hip), panoptic post-processing (csrc/panop.hip) - each a function of (be, dev): `be` is the C
oracle on the CPU (tests/test_stage_edges_cpu.py) or libpascohip.so on the GPU (tests/test_hip_stage_edges.py).  Every result
is held to tests/stage_ref.py: integers, flags and moved or selected floats bit for bit, computed floats within
K 2^-24 scale.  The raw entry points (be.fn[...]) are called where the Python wrapper would hide an argument."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pasco_amd.me.backend import SemEnsDesc, _ptr
from tests import stage_ref as ref
from tests.coords_edge_cases import same

I32, F32, U8, I64 = torch.int32, torch.float32, torch.uint8, torch.int64
_vp = C.c_void_p
FILL = 0x5A5A5A5A

# row counts around the sweep of each launch formula (ref.sweeps), and the widths around the 64-lane wave
ENS_U = (1, 3, 4, 5, 65535, 65536, 65537, 131073)
ARGMAX_N = (1, 3, 4, 5, 16383, 16384, 16385, 32769)
BOUNDS_N = (0, 1, 65535, 65536, 65537, 131073)
CELLS_V = (1, 3, 4, 5)
WIDTHS = (1, 63, 64, 65, 127, 128)
PANOP_Q = (1, 5, 64, 65, 127, 128)
for _kernel, _sizes in (("ens", ENS_U), ("argmax", ARGMAX_N), ("bounds", BOUNDS_N), ("cells", CELLS_V)):
    assert {ref.sweeps(_kernel, s) for s in _sizes if s > 0} == {"under", "exact", "over"}, (_kernel, _sizes)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def fbits(values):
    return torch.tensor(values, dtype=I32).view(F32)


def filled(shape, dtype, dev):
    """A buffer of a recognisable pattern: what a call must write is compared, what it must not is still the pattern."""
    n = int(np.prod(shape))
    size = {I32: 4, F32: 4, U8: 1}[dtype]
    raw = torch.full(((n * size + 3) // 4 + 1,), FILL, dtype=I32, device=dev)
    return raw.view(U8)[: n * size].view(dtype).view(*shape) if n else torch.empty(shape, dtype=dtype, device=dev)


# ---- sem_ensemble ------------------------------------------------------------------------------------------------------------
def run_sem(be, dev, logits, rows, c, n_sites, conf_on, offset):
    """The raw call.  offset = 1: every logits[i] and out[i] is a view one float into a larger buffer (4-byte aligned only)."""
    m = len(logits)
    d = SemEnsDesc()
    d.m, d.c, d.n_sites = m, c, n_sites
    hold, outs, confs = [], [], []
    for i in range(m + 1):
        if i < m:
            buf = torch.zeros(logits[i].numel() + 4 + offset, dtype=F32, device=dev)
            assert buf.data_ptr() % 16 == 0
            lv = buf[offset:offset + logits[i].numel()]
            lv.copy_(logits[i].reshape(-1))
            r = rows[i].to(dev)
            hold += [buf, r]
            d.logits[i], d.rows[i] = lv.data_ptr(), r.data_ptr()
        ob = filled((n_sites * c + 4 + offset,), F32, dev)
        ov = ob[offset:offset + n_sites * c]
        hold.append(ob)
        outs.append((ob, ov))
        d.out[i] = ov.data_ptr()
        cf = filled((n_sites,), F32, dev) if conf_on[i] else None
        confs.append(cf)
        d.conf[i] = _ptr(cf)
    be._check(be.fn["sem_ensemble"](C.byref(d), be.stream(dev)), "sem_ensemble")
    for ob, ov in outs:                                                   # nothing written around the rows
        rest = torch.cat([ob[:offset], ob[offset + n_sites * c:]]).cpu()
        same(rest, fbits([FILL]).repeat(rest.numel()), "sem_ensemble: written outside out[i]")
    return [ov.view(n_sites, c).cpu() for _, ov in outs], [None if cf is None else cf.cpu() for cf in confs]


def sem_ensemble(be, dev, c, m, n_sites):
    """Softmax rows, their mean and the row maxima against fp64; the one-hot of class 0 where a subnet (or every subnet) is
    absent, the last row of a subnet, a subnet of one row, two equal maxima, logits over +-80; conf[i] = NULL for some and
    for all i; the 4-byte-aligned twin call (the scalar kernel when c = 20) bit-equal to the aligned one."""
    g = gen(1000 * c + 10 * m + n_sites)
    rec = ref.Rec(f"sem_ensemble-c{c}-m{m}-n{n_sites}")
    n_i = [1] + [int(torch.randint(5, 60, (1,), generator=g)) for _ in range(m - 1)]
    n_i = n_i[::-1] if m > 1 else [7]                                   # m > 1: the LAST subnet has one row
    logits = [torch.randn(n, c, generator=g) * 3 for n in n_i]
    logits[0][0] = torch.tensor([80.0] + [-80.0 if ch % 2 else -75.0 for ch in range(1, c)])     # p exactly 1 and 0
    if n_i[0] > 2:
        logits[0][1, 3] = logits[0][1, 7] = logits[0][1].max() + 1                                # two equal maxima
    rows = [torch.randint(-max(n // 2, 1), n, (n_sites,), generator=g).clamp(min=-1).int() for n in n_i]
    for i, n in enumerate(n_i):
        rows[i][-1] = n - 1                                              # the subnet's last row
    if n_sites > 1:
        for i in range(m):
            rows[i][0] = -1                                              # every subnet absent
        rows[0][1] = 0
    if n_sites > 3:
        rows[0][2] = min(1, n_i[0] - 1)
    exp, exp_conf = ref.sem_ensemble(logits, rows)
    t_out, t_conf = ref.sem_ensemble_torch32(logits, rows)
    all_on = [True] * (m + 1)
    outs, confs = run_sem(be, dev, logits, rows, c, n_sites, all_on, 0)
    for i in range(m + 1):
        rec.add("softmax" if i < m else "mean", outs[i], exp[i], 1.0, t_out[i])
        rec.add("conf", confs[i], exp_conf[i], 1.0, t_conf[i])
        same(confs[i], outs[i].max(dim=1).values, f"conf[{i}] is the maximum of the written row")
        if i < m:
            absent = rows[i] < 0
            one_hot = torch.zeros(c)
            one_hot[0] = 1.0
            same(outs[i][absent], one_hot.repeat(int(absent.sum()), 1), f"out[{i}] where the subnet is absent")
    hit = rows[0] == 0
    same(outs[0][hit], exp[0][hit].float(), "logits over +-80: p exactly 1 and 0")
    if n_i[0] > 2:
        two = outs[0][rows[0] == 1]
        same(two[:, 3], two[:, 7], "two equal maxima")
    if n_sites > 1:
        same(outs[m][0], outs[0][0], "mean where every subnet is absent")
        same(confs[m][:1], torch.ones(1), "confidence where every subnet is absent")
    # the twin through views one float into a larger buffer; conf = NULL for some i and for all i
    some = [i % 2 == 0 for i in range(m + 1)]
    for what, conf_on, off in (("unaligned twin", all_on, 1), ("conf NULL for some", some, 0), ("conf NULL for some, unaligned", some, 1),
                               ("conf NULL for all", [False] * (m + 1), 0)):
        o2, c2 = run_sem(be, dev, logits, rows, c, n_sites, conf_on, off)
        for i in range(m + 1):
            same(o2[i], outs[i], f"{what}: out[{i}]")
            if conf_on[i]:
                same(c2[i], confs[i], f"{what}: conf[{i}]")
    rec.done()


# ---- ens_resample / ens_merge / ens_finish ---------------------------------------------------------------------------------------
BAND = (-102.5, -100.0, -95.0, -91.0, -89.5, -88.8)          # expf(-x) overflows: the fp32 quotient is an exact 0


def ens_rows(be, dev, u, q, torch32=True):
    """The three row kernels of the panoptic ensemble at (u, q): below, at and beyond one sweep of the grid-stride loop, q
    around the wave's 64 lanes."""
    g = gen(7 * u + q)
    rec = ref.Rec(f"ens_rows-u{u}-q{q}")
    n = min(u, 4000) + 8
    n_sites = u + 11
    logits = torch.randn(n, q, generator=g) * 4
    edge = torch.tensor([0.0, 88.0, -88.0, -88.8, -95.0, -110.0, -200.0, 30.0])
    logits[0] = edge[torch.arange(q) % 8]
    logits[1] = torch.tensor(BAND)[torch.arange(q) % len(BAND)]                     # every entry in the overflow band
    logits[2] = -110.0
    rows = torch.randint(-n // 3, n, (n_sites,), generator=g).clamp(min=-1).int()
    sel = torch.randperm(n_sites, generator=g)[:u].int()
    rows[sel[:3].long()] = torch.tensor([0, 1, 2], dtype=I32)[: min(u, 3)]
    if u > 3:
        rows[sel[3].long()] = -1
    for name, rw in (("", rows), (" no voxel anywhere", torch.full_like(rows, -1))):
        out, flag = be.ens_resample(logits.to(dev), rw.to(dev), sel.to(dev))
        out, flag = out.cpu(), flag.cpu()
        rec.add("resample", out, ref.ens_resample(logits, rw, sel), 1.0, ref.ens_resample_torch32(logits, rw, sel) if torch32 else None)
        same(flag, (out != 0).any(dim=1).to(U8), "ens_resample" + name + ": flag = a written entry is non-zero")
        gone = rw[sel.long()] < 0
        assert not bool(out[gone].any()) and not bool(flag[gone].any()), "ens_resample: a site without a voxel is not a zero row"
        if not name:
            probs = out
            assert int(flag[0]) == 1
            if u >= 3:
                same(out[1], torch.zeros(q), "ens_resample: the overflow band gives exact zeros")
                assert int(flag[1]) == 0 and int(flag[2]) == 0
            low = logits[0] <= -88.8
            same(out[0][low], torch.zeros(int(low.sum())), "ens_resample: logits of -88.8 and below")
    m2 = torch.rand(u, q, generator=g)
    combos = [(i, kind) for i in (1, 2, 7) for kind in ("identity", "reversed", "random")] if u <= 64 else [(2, "random")]
    for i, kind in combos:
        perm = {"identity": torch.arange(q), "reversed": torch.arange(q - 1, -1, -1), "random": torch.randperm(q, generator=g)}[kind]
        anchor = torch.rand(u, q, generator=g) if i != 2 else probs.clone()
        got = be.ens_merge(anchor.clone().to(dev), m2.to(dev), perm.int().to(dev), i)
        same(got, ref.ens_merge(anchor, m2, perm, i), f"ens_merge i={i} {kind}")
    c = 20
    sem = torch.rand(n_sites, c, generator=g)
    sem[::3, 0] = 2.0                                                   # class 0 wins
    sem[1::7] = 0.25                                                    # every class ties with class 0: the first wins
    anchor = torch.rand(u, q, generator=g)
    anchor[::5] = 0.0
    order = torch.randperm(q, generator=g).int()
    for qk in (max(1, q // 2), q):                                      # qk = q: both columns of every lane are written
        keep = order[:qk].contiguous()
        got, flag = be.ens_finish(anchor.to(dev), keep.to(dev), sem.to(dev), sel.to(dev))
        exp, exp_flag = ref.ens_finish(anchor, keep, sem, sel)
        same(got, exp, f"ens_finish qk={qk}")
        same(flag, exp_flag, f"ens_finish qk={qk} flag")
    rec.done()


def ens_finish_edges(be, dev):
    """q = 128 with qk = 0, 1, 65, 128; c = 1, 2, 19, 20, 64; the class-0 test under exact ties with class 0, a maximum in the
    last column, and class 0 the maximum."""
    g = gen(31)
    u, q = 9, 128
    n_sites = 12
    sel = torch.randperm(n_sites, generator=g)[:u].int()
    anchor = torch.rand(u, q, generator=g)
    anchor[4] = 0.0
    for c in (1, 2, 19, 20, 64):
        sem = torch.rand(n_sites, c, generator=g) * 0.5
        for j, s in enumerate(sel.long().tolist()):
            kind = j % 4
            if kind == 0:
                sem[s] = 0.125                                           # every class ties with class 0
            elif kind == 1:
                sem[s, c - 1] = 0.75                                     # the maximum in the last column
            elif kind == 2:
                sem[s, 0] = 0.75                                         # class 0 alone
            else:
                sem[s, 0] = sem[s, c // 2] = 0.75                        # class 0 and a later class tie
        for qk in (0, 1, 65, 128):
            keep = torch.randperm(q, generator=g)[:qk].int()
            out = filled((u, max(qk, 1)), F32, dev)[:, :qk].contiguous()
            flag = filled((u,), U8, dev)
            kp = keep.to(dev) if qk else torch.zeros(1, dtype=I32, device=dev)
            a, s_, sl = anchor.to(dev), sem.to(dev), sel.to(dev)
            be._check(be.fn["ens_finish"](_ptr(a), u, q, _ptr(kp), qk, _ptr(s_), c, _ptr(sl), _ptr(out), _ptr(flag), be.stream(dev)),
                      "ens_finish")
            exp, exp_flag = ref.ens_finish(anchor, keep, sem, sel)
            same(out, exp, f"ens_finish c={c} qk={qk}")
            same(flag, exp_flag, f"ens_finish c={c} qk={qk} flag")
            if c == 1:
                assert not bool(flag.any()), "one class: class 0 always wins"


# ---- project_canonical ---------------------------------------------------------------------------------------------------------
def rigid(kind, g):
    T = torch.eye(4)
    if kind.startswith("flip"):
        T[int(kind[-1]), int(kind[-1])] = -1.0
    elif kind.startswith("rot"):
        c, s = {"0": (1.0, 0.0), "90": (0.0, 1.0), "180": (-1.0, 0.0), "270": (0.0, -1.0)}[kind[3:]]
        T[0, 0], T[0, 1], T[1, 0], T[1, 1] = c, -s, s, c
    elif kind.startswith("shift"):
        T[:3, 3] = float(kind[5:])
    elif kind == "random":
        a = torch.linalg.qr(torch.randn(3, 3, generator=g))[0]
        T[:3, :3] = a
        T[:3, 3] = torch.randn(3, generator=g) * 2
    return T


KINDS = ("identity", "flip0", "flip1", "flip2", "rot0", "rot90", "rot180", "rot270", "shift0.1", "shift-0.1", "shift0.3", "shift-0.3",
         "random")


def project_canonical(be, dev, size, full=False):
    """Exact flips and quarter turns, half-voxel translations (every site on a tie of the rounding) and a random rigid T, at
    resolution 0.2 and at 0.4 with another min_bound, bit for bit."""
    g = gen(sum(size))
    grids = ((0.2, (0.0, -25.6, -2.0)), (0.4, (-3.2, 1.6, -0.4)))
    for kind in (("random", "shift0.1") if full else KINDS):
        T = rigid(kind, g)
        for res, mb in (grids[:1] if full else grids):
            if kind.startswith("shift") and res == 0.4:
                T = T.clone()
                T[:3, 3] *= 2                                            # half a voxel of that grid
            got = be.project_canonical(T.to(dev), size, res, mb)
            same(got, ref.project_canonical(T, size, res, mb), f"project_canonical {kind} {size} res {res}")


# ---- panoptic post-processing ------------------------------------------------------------------------------------------------------
def class_probs(g, q, c1, mode):
    """Class probabilities [q, c1] on a grid of 1 / 64 with the edge rows of panop_queries."""
    qp = torch.randint(0, 17, (q, c1), generator=g).float() / 64
    top = torch.randint(0, c1, (q,), generator=g)
    if mode == "all":
        top = torch.randint(1, max(c1 - 1, 2), (q,), generator=g)
    elif mode == "none":
        top = torch.where(torch.arange(q) % 2 == 0, 0, c1 - 1)
    qp[torch.arange(q), top] = torch.randint(40, 64, (q,), generator=g).float() / 64
    if mode == "mixed" and c1 > 2:
        edge = [(1, 0.5, None), (1, 0.75, 2 if c1 > 3 else None), (0, 0.75, 1), (c1 - 1, 0.75, None), (c1 - 2, 0.75, c1 - 1),
                (1, float(np.nextafter(np.float32(0.5), np.float32(1))), None)]
        for j, (cls, v, tie) in enumerate(edge[: max(q - 1, 0)]):      # prob == thr, ties (the first wins), class 0, the dustbin
            qp[j + 1] = 0.0625
            qp[j + 1, cls] = v
            if tie is not None:
                qp[j + 1, tie] = v
    return qp


def run_queries(be, dev, qp, thr):
    q, c1 = qp.shape
    qtab, nk = filled((4, 128), I32, dev), filled((1,), I32, dev)
    x = qp.to(dev)
    be._check(be.fn["panop_queries"](_ptr(x), q, c1, float(thr), _ptr(qtab), _ptr(nk), be.stream(dev)), "panop_queries")
    return qtab.cpu(), int(nk.item())


def panop_queries(be, dev, q, c1, mode):
    """Labels, probabilities, the kept ranks and the entries at and beyond q; prob == thr is not kept; c1 = 2 keeps nothing."""
    g = gen(100 * q + c1)
    qp = class_probs(g, q, c1, mode)
    got, nk = run_queries(be, dev, qp, 0.5)
    exp, K, written = ref.panop_queries(qp, 0.5)
    assert nk == K, (nk, K)
    same(torch.where(written, got, torch.full_like(got, FILL)), torch.where(written, exp, torch.full_like(exp, FILL)), "qtab")
    if mode == "all":
        assert K == q
    if mode == "none" or c1 == 2:
        assert K == 0
    if mode == "mixed" and c1 > 3 and q >= 7:
        assert got[0, 1] == -1 and got[0, 2] >= 0 and got[2, 2] == 1 and got[0, 3] == -1 and got[0, 4] == -1 and got[0, 6] >= 0


def kept_table(g, q, kept, p_equal=None):
    """qtab of q queries of which the columns `kept` are kept; the others carry a LARGER probability (class 0 winners)."""
    qp = torch.full((q, 8), 1.0 / 64)
    p = torch.randint(36, 56, (q,), generator=g).float() / 64
    if p_equal is not None:
        p[:] = p_equal
    qp[torch.arange(q), 0] = 60.0 / 64
    for col in kept:
        qp[col, 0] = 1.0 / 64
        qp[col, 1 + col % 6] = p[col]
    qtab, K, _ = ref.panop_queries(qp, 0.5)
    assert K == len(kept)
    return qtab


def run_argmax(be, dev, masks, qtab, occ_thr, carry=None):
    n, q = masks.shape
    winner, own = filled((max(n, 1),), I32, dev), filled((max(n, 1),), U8, dev)
    conf, vunc = filled((max(n, 1),), F32, dev), filled((max(n, 1),), F32, dev)
    areas = torch.zeros((2, 128), dtype=I32, device=dev) if carry is None else carry.clone().to(dev)
    x, qt = masks.to(dev), qtab.to(dev)
    be._check(be.fn["panop_argmax"](_ptr(x), n, q, _ptr(qt), float(occ_thr), _ptr(winner), _ptr(own), _ptr(conf), _ptr(vunc), _ptr(areas),
                                    be.stream(dev)), "panop_argmax")
    return winner[:n].cpu(), own[:n].cpu(), conf[:n].cpu(), vunc[:n].cpu(), areas.cpu()


def check_argmax(rec, be, dev, masks, qtab, occ_thr, what, carry=None, torch32=True):
    winner, own, conf, vunc, areas = run_argmax(be, dev, masks, qtab, occ_thr, carry)
    e = ref.panop_argmax(masks, qtab, occ_thr)
    same(winner, e["winner"], what + " winner")
    same(own, e["own"], what + " own")
    base = torch.zeros((2, 128), dtype=torch.int64) if carry is None else carry.long()
    same(areas, (base + e["areas"]).int(), what + " areas")
    t_conf = t_vunc = None
    if torch32 and bool((qtab[0, : masks.shape[1]] >= 0).any()):
        t_conf, t_vunc = ref.panop_argmax_torch32(masks, qtab)
    rec.add("panop_conf", conf, e["conf"], e["conf_scale"], t_conf)
    rec.add("panop_vunc", vunc, e["vunc"], e["vunc_scale"], t_vunc)
    n_kept = int((qtab[0, : masks.shape[1]] >= 0).sum())
    assert bool(((winner >= 0) & (winner < n_kept)).all()) if n_kept else bool((winner == -1).all()), what + ": winner is no kept index"
    return winner, own, conf, vunc, areas


def grid_masks(g, n, q, lo=16):
    """Mask probabilities on a grid of 1 / 64 in [lo / 64, 1]: products with the grid probabilities are exact in fp32, ties are
    exact ties, and the kept sum of a row stays well away from 0."""
    return torch.randint(lo, 65, (n, q), generator=g).float() / 64


def panop_argmax(be, dev, n, q, torch32=True):
    """Winner, ownership, areas and the two ratios at (n, q): rows below, at and beyond one sweep; cross-lane and same-lane
    ties; a larger value in a column that is not kept; rows whose kept masks are all 0; masks at occ_thr and one ulp below;
    a non-zero carry in `areas` (the kernel accumulates: include/pasco_hip.h)."""
    g = gen(13 * n + q)
    rec = ref.Rec(f"panop_argmax-n{n}-q{q}")
    occ = 0.5
    kept = sorted(set(torch.nonzero(torch.rand(q, generator=g) < 0.6).flatten().tolist()) | {0, q - 1} | ({min(64, q - 1)} if q > 2 else set()))
    if q >= 5:
        kept = [k for k in kept if k != 2]                               # column 2 is never kept, and carries the largest values
    qtab = kept_table(g, q, kept, p_equal=0.625)                        # equal probabilities: the masks decide, ties are exact
    masks = grid_masks(g, n, q)
    r = torch.arange(n)
    if q >= 5:
        masks[:, 2] = 1.0
    masks[r % 6 == 1] = masks[r % 6 == 1].clamp(max=0.75)               # every kept query ties at 0.75 in some rows ...
    masks[r % 6 == 1, :: 2] = 0.75                                       # ... cross-lane, and same-lane where q > 64 (l, l + 64)
    masks[r % 6 == 2] = 0.0                                              # kept masks all 0: vunc is 0 / 0
    masks[r % 6 == 3] = masks[r % 6 == 3].clamp(max=occ)                 # the winner sits exactly on occ_thr: owned
    masks[r % 6 == 3, kept[0]] = occ
    masks[r % 6 == 4] = masks[r % 6 == 4].clamp(max=float(np.nextafter(np.float32(occ), np.float32(0))))     # one ulp below
    carry = torch.zeros((2, 128), dtype=I32)
    carry[:, : len(kept)] = torch.randint(1, 1000, (2, len(kept)), generator=g, dtype=I32)
    _, own, conf, vunc, _ = check_argmax(rec, be, dev, masks, qtab, occ, "argmax", carry, torch32)
    if n > 2:
        assert bool(torch.isnan(vunc[r % 6 == 2]).all()) and not bool(conf[r % 6 == 2].any()) and not bool(own[r % 6 == 2].any())
    if n > 4:
        assert bool(own[r % 6 == 3].all()) and not bool(own[r % 6 == 4].any())
    qtab_none = kept_table(g, q, [])
    winner, own, conf, vunc, areas = check_argmax(rec, be, dev, masks, qtab_none, occ, "argmax K = 0")
    assert bool((winner == -1).all()) and not bool(own.any()) and not bool(conf.any()) and not bool(vunc.any()) and not bool(areas.any())
    rec.done()


def panop_argmax_areas(be, dev, q):
    """Every row won by one kept index - 0, 63, 64, K - 1 - with all queries kept (K = q): the lane-private area counters."""
    g = gen(q)
    rec = ref.Rec(f"panop_argmax_areas-q{q}")
    n = 70
    qtab = kept_table(g, q, list(range(q)))
    for k in sorted({0, min(63, q - 1), min(64, q - 1), q - 1}):
        masks = grid_masks(g, n, q).clamp(max=0.5)
        masks[:, k] = 1.0
        masks[::7, k] = 0.25                                             # a few rows where k loses
        _, _, _, _, areas = check_argmax(rec, be, dev, masks, qtab, 0.5, f"areas k={k}")
        assert int(areas[0, k]) == n - len(range(0, n, 7))
    rec.done()


def run_write(be, dev, n, winner, own, conf, vunc, areas, qtab, K, thr, thing, with_seg=True):
    outs = [filled((max(n, 1),), dt, dev) for dt in (I32, I32, F32, F32, F32)]
    seg = filled((5, 128), I32, dev) if with_seg else None
    args = [t.to(dev) for t in (winner, own, conf, vunc, areas.int(), qtab)]
    nk = torch.tensor([K], dtype=I32, device=dev)
    be._check(be.fn["panop_write"](n, *[_ptr(t) for t in args], _ptr(nk), float(thr), int(thing), *[_ptr(t) for t in outs], _ptr(seg),
                                   be.stream(dev)), "panop_write")
    return [t[:n].cpu() for t in outs], None if seg is None else seg.cpu()


def check_write(be, dev, n, winner, own, conf, vunc, areas, qtab, K, thr, thing, what):
    e = ref.panop_write(winner, own, conf, vunc, areas, qtab, K, thr, thing)
    for with_seg in (True, False):
        outs, seg = run_write(be, dev, n, winner, own, conf, vunc, areas, qtab, K, thr, thing, with_seg)
        for got, name in zip(outs, ("panoptic", "semantic", "ins_unc", "vox_conf", "vox_unc")):
            same(got, e[name], f"{what} seg={with_seg} {name}")
        if with_seg:
            assert int(seg[4, 0]) == e["n_seg"], (what, int(seg[4, 0]), e["n_seg"])
            same(seg[:4, : e["n_seg"]], e["seg"][:4, : e["n_seg"]], what + " segments")
            same(seg[:4, e["n_seg"]:], torch.full((4, 128 - e["n_seg"]), FILL, dtype=I32), what + ": written beyond the segments")
    return e


def panop_write(be, dev, n):
    """The sequential walk: ma / oa on the threshold (2 / 5 against 0.4, 1 / 2 against 0.5) and one count below, oa > 0 with
    ma = 0, three stuff queries of one class merged, thing classes at bit 40 and at 63, seg = NULL, the count word, n = 0."""
    g = gen(n + 5)
    classes = [3, 40, 3, 63, 3, 7, 40, 7, 9]
    K = len(classes)
    qtab = torch.zeros((4, 128), dtype=I32)
    qtab[0] = -1
    qids = [2, 5, 6, 64, 65, 90, 100, 126, 127]
    for k, (qid, cls) in enumerate(zip(qids, classes)):
        qtab[0, qid], qtab[1, k], qtab[2, qid] = k, qid, cls
        qtab[3, qid] = int(np.float32(0.55 + k / 32).view(np.int32))
    thing = (1 << 40) | (1 << 63)
    winner = torch.randint(-1, K, (n,), generator=g).int()
    own = (torch.rand(n, generator=g) < 0.7).to(U8)
    conf, vunc = torch.rand(n, generator=g), torch.rand(n, generator=g)
    vunc[::3] = float("nan")                                             # moved as it is where the query opened a segment
    conf[1::4] = -0.0
    for thr, table in ((0.4, [(2, 5), (199, 500), (1, 2), (0, 3), (5, 5), (3, 3), (2, 5), (1999, 5000), (7, 7)]),
                       (0.5, [(1, 2), (499, 1000), (1, 2), (4, 4), (1, 2), (2, 2), (0, 0), (4, 8), (5, 9)])):
        areas = torch.zeros((2, 128), dtype=I32)
        areas[:, :K] = torch.tensor(table, dtype=I32).t()
        e = check_write(be, dev, n, winner, own, conf, vunc, areas, qtab, K, thr, thing, f"write n={n} thr={thr}")
        ids = e["seg"][0, : e["n_seg"]].tolist()
        assert ids == list(range(1, e["n_seg"] + 1)) and e["seg"][2, : e["n_seg"]].tolist().count(3) == 1
        if thr == 0.4:
            assert e["seg"][3, : e["n_seg"]].tolist() == [2, 90, 100, 127]      # 2/5 kept; 199/500, 1999/5000 and ma = 0 skipped; stuff 3 merged
    none = torch.full_like(winner, -1)                                   # nothing kept: panop_argmax answers -1 everywhere
    check_write(be, dev, n, none, own, conf, vunc, torch.zeros((2, 128), dtype=I32), qtab, 0, 0.4, thing, f"write n={n} K=0")


def panop_chain(be, dev, q, n=300):
    """queries -> argmax -> write on the library's own tables, with K = q = 128 among the shapes: the NaN of a row whose kept
    products sum to 0 never reaches vox_unc (occ_thr > 0), every output against the references."""
    g = gen(q + 77)
    rec = ref.Rec(f"panop_chain-q{q}")
    qp = class_probs(g, q, 21, "all" if q == 128 else "mixed")
    qtab, K = run_queries(be, dev, qp, 0.5)
    exp_tab, exp_K, written = ref.panop_queries(qp, 0.5)
    assert K == exp_K
    qtab = torch.where(written, qtab, torch.zeros_like(qtab))
    same(qtab, torch.where(written, exp_tab, torch.zeros_like(exp_tab)), "chain qtab")
    masks = grid_masks(g, n, q)
    masks[::4] = 0.0
    winner, own, conf, vunc, areas = check_argmax(rec, be, dev, masks, qtab, 0.3, "chain argmax")
    if K:
        assert bool(torch.isnan(vunc[::4]).all())
    thing = sum(1 << c for c in range(1, 9))
    for thr in (0.0, 0.5, 0.8):
        e = check_write(be, dev, n, winner, own, conf, vunc, areas, qtab, K, thr, thing, f"chain write thr={thr}")
        outs, _ = run_write(be, dev, n, winner, own, conf, vunc, areas, qtab, K, thr, thing)
        assert not bool(torch.isnan(outs[4]).any()), "a NaN reached vox_unc"
    rec.done()


# ---- input stage ---------------------------------------------------------------------------------------------------------------
def h3(vals):
    return (C.c_int32 * 3)(*[int(v) for v in vals])


def points_bounds(be, dev, n):
    """Bounds over n points around the 65 536-point sweep; int64 values beyond int32 on both sides clamp; n = 0: sentinels."""
    g = gen(n + 1)
    xyz = torch.randint(-50, 60, (n, 3), generator=g, dtype=I64)
    variants = [("plain", xyz)]
    if n >= 2:
        far = xyz.clone()
        far[n // 2] = torch.tensor([2 ** 31 + 5, -2 ** 31 - 9, 2 ** 40])
        far[n - 1] = torch.tensor([-2 ** 50, 2 ** 31 - 1, -2 ** 31])
        variants.append(("beyond int32", far))
        neg = -xyz.abs() - 1
        neg[0] = torch.tensor([-1, -2 ** 31, -7])
        variants.append(("negative", neg))
        last = torch.zeros_like(xyz)
        last[n - 1] = torch.tensor([-3, 9, 4])
        variants.append(("the extremes in the last point", last))
    for name, pts in variants:
        out = filled((6,), I32, dev)
        x = pts.to(dev)
        be._check(be.fn["points_bounds"](_ptr(x) if n else None, n, _ptr(out), be.stream(dev)), "points_bounds")
        same(out, ref.points_bounds(pts), f"points_bounds n={n} {name}")


def points_mark(be, dev):
    """A point one step outside each of the six faces raises status bit 3 and leaves every flag to the inside points; boxes of
    2^31 - 1 sites are served, boxes of 2^31 refused before a launch; mask_compact_rank with n = 0."""
    g = gen(3)
    lo, dims = (-3, 2, -1), (5, 4, 3)
    inside = torch.stack([torch.randint(lo[a], lo[a] + dims[a], (40,), generator=g, dtype=I64) for a in range(3)], 1)
    outside = [None]
    for a in range(3):
        for v in (lo[a] - 1, lo[a] + dims[a]):
            p = torch.tensor([lo[0] + dims[0] - 1, lo[1], lo[2] + dims[2] - 1], dtype=I64)
            p[a] = v                                                     # its flat index would land on another site
            outside.append(p)
    for p in outside:
        pts = inside if p is None else torch.cat([inside[:20], p[None], inside[20:]])
        flags = torch.zeros(int(np.prod(dims)), dtype=U8, device=dev)
        status = torch.zeros(1, dtype=I32, device=dev)
        x = pts.to(dev)
        be._check(be.fn["points_mark"](_ptr(x), pts.shape[0], C.cast(h3(lo), _vp), C.cast(h3(dims), _vp), _ptr(flags), _ptr(status),
                                       be.stream(dev)), "points_mark")
        exp, exp_status = ref.points_mark(pts, lo, dims)
        same(flags, exp, f"points_mark flags, outside point {None if p is None else p.tolist()}")
        assert int(status.item()) == exp_status == (0 if p is None else 8)
    one = torch.zeros((1, 3), dtype=I64, device=dev)                      # site 0 of either box: 16 bytes of flags do
    for dims_big, ok in (((2 ** 31 - 1, 1, 1), True), ((2 ** 30, 2, 1), False), ((2048, 1024, 1024), False), ((2 ** 31 - 1, 2 ** 31 - 1, 4), False)):
        flags = torch.zeros(16, dtype=U8, device=dev)
        rc = be.fn["points_mark"](_ptr(one), 1, C.cast(h3((0, 0, 0)), _vp), C.cast(h3(dims_big), _vp), _ptr(flags), None, be.stream(dev))
        assert (rc == 0) == ok, (dims_big, rc)
        assert flags.cpu().tolist() == [1 if ok else 0] + [0] * 15
    keep, cnt = filled((1,), I32, dev), filled((1,), I32, dev)
    ws = torch.empty(max(int(be.fn["workspace_bytes"](0)), 16), dtype=U8, device=dev)
    be._check(be.fn["mask_compact_rank"](None, 0, _ptr(keep), None, _ptr(cnt), _ptr(ws), ws.numel(), be.stream(dev)), "mask_compact_rank")
    assert int(cnt.item()) == 0
    same(keep, torch.full((1,), FILL, dtype=I32), "mask_compact_rank n = 0: keep_rows written")


def run_stage(be, dev, h, xyz, starts, lo, dims):
    """points_mark -> mask_compact_rank -> points_link -> cells_max through the raw entry points, each step checked
    -> (coords, feats, status)."""
    n, c = h.shape
    m = len(starts) - 1
    nsites = int(np.prod(dims))
    hlo, hdim = C.cast(h3(lo), _vp), C.cast(h3(dims), _vp)
    hst = (C.c_int64 * (m + 1))(*[int(s) for s in starts])
    st = be.stream(dev)
    x, hd_ = xyz.to(dev), h.to(dev)
    flags = torch.zeros(nsites, dtype=U8, device=dev)
    status = torch.zeros(1, dtype=I32, device=dev)
    be._check(be.fn["points_mark"](_ptr(x), n, hlo, hdim, _ptr(flags), _ptr(status), st), "points_mark")
    exp_flags, _ = ref.points_mark(xyz, lo, dims)
    same(flags, exp_flags, "stage flags")
    sites = filled((nsites,), I32, dev)
    rank = filled((nsites,), I32, dev)
    cnt = filled((1,), I32, dev)
    ws = torch.empty(int(be.fn["workspace_bytes"](nsites)), dtype=U8, device=dev)
    be._check(be.fn["mask_compact_rank"](_ptr(flags), nsites, _ptr(sites), _ptr(rank), _ptr(cnt), _ptr(ws), ws.numel(), st), "mask_compact_rank")
    exp_sites, exp_rank = ref.compact_rank(exp_flags)
    v = int(cnt.item())
    assert v == exp_sites.numel()
    same(sites[:v], exp_sites, "stage sites")
    same(rank, exp_rank, "stage rank_of")
    head = torch.full((max(v * m, 1),), -1, dtype=I32, device=dev)
    nxt = filled((n,), I32, dev)
    be._check(be.fn["points_link"](_ptr(x), n, C.cast(hst, _vp), m, hlo, hdim, _ptr(rank), _ptr(head), _ptr(nxt), st), "points_link")
    s = ref.sites_of(xyz, lo, dims)
    cell = np.where(s >= 0, exp_rank.numpy()[np.clip(s, 0, None)].astype(np.int64) * m + ref.subnet_of(n, starts), -1)
    exp_chains = [[] for _ in range(v * m)]
    for i in np.nonzero(cell >= 0)[0]:
        exp_chains[cell[i]].append(int(i))
    assert ref.chains(head, nxt, v * m) == exp_chains, "points_link: the chains are not the cells' points"
    assert bool((nxt.cpu()[torch.from_numpy(s < 0)] == -1).all()), "points_link: next of a point outside the box"
    out = filled((v, m * c), F32, dev)
    coords = filled((v, 4), I32, dev)
    be._check(be.fn["cells_max"](_ptr(hd_), c, _ptr(head), _ptr(nxt), v, m, _ptr(sites), hlo, hdim, _ptr(out), _ptr(coords), _ptr(status), st),
              "cells_max")
    return coords.cpu(), out.cpu(), int(status.item())


def scene(g, m, v, n_per, dims, empty=()):
    """Points of m subnets (those in `empty` have none) on v distinct sites of a box -> (xyz, starts, lo)."""
    lo = (-4, 3, -2)
    nsites = int(np.prod(dims))
    occupied = torch.randperm(nsites, generator=g)[:v]
    pts, starts = [], [0]
    for b in range(m):
        k = 0 if b in empty else n_per
        s = occupied[torch.randint(0, v, (k,), generator=g)]
        if k and b == 0:
            s[: min(v, k)] = occupied[: min(v, k)]                       # every site is occupied by some point
        pts.append(torch.stack([s // (dims[1] * dims[2]) + lo[0], s // dims[2] % dims[1] + lo[1], s % dims[2] + lo[2]], 1))
        starts.append(starts[-1] + k)
    return torch.cat(pts).long(), starts, lo


def cells(be, dev, m, c, v, empty=(), big=0):
    """Voxel max + channel concatenation: m subnets (some empty), c channels (m c / 4 below, at and beyond the 64 lanes), v rows
    around the four waves of a workgroup, a cell of `big` points, voxels held by one subnet only (zeros for the others)."""
    g = gen(1000 * m + 10 * c + v + big)
    dims = (3, 5, 4)
    first = min(set(range(m)) - set(empty))
    xyz, starts, lo = scene(g, m, v, max(2 * v, 6), dims, empty)
    n = xyz.shape[0]
    if big:                                                              # `big` more points of the last non-empty subnet in one cell
        last = max(set(range(m)) - set(empty))
        at = starts[last + 1]
        xyz = torch.cat([xyz[:at], xyz[starts[first]][None].repeat(big, 1), xyz[at:]])
        starts = [s + (big if b > last else 0) for b, s in enumerate(starts)]
        n += big
    h = torch.randn(n, c, generator=g)
    h[h == 0] = 1.0
    coords, feats, status = run_stage(be, dev, h, xyz, starts, lo, dims)
    e_coords, e_feats, e_status = ref.cells_max(h, xyz, starts, lo, dims)
    same(coords, e_coords, "cells_max coords")
    same(feats, e_feats, "cells_max feats")
    assert status == e_status == 0
    assert e_coords.shape[0] == v or first != 0
    for b in empty:
        assert not bool(feats[:, b * c:(b + 1) * c].any()), "an empty subnet's channels are not zero"


def special_scene(order_seed):
    """Two subnets on six sites; subnet 0's cells hold: +0.0 and -0.0 with negatives (zero maximum, both signs), NaN first / in
    the middle / last in point order, -inf only, -0.0 only (with negatives).  The points of each subnet in a seeded order."""
    c = 4
    lo, dims = (0, 0, 0), (6, 1, 1)
    nan = float("nan")
    cells_ = [[-1.0, 0.0, -0.0, -2.0, -0.0], [nan, 1.0, 2.0, -1.0], [1.0, nan, 5.0, 0.5], [3.0, -3.0, 0.25, nan], [float("-inf")] * 3,
              [-0.0, -1.5, -0.0]]
    xs, hs = [], []
    for site, vals in enumerate(cells_):
        for j, val in enumerate(vals):
            xs.append([site, 0, 0])
            hs.append([val, -val if val == val else 1.0, vals[(j + 1) % len(vals)], -7.0 if site != 4 else float("-inf")])
    x0, h0 = torch.tensor(xs, dtype=I64), torch.tensor(hs, dtype=F32)
    g = gen(9)
    x1 = torch.tensor([[s, 0, 0] for s in (0, 0, 2, 5, 5, 5)], dtype=I64)
    h1 = torch.randn(6, c, generator=g)
    h1[3:] = torch.tensor([[-0.0] * c, [0.0, -0.0, -0.0, -1.0], [-0.0, -0.0, 0.0, -0.0]])
    pg = gen(order_seed)
    p0, p1 = torch.randperm(x0.shape[0], generator=pg), torch.randperm(6, generator=pg)
    return torch.cat([h0[p0], h1[p1]]), torch.cat([x0[p0], x1[p1]]), [0, x0.shape[0], x0.shape[0] + 6], lo, dims


def cells_order(be, dev):
    """The same points in two orders within each subnet, each order run twice: the rows and the status word are bit-equal all
    four times and equal to the maximum by value - NaN propagates as 0x7FC00000, a zero maximum is +0.0 when both signs
    occur, -inf alone stays, a cell of -0.0 and negatives is -0.0."""
    runs = []
    for seed in (1, 1, 2, 2):
        h, xyz, starts, lo, dims = special_scene(seed)
        coords, feats, status = run_stage(be, dev, h, xyz, starts, lo, dims)
        e_coords, e_feats, e_status = ref.cells_max(h, xyz, starts, lo, dims)
        same(coords, e_coords, f"order {seed} coords")
        same(feats, e_feats, f"order {seed} feats")
        assert status == e_status
        runs.append((feats, status))
    for feats, status in runs[1:]:
        same(feats, runs[0][0], "cells_max depends on the order of the points")
        assert status == runs[0][1]
    bits = runs[0][0].view(I32)
    assert bits[0, 0] == 0 and bits[1, 0] == bits[2, 0] == bits[3, 0] == ref.NAN_BITS and bits[4, 0] == fbits([-0x800000]).view(I32)[0]
    assert bits[5, 0] == -0x80000000 and runs[0][1] == 0


def cells_zero_rows(be, dev):
    """A merged row that compares equal to zero in every channel raises status bit 3: an all-(+0.0) row, and a row of only
    -0.0 (written as -0.0); a NaN alone does not make a row zero."""
    lo, dims = (0, 0, 0), (3, 1, 1)
    xyz = torch.tensor([[0, 0, 0], [1, 0, 0], [1, 0, 0], [2, 0, 0]], dtype=I64)
    for what, row1, flagged in (("+0.0", [0.0] * 4, True), ("-0.0", [-0.0] * 4, True), ("NaN", [0.0, float("nan"), 0.0, 0.0], False),
                                ("denormal", [0.0, 1e-45, 0.0, 0.0], False)):
        h = torch.tensor([[1.0, 0.0, 0.0, 0.0], row1, row1, [0.0, 0.0, 0.0, -1.0]], dtype=F32)
        coords, feats, status = run_stage(be, dev, h, xyz, [0, 2, 4], lo, dims)
        e_coords, e_feats, e_status = ref.cells_max(h, xyz, [0, 2, 4], lo, dims)
        same(feats, e_feats, f"zero row {what}")
        same(coords, e_coords, f"zero row {what} coords")
        assert status == e_status == (8 if flagged else 0), (what, status, e_status)


# ---- keep_mask and sine_pe ---------------------------------------------------------------------------------------------------------
def keep_mask(be, dev):
    """n_src = 0 with and without a box, n_src = 8 of both kinds, and only the last row of a last partial wave kept with
    fallback_rows > n: the fallback does not fire."""
    g = gen(17)
    n = 64 * 5 + 37
    coords = torch.cat([torch.zeros(n, 1, dtype=I32), torch.randint(-9, 10, (n, 3), generator=g, dtype=I32)], 1)
    lo, hi = torch.tensor([-4, -5, -3], dtype=I32), torch.tensor([5, 4, 6], dtype=I32)
    last = torch.zeros(n, dtype=U8)
    last[-1] = 1
    table = [("no source, a box", [], 0, True, 0), ("no source, no box", [], 0, False, 0),
             ("8 byte sources", [(torch.rand(n, generator=g) < 0.1).to(U8) * 7 for _ in range(8)], 0, True, 0),
             ("8 row sources", [torch.randint(-9, 2, (n,), generator=g).clamp(min=-1).int() for _ in range(8)], 1, False, 1000),
             ("last row only, fallback > n", [torch.zeros(n, dtype=U8), last], 0, False, n + 100),
             ("last row only, fallback > n, a box", [last], 0, True, n + 100),
             ("nothing kept, fallback", [torch.zeros(n, dtype=U8)], 0, True, 100)]
    for what, srcs, kind, box, fb in table:
        dsrc = [s.to(dev) for s in srcs]
        ptrs = (_vp * 8)(*[s.data_ptr() for s in dsrc])
        out, any_word = filled((n,), U8, dev), filled((1,), I32, dev)
        cd, lod, hid = coords.to(dev), lo.to(dev), hi.to(dev)
        be._check(be.fn["keep_mask"](C.cast(ptrs, _vp), len(srcs), kind, _ptr(cd) if box else None, n, _ptr(lod) if box else None,
                                     _ptr(hid) if box else None, fb, _ptr(out), _ptr(any_word), be.stream(dev)), "keep_mask")
        exp = ref.keep_mask(srcs, kind, coords, lo if box else None, hi if box else None, fb, n)
        same(out, exp, "keep_mask " + what)
        if what.startswith("last row only"):
            assert int(exp[: n - 1].sum()) == 0


def sine_pe(be, dev, f):
    """Coordinate 0, negative coordinates and the seam of the table (tab_lo - 1, tab_lo, tab_lo + tab_n - 1, tab_lo + tab_n):
    table and evaluation bit-equal there, the values against fp64 sin / cos of the fp32-formed argument."""
    import math
    rec = ref.Rec(f"sine_pe-f{f}")
    dim_t = (10000.0 ** (2 * (torch.arange(f) // 2).float() / f)).contiguous()
    scale = 2 * math.pi
    tab_lo, tab_n = -2, 40
    vals = [0, -1, -2, -3, -40, 1, 5, 31, 32, tab_lo - 1, tab_lo, tab_lo + tab_n - 1, tab_lo + tab_n, 255, 1000, -1000]
    table = be.sine_pe_table(dim_t.to(dev), scale, tab_lo, tab_lo + tab_n)
    for cstride, coff in ((3, 0), (4, 1)):
        v = torch.tensor(vals, dtype=I32)
        coords = torch.full((len(vals), cstride), 12345, dtype=I32)
        coords[:, coff], coords[:, coff + 1], coords[:, coff + 2] = v, v.flip(0), v.roll(3)
        plain = be.sine_pe(coords.to(dev), dim_t.to(dev), scale, coff=coff)
        looked = be.sine_pe(coords.to(dev), dim_t.to(dev), scale, coff=coff, table=table, tab_lo=tab_lo)
        same(looked, plain.cpu(), f"sine_pe cstride={cstride}: the table and the evaluation differ")
        rec.add("sine_pe", plain, ref.sine_pe(coords, cstride, coff, dim_t, scale), 1.0, ref.sine_pe_torch32(coords, cstride, coff, dim_t, scale))
    rec.done()


# ---- the S10 size ----------------------------------------------------------------------------------------------------------------
def full_size(be, dev):
    """210 542 rows of q = 100 (the voxel count of the benchmark scene's finest level): the row kernels and the competition."""
    ens_rows(be, dev, 210542, 100, torch32=False)
    panop_argmax(be, dev, 210542, 100, torch32=False)


def _case(fn, **kw):
    f = functools.partial(fn, **kw)
    return pytest.param(f, id="-".join([fn.__name__] + [f"{k}{v}" for k, v in kw.items()]))


CASES = ([_case(sem_ensemble, c=c, m=m, n_sites=n) for c, m, n in ((20, 1, 1), (20, 3, 255), (20, 8, 256), (20, 3, 257), (19, 1, 257),
                                                                  (19, 3, 1), (19, 8, 255), (19, 3, 256))]
         + [_case(ens_rows, u=u, q=5) for u in ENS_U] + [_case(ens_rows, u=7, q=q) for q in WIDTHS]
         + [_case(ens_rows, u=65537, q=128), _case(ens_finish_edges)]
         + [_case(project_canonical, size=s) for s in ((1, 1, 1), (1, 7, 3), (5, 1, 9), (16, 16, 1), (19, 27, 1))]
         + [_case(project_canonical, size=(256, 256, 32), full=True)]
         + [_case(panop_queries, q=q, c1=c1, mode=mode) for q in PANOP_Q for c1, mode in ((21, "mixed"), (64, "all"), (3, "none"), (2, "mixed"))]
         + [_case(panop_argmax, n=n, q=8) for n in ARGMAX_N] + [_case(panop_argmax, n=70, q=q) for q in PANOP_Q]
         + [_case(panop_argmax, n=16385, q=128)] + [_case(panop_argmax_areas, q=q) for q in (5, 64, 65, 128)]
         + [_case(panop_write, n=n) for n in (0, 255, 256, 257)] + [_case(panop_chain, q=q) for q in (1, 65, 128)]
         + [_case(points_bounds, n=n) for n in BOUNDS_N] + [_case(points_mark)]
         + [_case(cells, m=m, c=c, v=v) for m, c, v in ((1, 4, 1), (3, 8, 3), (8, 60, 4), (8, 64, 5), (1, 64, 5), (3, 60, 4), (8, 32, 3))]
         + [_case(cells, m=3, c=8, v=5, empty=e) for e in ((0,), (1,), (2,))] + [_case(cells, m=8, c=4, v=4, empty=(0, 3, 4, 7))]
         + [_case(cells, m=3, c=8, v=5, big=5000), _case(cells_order), _case(cells_zero_rows), _case(keep_mask)]
         + [_case(sine_pe, f=f) for f in (2, 128)])
assert (19 * 27 * 1) % 256 == 1
