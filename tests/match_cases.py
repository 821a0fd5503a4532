"""Cases of the matcher and mask-loss family (include/pasco_match.h), shared by tests/test_match_cpu.py (pasco_amd/grad/host.py)
and tests/test_hip_match.py (libpascohip.so).  The device decides the route: the checks move the operands there and call
`pasco_amd.grad` / `pasco_amd.grad.criterion`.

Operands are seeded randn logits [N, Q], targets bool [N, T] and an unknown flag per row by pattern.  The references
(tests/match_ref64.py) are computed once per (shape, pattern) and shared; nobody writes to them."""
import functools
import itertools

import numpy as np
import torch

from pasco_amd.grad import criterion as crit
from pasco_amd.grad import host
from pasco_amd.grad.matchlib import BIT_KNOWN, BIT_MATCHABLE, geometry
from tests import match_ref64 as mref

# (Q, T, N)
SHAPES = [
    (1, 1, 1), (1, 1, 2), (3, 2, 3),                  # the corners of the served range; an odd row tail for the two-row MFMA
    (31, 1, 65), (32, 32, 64), (33, 33, 63),          # around the 32-wide tiles: 1 / 1 / 2 query tiles, 1 / 1 / 2 target tiles
    (7, 3, 70),
    (100, 30, 257),                                   # the decoder's shape; three row ranges, the last with one row
    (128, 128, 130),                                  # both limits; two ranges
    (3, 2, 0),                                        # no rows
    # past the first trip: T in 65 .. 96 (three 32-wide target tiles) at both ends and in the middle, each with a partial last
    # range; as many ranges as there can be; ranges that have grown past their least length
    (3, 70, 300), (5, 65, 129), (100, 96, 257),
    (7, 3, 32768),
    (7, 3, 32769),
]
MULTI = (100, 30, 257)
LONG_SHAPES = SHAPES[-5:]
REPEAT_SHAPES = ((33, 33, 63), MULTI, (5, 65, 129), (7, 3, 32769))      # the two-calls-same-bits and workspace test
PATTERNS = ("partition", "sparse", "several", "all_unknown", "first_range_unknown", "scaled3", "pm80")
N_CLASSES = 20

assert geometry(257, 100, 30)["ranges"] == 3 and geometry(256, 100, 30)["ranges"] == 2, \
    "257 rows is the smallest count with three ranges"
assert MULTI[2] % geometry(MULTI[2], MULTI[0], MULTI[1])["range_rows"] != 0, "a partial last range"


# !! `launch_class` restates the dispatch of pm_pair_sums (pasco_amd/csrc/match.hip: k_pair_part<TT> on pad32(T) / 32, the rows
# !! per range and the ranges, the latter two through the binding's `geometry`).  It is used to CHOOSE shapes and to assert, at
# !! import, that SHAPES reaches the classes below - never to form an expected value: those come from tests/match_ref64.py.
MIN_RANGE, MAX_RANGES = 128, 256


def launch_class(shape):
    q, t, n = shape
    g = geometry(n, q, t)
    return dict(tt=-(-t // 32), ranges=g["ranges"], range_rows=g["range_rows"],
                partial_last=g["range_rows"] > 0 and n % g["range_rows"] != 0)


def _check_shapes():
    v = {s: launch_class(s) for s in SHAPES}
    for tt in (1, 2, 3, 4):
        assert any(x["tt"] == tt for x in v.values()), f"k_pair_part<{tt}> is not launched"
    three = [x for s, x in v.items() if x["tt"] == 3]
    assert {s[1] for s, x in v.items() if x["tt"] == 3} == {65, 70, 96}, "pad32(T) / 32 == 3 at both ends and in the middle"
    assert all(x["partial_last"] and x["ranges"] >= 2 for x in three), "each with a partial last range"
    assert any(x["ranges"] == MAX_RANGES and x["range_rows"] == MIN_RANGE and not x["partial_last"] for x in v.values()), "ranges == 256"
    assert any(x["range_rows"] > MIN_RANGE and x["partial_last"] for x in v.values()), "range_rows > 128"
    assert v[(7, 3, 32769)]["range_rows"] == 160 and v[(7, 3, 32769)]["ranges"] == 205
    assert all(x["ranges"] <= 3 and x["range_rows"] == MIN_RANGE for s, x in v.items() if s not in LONG_SHAPES and s[2] > 0)
    assert all(s in SHAPES for s in REPEAT_SHAPES) and LONG_SHAPES[1] in REPEAT_SHAPES and LONG_SHAPES[4] in REPEAT_SHAPES


_check_shapes()


def pack_words(tgt, known):
    """tgt bool [N, T], known bool [N] -> (tbits int32 [N, 4], flags uint8 [N]) with numpy, independent of the code under test."""
    n, t = tgt.shape
    w = np.zeros((n, 4), dtype=np.uint32)
    a = tgt.numpy()
    for k in range(t):
        w[:, k >> 5] |= a[:, k].astype(np.uint32) << np.uint32(k & 31)
    kn = known.numpy()
    flags = kn.astype(np.uint8) | ((kn & a.any(axis=1)).astype(np.uint8) << 1)
    return torch.from_numpy(w.view(np.int32).copy()), torch.from_numpy(flags.astype(np.uint8))


class Inputs:
    def __init__(self, shape, pattern):
        Q, T, N = shape
        self.shape, self.pattern = shape, pattern
        g = torch.Generator().manual_seed(9000 + 131 * N + 7 * Q + T + 1000 * PATTERNS.index(pattern))
        x = torch.randn(N, Q, generator=g)
        if pattern == "scaled3":
            x = x * 3
        if pattern == "pm80":
            x = torch.where(x >= 0, torch.full_like(x, 80.0), torch.full_like(x, -80.0))
        self.logits = x.contiguous()
        if pattern == "partition":
            tgt = torch.nn.functional.one_hot(torch.randint(0, T, (N,), generator=g), T).bool()
        elif pattern == "several":
            tgt = torch.rand(N, T, generator=g) < min(0.5, 3.0 / T)
            tgt[:, 0] |= ~tgt.any(dim=1)
        else:                                          # a partition with 30 % of the rows in no target
            tgt = torch.nn.functional.one_hot(torch.randint(0, T, (N,), generator=g), T).bool()
            tgt &= (torch.rand(N, generator=g) >= 0.3)[:, None]
        known = torch.ones(N, dtype=torch.bool)
        if pattern == "all_unknown":
            known[:] = False
        elif pattern == "first_range_unknown":
            known[:geometry(N, Q, T)["range_rows"]] = False
        elif pattern in ("sparse", "scaled3"):
            known = torch.rand(N, generator=g) >= 0.2
        self.tgt, self.known = tgt, known
        self.tbits, self.flags = pack_words(tgt, known)
        self.query_logits = torch.randn(Q, N_CLASSES + 1, generator=g)
        self.labels = torch.randint(0, N_CLASSES, (T,), generator=g)
        self.class_weights = torch.rand(N_CLASSES + 1, generator=g) + 0.5
        self.g_mask = torch.randn(min(Q, T), generator=g)
        self.g_dice = torch.randn(min(Q, T), generator=g)

    @functools.cached_property
    def matcher64(self):
        return mref.matcher_terms(self.logits, self.tgt, self.known, torch.float64)

    @functools.cached_property
    def matcher32(self):
        return mref.matcher_terms(self.logits, self.tgt, self.known, torch.float32)

    def cost(self, dtype):
        return mref.matcher_cost(self.logits, self.tgt, self.known, self.query_logits, self.labels, self.class_weights, dtype)

    @functools.cached_property
    def optimum(self):
        """(src, tgt) of the fp64 optimum: the pairs every route's losses are computed for."""
        return host.assign(self.cost(torch.float64))

    @functools.cached_property
    def pair_weights(self):
        return self.class_weights[self.labels[self.optimum[1]]]

    def _losses(self, dtype):
        s, t = self.optimum
        return mref.losses(self.logits, self.tgt, self.known, s, t, self.pair_weights, self.g_mask, self.g_dice, dtype)

    @functools.cached_property
    def losses64(self):
        return self._losses(torch.float64)

    @functools.cached_property
    def losses32(self):
        return self._losses(torch.float32)

    def packed(self, dev, tbits=None):
        return crit.PackedTargets((self.tbits if tbits is None else tbits).to(dev), self.flags.to(dev),
                                  torch.zeros(1, dtype=torch.int32, device=dev), self.shape[1])


@functools.lru_cache(maxsize=None)
def inputs(shape, pattern):
    return Inputs(shape, pattern)


def _label(name, shape, pattern, what):
    return f"{name} Q{shape[0]} T{shape[1]} N{shape[2]} {pattern} {what}"


def check_precision(dev, M, name, shape, pattern):
    """focal_sum / count, dice, both losses and dlogits against fp64 by the ratio rule; the exact conditions on the way."""
    import pasco_amd.grad as G
    x = inputs(shape, pattern)
    Q, T, N = shape
    worst = 0.0
    # the matcher's sums
    focal_sum, dice, stats, count = G.pair_sums(x.logits.to(dev), x.tbits.to(dev), x.flags.to(dev), BIT_MATCHABLE, T)
    f64, d64, m = x.matcher64
    f32, d32, _ = x.matcher32
    assert int(count) == m == int((x.known & x.tgt.any(dim=1)).sum())
    focal = focal_sum / max(m, 1)
    worst = max(worst, mref.ratio_check(_label(name, shape, pattern, "focal"), focal, f64, f32, M))
    worst = max(worst, mref.ratio_check(_label(name, shape, pattern, "dice"), dice, d64, d32, M))
    if pattern == "partition":
        want = x.tgt.sum(dim=0).to(stats.dtype)[None, :].expand(Q, T)
        assert torch.equal(stats[:, :, 2].cpu(), want), "tsum of a partition is an exact integer"
    # the losses of the fp64 optimum's pairs
    src, tgt = x.optimum
    logits = x.logits.clone().to(dev).requires_grad_(True)
    lm, ld = crit.mask_losses(logits, x.packed(dev), src, tgt, x.pair_weights.to(dev))
    (lm * x.g_mask.to(dev)).sum().add((ld * x.g_dice.to(dev)).sum()).backward()
    dl = logits.grad if logits.grad is not None else torch.zeros_like(logits)
    lm64, ld64, dl64 = x.losses64
    lm32, ld32, dl32 = x.losses32
    worst = max(worst, mref.ratio_check(_label(name, shape, pattern, "loss_mask"), lm, lm64, lm32, M))
    worst = max(worst, mref.ratio_check(_label(name, shape, pattern, "loss_dice"), ld, ld64, ld32, M))
    worst = max(worst, mref.ratio_check(_label(name, shape, pattern, "dlogits"), dl, dl64, dl32, M))
    unmatched = torch.ones(Q, dtype=torch.bool)
    unmatched[src] = False
    dl = dl.cpu()
    assert not bool(dl[:, unmatched].any()), "dlogits: exactly 0 in unmatched columns"
    assert not bool(dl[~x.known].any()), "dlogits: exactly 0 in unknown rows"
    assert bool(torch.isfinite(dl).all())
    print(f"PM_WORST {_label(name, shape, pattern, '')} {worst:.3f}")
    return worst


def check_assignment(dev, M, name, shape, pattern):
    """End to end: the matcher's assignment is valid and, under the fp64 cost, within 2 K e of the fp64 optimum, e = M x the
    yardstick's elementwise cost error (an elementwise cost error of e moves the total of K pairs by at most K e, for the
    optimum and for the answer: 2 K e)."""
    x = inputs(shape, pattern)
    Q, T, N = shape
    matcher = crit.HungarianMatcher()
    src, tgt = matcher.match_packed(x.logits.to(dev), x.query_logits.to(dev), x.labels.to(dev), x.class_weights.to(dev), x.packed(dev))
    K = min(Q, T)
    assert src.dtype == torch.int64 and tgt.dtype == torch.int64 and not src.is_cuda
    assert src.shape == (K,) and tgt.shape == (K,)
    assert bool((src[1:] > src[:-1]).all()), "rows ascending"
    assert len(set(tgt.tolist())) == K and 0 <= int(tgt.min()) and int(tgt.max()) < T and 0 <= int(src.min()) and int(src.max()) < Q
    C64 = x.cost(torch.float64)
    e = mref.bound_for(M, C64.numel()) * float((x.cost(torch.float32).double() - C64).abs().max())
    o_src, o_tgt = x.optimum
    gap = float(C64[src, tgt].sum() - C64[o_src, o_tgt].sum())
    print(f"PM_ASSIGN {_label(name, shape, pattern, '')} gap {gap:.3e}  bound {2 * K * e:.3e}")
    assert gap <= 2 * K * e
    return src, tgt


def check_indices_equal(dev, M, name):
    """The two seeded cases whose assignment is the same in fp32 and fp64."""
    for shape in (MULTI, (7, 3, 70)):
        src, tgt = check_assignment(dev, M, name, shape, "scaled3")
        o_src, o_tgt = inputs(shape, "scaled3").optimum
        assert torch.equal(src, o_src) and torch.equal(tgt, o_tgt), shape


def check_garbage_bits(dev, shape=(33, 33, 63)):
    """Garbage in the word bits at positions >= T changes no output bit."""
    import pasco_amd.grad as G
    x = inputs(shape, "sparse")
    Q, T, N = shape
    g = torch.Generator().manual_seed(5)
    junk = torch.randint(-2 ** 31, 2 ** 31, (N, 4), generator=g, dtype=torch.int64).to(torch.int32)
    keep = torch.zeros(4, dtype=torch.int64)
    for k in range(T):
        keep[k >> 5] |= 1 << (k & 31)
    keep = torch.where(keep >= 2 ** 31, keep - 2 ** 32, keep).to(torch.int32)
    dirty = (x.tbits & keep) | (junk & ~keep)
    assert not torch.equal(dirty, x.tbits)
    for bit in (BIT_KNOWN, BIT_MATCHABLE):
        a = G.pair_sums(x.logits.to(dev), x.tbits.to(dev), x.flags.to(dev), bit, T)
        b = G.pair_sums(x.logits.to(dev), dirty.to(dev), x.flags.to(dev), bit, T)
        for s, t_ in zip(a, b):
            assert torch.equal(s, t_)
    tq = torch.full((Q,), -1, dtype=torch.int32)
    tq[x.optimum[0]] = x.optimum[1].to(torch.int32)
    coef = torch.randn(Q, 3, generator=g)
    a = G.mask_loss_bwd(x.logits.to(dev), x.tbits.to(dev), x.flags.to(dev), tq.to(dev), coef.to(dev), T)
    b = G.mask_loss_bwd(x.logits.to(dev), dirty.to(dev), x.flags.to(dev), tq.to(dev), coef.to(dev), T)
    assert torch.equal(a, b)


# ---- pm_target_pack ----------------------------------------------------------------------------------------------------------
def pack_case(t, dims=(5, 6, 7), origin=(3, -2, 10), with_unknown=True, n_outside=0, seed=0):
    """Every voxel of the grid once (so every face), in a seeded order, then `n_outside` rows just outside each face."""
    g = torch.Generator().manual_seed(100 + seed + t)
    dx, dy, dz = dims
    masks = (torch.rand(t, dx, dy, dz, generator=g) < 0.3).to(torch.uint8) * torch.randint(1, 255, (t, dx, dy, dz), generator=g).to(torch.uint8)
    unknown = (torch.rand(dx, dy, dz, generator=g) < 0.25).to(torch.uint8) if with_unknown else None
    vox = torch.tensor(list(itertools.product(range(dx), range(dy), range(dz))), dtype=torch.int32)
    vox = vox[torch.randperm(vox.shape[0], generator=g)]
    outside = []
    for axis in range(3):
        for v in (-1, dims[axis]):
            c = [dims[0] // 2, dims[1] // 2, dims[2] // 2]
            c[axis] = v
            outside.append(c)
    outside = torch.tensor(outside[:n_outside] if n_outside else [], dtype=torch.int32).reshape(-1, 3)
    vox = torch.cat([vox[:50], outside, vox[50:]])
    coords = torch.cat([torch.full((vox.shape[0], 1), 9, dtype=torch.int32), vox + torch.tensor(origin, dtype=torch.int32)], dim=1)
    return masks, unknown, coords.contiguous(), vox


def check_target_pack(dev, t, with_unknown, n_outside):
    import pasco_amd.grad as G
    dims, origin = (5, 6, 7), (3, -2, 10)
    masks, unknown, coords, vox = pack_case(t, dims, origin, with_unknown, n_outside)
    tbits, flags, oob = G.target_pack(masks.to(dev), None if unknown is None else unknown.to(dev), coords.to(dev), origin)
    v = vox.numpy().astype(np.int64)
    inside = ((v >= 0) & (v < np.array(dims))).all(axis=1)
    vc = np.where(inside[:, None], v, 0)
    tg = (masks.numpy()[:, vc[:, 0], vc[:, 1], vc[:, 2]] != 0).T & inside[:, None]
    kn = inside & (True if unknown is None else unknown.numpy()[vc[:, 0], vc[:, 1], vc[:, 2]] == 0)
    want_bits, want_flags = pack_words(torch.from_numpy(tg), torch.from_numpy(kn))
    assert int(oob) == n_outside == int((~inside).sum())
    assert tbits.dtype == torch.int32 and flags.dtype == torch.uint8
    assert torch.equal(tbits.cpu(), want_bits), "tbits against a numpy gather"
    assert torch.equal(flags.cpu(), want_flags), "flags against a numpy gather"
    assert not bool(tbits.cpu()[~torch.from_numpy(inside)].any()) and not bool(flags.cpu()[~torch.from_numpy(inside)].any())


# ---- pm_assign ---------------------------------------------------------------------------------------------------------------
def small_cost_cases():
    """The list tools/pm_assign_check.cpp walks too: every Q, T <= 5 with seeded costs, plain, with ties (integers 0..2) and with
    equal columns."""
    out = []
    for q in range(1, 6):
        for t in range(1, 6):
            for k, kind in enumerate(("plain", "ties", "equal_columns")):
                s, vals = 17 * q + t + 1000 * k, []
                for _ in range(q * t):             # the generator of tools/pm_assign_check.cpp
                    s = (s * 6364136223846793005 + 1442695040888963407) % 2 ** 64
                    vals.append((s >> 11) / 2.0 ** 53)
                c = torch.tensor(vals, dtype=torch.float64).reshape(q, t)
                if kind == "ties":
                    c = torch.floor(c * 3)
                if kind == "equal_columns":
                    c = c[:, :1].expand(q, t).contiguous()
                out.append((q, t, kind, c))
    return out


def brute_force(c):
    q, t = c.shape
    best = None
    if q <= t:
        for cols in itertools.permutations(range(t), q):
            s = sum(float(c[i, j]) for i, j in enumerate(cols))
            best = s if best is None or s < best else best
    else:
        for rows in itertools.permutations(range(q), t):
            s = sum(float(c[i, j]) for j, i in enumerate(rows))
            best = s if best is None or s < best else best
    return best


def check_assign_against_brute_force(assign):
    for q, t, kind, c in small_cost_cases():
        row, col = assign(c)
        k = min(q, t)
        assert row.shape == (k,) and col.shape == (k,), (q, t, kind)
        assert len(set(row.tolist())) == k and len(set(col.tolist())) == k and row.tolist() == sorted(row.tolist()), (q, t, kind)
        assert 0 <= min(row.tolist()) and max(row.tolist()) < q and 0 <= min(col.tolist()) and max(col.tolist()) < t
        got = float(c[row, col].sum())
        assert abs(got - brute_force(c)) <= 1e-12, (q, t, kind, got, brute_force(c))


# ---- the recorded reference scenes (tests/golden/make_golden_match.py) ---------------------------------------------------------
GOLDEN_SCENES = ("a", "b", "c")


@functools.lru_cache(maxsize=None)
def golden(scene):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"match_{scene}.npz")) as z:
        return {k: z[k] for k in z.files}


def build_criterion(z, dev):
    weight_dict = dict(zip(z["weight_names"].tolist(), (float(v) for v in z["weight_values"])))
    cw = torch.from_numpy(z["class_weights"]).to(dev)
    return crit.SetCriterion(N_CLASSES, crit.HungarianMatcher(1, 1, 1), weight_dict, 0.1, [cw], torch.ones(N_CLASSES)).to(dev)


def check_golden(dev, M, name, scene):
    """SetCriterion on a recorded scene: the reference's keys, its matches, its values and gradients by the ratio rule (the
    yardstick is the reference's own fp32 run), the targets packed once for all levels."""
    import pasco_amd.grad as G
    import pasco_amd.me as ME
    z = golden(scene)
    L = int(z["n_levels"])
    criterion = build_criterion(z, dev)
    coords = torch.from_numpy(z["coords"]).to(dev)
    leaves, outs, main = [], [], None
    for lv in range(L):
        f = torch.from_numpy(z[f"logits{lv}"]).float().to(dev).requires_grad_(True)
        ql = torch.from_numpy(z[f"query_logits{lv}"]).to(dev).requires_grad_(True)
        if main is None:
            st = main = ME.SparseTensor(features=f, coordinates=coords)
        else:
            st = ME.SparseTensor(features=f, coordinate_map_key=main.coordinate_map_key, coordinate_manager=main.coordinate_manager)
        leaves.append((f, ql))
        outs.append({"voxel_logits": st, "query_logits": ql})
    outputs = dict(outs[0])
    if L > 1:
        outputs["aux_outputs"] = outs[1:]
    targets = [{"labels": torch.from_numpy(z["labels"]).to(dev), "masks": torch.from_numpy(z["masks"]).to(dev)}]
    unknown = torch.from_numpy(z["unknown"]).bool().to(dev)[None]
    calls, inner = [], G.target_pack
    G.target_pack = lambda *a, **k: (calls.append(1), inner(*a, **k))[1]
    try:
        marker = object()
        losses = criterion(None, outputs, targets, None, unknown, 0, marker, torch.from_numpy(z["min_c"]))
    finally:
        G.target_pack = inner
    assert len(calls) == 1, "the targets are packed once per batch element and reused by every level"
    assert sorted(losses.keys()) == z["keys"].tolist() and sorted(losses["loss_aux"].keys()) == z["aux_keys"].tolist()
    assert losses["indices"] is marker
    assert losses["ssc_ce_loss"] == 0.0 and losses["ssc_lovasz_loss"] == 0.0
    assert all(v == 0.0 for k, v in losses["loss_aux"].items() if k.startswith("ssc_"))
    assert len(criterion.matched) == L
    got = []
    for lv in range(L):
        src, tgt = criterion.matched[lv][0]
        assert torch.equal(src, torch.from_numpy(z[f"src{lv}"])) and torch.equal(tgt, torch.from_numpy(z[f"tgt{lv}"])), f"level {lv}"
        suffix = "" if lv == 0 else f"_level{lv - 1}"
        d = losses if lv == 0 else losses["loss_aux"]
        got.append(torch.stack([d["loss_ce" + suffix], d["loss_mask" + suffix], d["loss_dice" + suffix]]))
    got = torch.stack(got)
    want64 = torch.stack([torch.from_numpy(z[f"loss64_{lv}"]) for lv in range(L)])
    want32 = torch.stack([torch.from_numpy(z[f"loss32_{lv}"]) for lv in range(L)])
    worst = mref.ratio_check(f"{name} scene {scene} losses", got, want64, want32, M)
    got.sum().backward()
    for lv, (f, ql) in enumerate(leaves):
        src = torch.from_numpy(z[f"src{lv}"])
        other = torch.ones(f.shape[1], dtype=torch.bool)
        other[src] = False
        g = f.grad.cpu()
        assert not bool(g[:, other].any()), "an unmatched column has a gradient"
        worst = max(worst, mref.ratio_check(f"{name} scene {scene} level {lv} dlogits", g[:, src], torch.from_numpy(z[f"dlogits64_{lv}"]),
                                            torch.from_numpy(z[f"dlogits32_{lv}"]), M))
        worst = max(worst, mref.ratio_check(f"{name} scene {scene} level {lv} dquery", ql.grad[0], torch.from_numpy(z[f"dquery64_{lv}"]),
                                            torch.from_numpy(z[f"dquery32_{lv}"]), M))
    print(f"PM_WORST {name} scene {scene} {worst:.3f}")


def check_state_dict_and_ssc(dev):
    z = golden("a")
    criterion = build_criterion(z, dev)
    assert set(criterion.state_dict()) == {"empty_weight", "compl_labelweights"}
    assert tuple(criterion.empty_weight.shape) == (N_CLASSES + 1,) and bool((criterion.empty_weight == 1).all())
    assert "never adds" in crit.SetCriterion.__doc__
