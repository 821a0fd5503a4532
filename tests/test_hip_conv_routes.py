"""Every kernel route of `conv_fwd` x the fused epilogue x edge shapes, against fp64 (tests/conv_ref64.py).

The routes are data (ROUTES): how a route is reached (map kind, channel counts, win / grid / rowlist tables, `routing` bits) and the
`conv_last_config()` key it must produce (kernel id, bm, bn, split over the offsets or not).  Every launch asserts its key, so a
dispatch change cannot move a case onto another kernel unnoticed; the last test checks that every declared route was reached.

Per route: a base shape that runs the full product act x tail x res_act x emit, and edge shapes (row counts at the route's tile
edges, column counts at its column-tile edges, cin with cpad != cin, kc 64 / 32, isolated rows, n_in != n_out, per-channel vectors
that are not 16-byte aligned, extreme weight scales, activations just under the operand's range guard, per-axis coordinates outside
the table) that run a covering set: every (tail, emit) pair, every act and both res_act.  Each result is held element-wise to
|got - ref| <= C_ROUTE * A + rounding (conv_ref64.py) on sampled rows; emitted operands bit for bit against `split_rows` of the
fp32 result, the operand-only launch (want_out=False) bit for bit against the emitted one; the status word clean, except bit value
4 where per-axis coordinates leave the table.  The worst err / A per route is printed at the end (-s)."""
import itertools
import zlib

import pytest
import torch

from pasco_amd.me.backend import (ROUTE_WIDE_ALWAYS, ROUTE_WIDE_NEVER, ROUTE_WIN_ALWAYS, ROUTE_WIN_NEVER,
                                  StatusError)
from pasco_amd.me.core import kernel_offsets
from tests.conv_ref64 import C_ROUTE, epilogue64, gather_sum64, violations, worst_ratio

pytestmark = pytest.mark.gpu

ACTS = (0, 1, 2)
TAILS = ("none", "bn2", "residual", "axis", "residual+axis")
EMITS = ("no", "plain", "osp_relu", "osp_leaky")
SLOPE = 0.1
T_AXIS, LO_AXIS = 24, -5
N_SAMPLE = 700

# name -> (key = (kernel, bm, bn, split over the offsets), operand mode, routing bits, map kind)
ROUTES = {
    "h2_bn32":        ((2, 128, 32, False), 2, 0, "k3"),
    "h2_bn64_bm64":   ((2, 64, 64, False), 2, 0, "k3"),
    "h2_bn64_bm128":  ((2, 128, 64, False), 2, 0, "k3"),
    "dma":            ((4, 128, 128, False), 2, 0, "k1x1x3"),
    "dma_ksplit":     ((4, 128, 128, True), 2, ROUTE_WIDE_NEVER, "k3"),
    "wop2":           ((5, 128, 64, False), 2, ROUTE_WIN_ALWAYS, "k3win"),
    "win_gather64":   ((5, 128, 64, False), 2, ROUTE_WIN_NEVER, "k3win"),
    "win128":         ((5, 128, 128, False), 2, ROUTE_WIN_ALWAYS, "k3win"),
    "wide256":        ((6, 256, 256, False), 2, ROUTE_WIDE_ALWAYS, "k3"),
    "wide256_ksplit": ((6, 256, 256, True), 2, ROUTE_WIDE_ALWAYS, "k3"),
    "wide128_ksplit": ((6, 256, 128, True), 2, ROUTE_WIDE_ALWAYS, "k3"),
    "wide128_tail":   ((4, 128, 128, True), 2, 0, "k3"),        # whole rounds on k_conv_wide<2>, left-over rows k_conv_dma split
    "lin":            ((7, 32, 128, False), 2, 0, "k1"),
    "grid":           ((8, 256, 128, False), 2, 0, "grid"),
    "grid_ksplit":    ((8, 256, 128, True), 2, 0, "grid"),
    "rowlist64":      ((3, 128, 64, False), 2, 0, "rl"),
    "rowlist128":     ((3, 128, 128, False), 2, 0, "rl"),
    "mode1":          ((1, 64, 64, False), 1, 0, "k3"),
    "mode1_ksplit":   ((1, 128, 128, True), 1, 0, "k3"),
    "mode0":          ((0, 64, 64, False), 0, 0, "k3"),
}


def _c(route, n, cin, cout, full=False, **var):
    return dict(route=route, n=n, cin=cin, cout=cout, full=full, **var)


CASES = [
    # k_conv_h2, 32-wide tiles: rows at the 128-row tile edges, cout 20 (columns past cout in the one tile)
    _c("h2_bn32", 1000, 64, 32, full=True),
    _c("h2_bn32", 1, 8, 32), _c("h2_bn32", 127, 40, 20), _c("h2_bn32", 128, 72, 32, iso=True), _c("h2_bn32", 129, 200, 20),
    _c("h2_bn32", 700, 64, 32, stride2=True, misalign=True), _c("h2_bn32", 300, 32, 32, pruned=True, axis_out=True),
    # k_conv_h2, 64-wide tiles without window tables: 64-row tiles below 512 row tiles of 128, 128-row tiles from there
    _c("h2_bn64_bm64", 1000, 64, 64, full=True),
    _c("h2_bn64_bm64", 1, 256, 48), _c("h2_bn64_bm64", 63, 288, 64), _c("h2_bn64_bm64", 64, 72, 60, iso=True),
    _c("h2_bn64_bm64", 65, 40, 36, misalign=True), _c("h2_bn64_bm64", 129, 8, 64, wscale=1e-4),
    _c("h2_bn64_bm64", 900, 64, 64, stride2=True, big=True), _c("h2_bn64_bm64", 500, 32, 64, pruned=True, axis_out=True),
    _c("h2_bn64_bm128", 65409, 32, 64, full=True), _c("h2_bn64_bm128", 66000, 40, 48, iso=True, misalign=True),
    # k_conv_dma, direct (3 offsets: no split): 128-wide tiles, cout 192 = one and a half column tiles
    _c("dma", 3001, 64, 128, full=True),
    _c("dma", 1, 40, 192), _c("dma", 127, 128, 128, iso=True), _c("dma", 128, 200, 192, misalign=True),
    _c("dma", 129, 72, 128, wscale=1e3), _c("dma", 1000, 8, 192, pruned=True, big=True), _c("dma", 600, 64, 128, axis_out=True),
    # k_conv_dma split over the offsets + k_splitk_epilogue (few-row maps)
    _c("dma_ksplit", 1000, 64, 128, full=True),
    _c("dma_ksplit", 1, 256, 128), _c("dma_ksplit", 127, 288, 256), _c("dma_ksplit", 129, 40, 192, iso=True),
    _c("dma_ksplit", 3001, 128, 128, stride2=True, misalign=True), _c("dma_ksplit", 500, 72, 128, wscale=1e-4, axis_out=True),
    # the window pair, 64-wide outputs: k_conv_wop2 forced (33 <= cout <= 64: fragment-order weights), and its gather side
    _c("wop2", 1000, 64, 64, full=True),
    _c("wop2", 1, 64, 36), _c("wop2", 127, 8, 48), _c("wop2", 128, 40, 60, iso=True), _c("wop2", 129, 72, 64, misalign=True),
    _c("wop2", 700, 200, 48, pruned=True, big=True), _c("wop2", 600, 256, 64, stride2=True), _c("wop2", 300, 288, 40, axis_out=True),
    _c("wop2", 400, 64, 64, wscale=1e3),
    _c("win_gather64", 1000, 64, 64, full=True),
    _c("win_gather64", 1, 40, 60), _c("win_gather64", 129, 72, 48, iso=True, misalign=True), _c("win_gather64", 600, 256, 64, pruned=True),
    # the window pair on 128-wide tiles (formed only where no split over the offsets was chosen: >= 512 row tiles)
    _c("win128", 65409, 40, 128, full=True), _c("win128", 66000, 128, 128, iso=True, misalign=True),
    # k_conv_wide: 256 x 256 unsplit, split over the offsets on few-row maps, 256 x 128 split
    _c("wide256", 41000, 32, 256, full=True),
    _c("wide256_ksplit", 3001, 64, 256, full=True),
    _c("wide256_ksplit", 1, 256, 256), _c("wide256_ksplit", 255, 288, 256, iso=True), _c("wide256_ksplit", 257, 40, 256, misalign=True),
    _c("wide256_ksplit", 2000, 72, 256, stride2=True, big=True), _c("wide256_ksplit", 700, 64, 256, pruned=True, axis_out=True),
    _c("wide128_ksplit", 3001, 64, 128, full=True),
    _c("wide128_ksplit", 1, 40, 128), _c("wide128_ksplit", 256, 72, 128, iso=True, misalign=True),
    _c("wide128_ksplit", 257, 256, 128, wscale=1e3), _c("wide128_ksplit", 900, 8, 128, pruned=True, axis_out=True),
    _c("wide128_tail", 70000, 32, 128, full=True),
    # k_conv_lin: k = 1 row streams (identity map, and a gather map with holes / repeats: n_in != n_out)
    _c("lin", 3001, 64, 128, full=True),
    _c("lin", 1, 40, 128), _c("lin", 31, 128, 256, gather=True), _c("lin", 32, 64, 128, misalign=True),
    _c("lin", 33, 40, 256, gather=True, axis_out=True), _c("lin", 2000, 128, 128, big=True, gather=True),
    # k_conv_grid (dense-grid promise): unsplit (one 32-channel chunk of a (1, 3, 1) box) and split (7 x 7 x 5 box)
    _c("grid", 1200, 32, 128, full=True, dims=(1, 20, 30, 2), box=(1, 3, 1)),
    _c("grid", 1, 32, 128, dims=(1, 1, 1, 1), box=(1, 3, 1)), _c("grid", 255, 32, 128, dims=(1, 1, 255, 1), box=(1, 3, 1)),
    _c("grid", 256, 32, 256, dims=(1, 1, 256, 1), box=(1, 3, 1), misalign=True),
    _c("grid", 257, 32, 128, dims=(1, 1, 257, 1), box=(1, 3, 1), big=True),
    _c("grid_ksplit", 6688, 64, 128, full=True, dims=(1, 38, 44, 4), box=(7, 7, 5)),
    _c("grid_ksplit", 594, 40, 128, dims=(2, 9, 11, 3), box=(7, 7, 5), misalign=True),
    # row lists (one-pair-per-row maps of generative transposed convolutions: the tail indexed through out_rows)
    _c("rowlist64", 2000, 128, 64, full=True),
    _c("rowlist64", 1, 40, 64), _c("rowlist64", 16, 72, 64, axis_out=True), _c("rowlist64", 17, 64, 64, misalign=True),
    _c("rowlist128", 2000, 256, 128, full=True),
    _c("rowlist128", 16, 128, 128, big=True), _c("rowlist128", 300, 40, 256, axis_out=True),
    # the exact paths the whole-step fallback reruns on: mode 1 (activations split in the kernel), mode 0 (fp32 MFMA)
    _c("mode1", 1000, 64, 64, full=True), _c("mode1", 129, 40, 64, iso=True, misalign=True),
    _c("mode1_ksplit", 1000, 64, 128, full=True), _c("mode1_ksplit", 1, 72, 128, pruned=True),
    _c("mode0", 1000, 64, 64, full=True), _c("mode0", 129, 40, 64, iso=True, misalign=True),
]

_REACHED = {}      # route -> key reached
_WORST = {}        # route -> worst err / A
_RAN = set()       # case ids that passed


def _case_id(c):
    extra = "-".join(k for k in ("full", "iso", "stride2", "pruned", "misalign", "big", "axis_out", "gather") if c.get(k))
    if c.get("wscale"):
        extra += f"-w{c['wscale']:g}"
    return f"{c['route']}-n{c['n']}-{c['cin']}x{c['cout']}" + (f"-{extra}" if extra else "")


def _k3_map(hip, c, g, offs):
    """random sites of a (E, E, 8) box; n_out rows of the output: the same map, a pruned subset of it, or its stride-2 map"""
    n = c["n"]
    n_in = n + n // 2 + 50 if c.get("pruned") else n
    e = max(2, int((4 * n_in / 8) ** 0.5) + 1)
    sites = torch.randperm(e * e * 8, generator=g)[:n_in]
    coords = torch.stack([torch.zeros_like(sites), sites // (e * 8), (sites // 8) % e, sites % 8], 1).int().cuda().contiguous()
    tk, tv, _, _, _ = hip.map_insert(coords, dedup=False)
    if c.get("stride2"):
        out = torch.unique(torch.cat([coords[:, :1], coords[:, 1:] // 2 * 2], 1), dim=0).int().contiguous()
    else:
        out = coords[:n].contiguous()
    return n_in, hip.nbr_build(out, tk, tv, offs)


def _rowlist_map(hip, c, g):
    """n parents (stride 2), their 8 children each (n = 1, 16, 17: all of them; else 80 % kept)"""
    n_par = c["n"] if c["n"] <= 17 else c["n"] // 6
    par = torch.cat([torch.zeros(n_par, 1, dtype=torch.int64), torch.randperm(60 ** 3, generator=g)[:n_par, None]
                     .div(torch.tensor([3600, 60, 1]), rounding_mode="floor") % 60 * 2], 1).int()
    kids = hip.coords_expand(par.cuda().contiguous(), 1)
    if c["n"] > 17:
        kids = kids[(torch.rand(kids.shape[0], generator=g) < 0.8).cuda()].contiguous()
    tk, tv, *_ = hip.map_insert(par.cuda().contiguous(), dedup=False)
    nbr = hip.nbr_build(kids, tk, tv, kernel_offsets(2, 1, 1, True))
    assert bool(((nbr >= 0).sum(0) == 1).all())
    return n_par, nbr


def _problem(hip, oracle, c):
    route = c["route"]
    kind = ROUTES[route][3]
    g = torch.Generator().manual_seed(zlib.crc32(_case_id(c).encode()))
    cin, cout = c["cin"], c["cout"]
    extra = {}
    if kind in ("k3", "k3win"):
        n_in, nbr = _k3_map(hip, c, g, kernel_offsets(3, 1))
    elif kind == "k1x1x3":
        n_in, nbr = _k3_map(hip, c, g, kernel_offsets((1, 1, 3), 1))
    elif kind == "k1":
        n_in, nbr = c["n"], None
        if c.get("gather"):                     # a k = 1 map with holes and repeats
            n_in = c["n"] + 17
            nbr = torch.randint(0, n_in, (1, c["n"]), generator=g, dtype=torch.int32)
            nbr[0, torch.rand(c["n"], generator=g) < 0.1] = -1
            nbr = nbr.cuda()
    elif kind == "grid":
        from tests.test_hip_grid import grid_map
        _, nbr = grid_map(oracle, hip, c["dims"], c["box"])
        nbr = nbr.cuda()
        n_in = nbr.shape[1]
        extra["grid"] = (c["dims"], c["box"])
    else:
        n_in, nbr = _rowlist_map(hip, c, g)
    n_out = nbr.shape[1] if nbr is not None else c["n"]
    iso = []
    if c.get("iso"):
        iso = sorted({0, n_out // 2, n_out - 1})
        nbr[:, iso] = -1
    if kind == "k3win":
        extra["win"] = hip.win_build(nbr)
    if kind == "rl":
        extra["rowlist"] = hip.rowlist_build(nbr)
    kvol = nbr.shape[0] if nbr is not None else 1
    x = torch.randn(n_in, cin, generator=g)
    w = torch.randn(kvol, cin, cout, generator=g) / (kvol * cin / 2) ** 0.5
    if c.get("big"):                            # activations up to 2000, just under the split operand's range guard (2047)
        x = x * (2000.0 / float(x.abs().max()))
        w = w * 1e-3
    if c.get("wscale"):
        w = w * c["wscale"]
    return dict(x=x.cuda(), w=w.cuda(), nbr=nbr, n_out=n_out, extra=extra, iso=iso, g=g)


def _vectors(c, g, n_out):
    cout = c["cout"]
    osc_gain = 1e-3 if (c.get("wscale") or 1.0) > 1 else 1.0      # outputs ~1e3: the emitted operand scaled back into range

    def vec(t):
        t = t.cuda()
        if c.get("misalign"):                   # 4-byte-aligned views: the epilogue's scalar path (par_vec = 0)
            buf = torch.empty(cout + 1, device="cuda")
            buf[1:] = t
            t = buf[1:]
            assert t.data_ptr() % 16 != 0
        return t

    sign = torch.where(torch.rand(cout, generator=g) < 0.25, -1.0, 1.0)
    ac = torch.cat([torch.zeros(n_out, 1, dtype=torch.int32),
                    torch.randint(LO_AXIS, LO_AXIS + T_AXIS, (n_out, 3), generator=g, dtype=torch.int32)], 1)
    if c.get("axis_out"):                       # a third of the rows partly outside [lo, lo + T): clamped, status bit value 4
        out_rows = torch.rand(n_out, generator=g) < 0.34
        out_rows[-1] = True
        col = 1 + int(torch.randint(0, 3, (1,), generator=g))
        ac[out_rows, col] += torch.where(torch.rand(int(out_rows.sum()), generator=g) < 0.5, -T_AXIS, T_AXIS).int()
    return dict(bias=vec(torch.randn(cout, generator=g)), es=vec((torch.rand(cout, generator=g) + 0.5) * sign),
                eb=vec(torch.randn(cout, generator=g) * 0.1), e2s=vec(torch.rand(cout, generator=g) + 0.5),
                e2b=vec(torch.randn(cout, generator=g) * 0.1), osc=vec((torch.rand(cout, generator=g) + 0.5) * osc_gain),
                osh=vec(torch.randn(cout, generator=g) * 0.1 * osc_gain),
                res=torch.randn(n_out, cout, generator=g).cuda(), tab=torch.randn(3, T_AXIS, cout, generator=g).cuda(),
                acoords=ac.cuda().contiguous())


def _combos(c, emits, tails):
    if c["full"]:
        return list(itertools.product(ACTS, tails, (0, 1), emits))
    out = []
    for i, (tail, emit) in enumerate(itertools.product(tails, emits)):
        out.append((ACTS[i % 3], tail, (i // 3) % 2, emit))
    return out


def _spec(v, act, tail, res_on):
    kw = dict(bias=v["bias"], slope=SLOPE)
    if act != 0:
        kw.update(epi_scale=v["es"], epi_shift=v["eb"], epi_act=act)
    if tail == "bn2":
        kw.update(epi2_scale=v["e2s"], epi2_shift=v["e2b"])
    if "residual" in tail:
        kw["residual"] = v["res"]
    if "axis" in tail:
        kw["axis"] = (v["tab"], v["acoords"], LO_AXIS)
    if res_on:
        kw["res_act"] = 2 if act == 2 else 1
    return kw


def _emit_arg(v, emit):
    return {"plain": (None, None, 0), "osp_relu": (v["osc"], v["osh"], 1), "osp_leaky": (v["osc"], v["osh"], 2)}[emit]


def _sample_rows(n_out, iso, g):
    if n_out <= N_SAMPLE:
        return torch.arange(n_out).cuda()
    r = torch.cat([torch.arange(160), torch.arange(n_out - 300, n_out), torch.tensor(iso, dtype=torch.long),
                   torch.arange(65536 - 130, 65536 + 130) if n_out > 65536 + 130 else torch.arange(0),
                   torch.randint(0, n_out, (N_SAMPLE,), generator=g)])
    return torch.unique(r).cuda()


@pytest.mark.parametrize("c", CASES, ids=_case_id)
def test_route_epilogue_against_fp64(hip, oracle, c):
    route = c["route"]
    key, mode, bits, kind = ROUTES[route]
    p = _problem(hip, oracle, c)
    x, w, nbr, n_out, g = p["x"], p["w"], p["nbr"], p["n_out"], p["g"]
    dev = x.device
    try:
        hip.check_status(dev)           # this case's flags only
    except StatusError:
        pass
    v = _vectors(c, g, n_out)
    rows = _sample_rows(n_out, p["iso"], g)
    acc, mag = gather_sum64(x, w, nbr, rows)
    if mode == 2:
        split = hip.split_weight_rows(w)
    elif mode == 1:
        split = hip.split_weight_f16(w)
    else:
        split = None
    emit_ok = mode == 2 and c["cout"] % 32 == 0
    emits = [e for e in EMITS if emit_ok or e == "no"]
    if c.get("wscale", 1.0) > 1:
        emits = [e for e in emits if e != "plain"]        # outputs ~1e3: a plain operand of them is out of range by design
    tails = [t for t in TAILS if not ("axis" in t and (mode != 2 or kind == "grid"))]
    worst = 0.0
    axis_seen = False
    with hip.routing(bits):
        # the refusals by design: mode 0 / 1 serve no per-axis table; k_conv_grid hands it to the gather kernels
        if mode != 2:
            with pytest.raises(ValueError):
                hip.conv_fwd(x, w, nbr, n_out, split=split, axis=(v["tab"], v["acoords"], LO_AXIS), **p["extra"])
        elif kind == "grid":
            hip.conv_fwd(x, w, nbr, n_out, split=split, axis=(v["tab"], v["acoords"], LO_AXIS), **p["extra"])
            assert hip.conv_last_config()["kernel"] != 8
            try:
                hip.check_status(dev)
            except StatusError as e:
                assert e.bits == 4 and c.get("axis_out")
        for act, tail, res_on, emit in _combos(c, emits, tails):
            kw = _spec(v, act, tail, res_on)
            what = f"{_case_id(c)} act={act} tail={tail} res_act={kw.get('res_act', 0)} emit={emit}"
            if emit == "no":
                out = hip.conv_fwd(x, w, nbr, n_out, split=split, **kw, **p["extra"])
            else:
                e = _emit_arg(v, emit)
                out, op = hip.conv_fwd(x, w, nbr, n_out, split=split, emit_split=e, **kw, **p["extra"])
            cfg = hip.conv_last_config()
            got_key = (cfg["kernel"], cfg["bm"], cfg["bn"], cfg["ksplit"] > 1)
            assert got_key == key, f"{what}: reached {got_key}, declared {key} ({cfg})"
            ref, a, ee = epilogue64(acc, mag, kw, rows)
            g_rows = out[rows]
            bad = violations(g_rows, ref, a, ee)
            r = worst_ratio(g_rows, ref, a, ee)
            if bool(bad.any()):
                i, j = (int(t[0]) for t in bad.nonzero(as_tuple=True))
                raise AssertionError(f"{what}: row {int(rows[i])} col {j}: got {float(g_rows[i, j]):.9g}, fp64 {float(ref[i, j]):.9g}, "
                                     f"A {float(a[i, j]):.3g}; {int(bad.sum())} elements outside the bound, worst err / A {r:.3g} "
                                     f"(C = {C_ROUTE:.3g})")
            worst = max(worst, r)
            if emit != "no":
                want = hip.split_rows(out, pro_scale=e[0], pro_shift=e[1], pro_act=e[2], slope=SLOPE)
                assert torch.equal(op.view(torch.int16), want.view(torch.int16)), f"{what}: emitted operand"
                none, only = hip.conv_fwd(x, w, nbr, n_out, split=split, emit_split=e, want_out=False, **kw, **p["extra"])
                assert none is None and torch.equal(only.view(torch.int16), op.view(torch.int16)), f"{what}: operand-only launch"
            axis_seen |= "axis" in tail
            if c.get("axis_out") and "axis" in tail:
                with pytest.raises(StatusError) as ei:
                    hip.check_status(dev)
                assert ei.value.bits == 4, f"{what}: status {ei.value.bits:#x}"
        hip.check_status(dev)
    if c.get("axis_out"):
        assert axis_seen or mode != 2 or kind == "grid"
    _REACHED[route] = key
    _WORST[route] = max(_WORST.get(route, 0.0), worst)
    _RAN.add(_case_id(c))


def test_guarded_module_48_channels_under_inference_mode(hip):
    """A guarded MinkowskiConvolution with 33..64 output channels on a map with window tables (k_conv_wop2 reads fragment-order
    weights cached on the split operand): under torch.inference_mode() the operand is an inference tensor.  Same result as under
    torch.no_grad(); an in-place weight update (load_state_dict) between two forwards changes it (the cache follows the weights)."""
    import pasco_amd.me as ME
    from tests.test_me_guarded_conv import _scene

    coords, feats = _scene(n=20000, extent=(64, 64, 16), c=48, seed=4)
    torch.manual_seed(9)
    conv = ME.MinkowskiConvolution(48, 48, kernel_size=3, bias=True, dimension=3).cuda().eval()

    def run(ctx):
        with ctx():
            return conv(ME.SparseTensor(feats.cuda(), coords.cuda())).F.clone()

    b = run(torch.inference_mode)         # first: the split operand and its fragments are made as inference tensors
    a = run(torch.no_grad)
    assert torch.equal(a, b)
    sd = {k: t.clone() for k, t in conv.state_dict().items()}
    sd["kernel"] = sd["kernel"] * 0.5 + 0.01
    conv.load_state_dict(sd)
    c_inf = run(torch.inference_mode)
    c_ng = run(torch.no_grad)
    assert torch.equal(c_inf, c_ng) and not torch.allclose(c_inf, a)
    hip.check_status(torch.device("cuda", 0))


def test_every_declared_route_was_reached(hip):
    declared = {r for r in ROUTES}
    ran_all = all(_case_id(c) in _RAN for c in CASES)
    print("\n[conv routes] route              key (kernel, bm, bn, ksplit)   worst err / A")
    for r in ROUTES:
        k = _REACHED.get(r)
        print(f"[conv routes] {r:18s} {str(k):30s} {_WORST.get(r, float('nan')):.3e}")
    print(f"[conv routes] C_ROUTE = {C_ROUTE:.3e}, worst over all routes {max(_WORST.values(), default=0.0):.3e}")
    if ran_all:
        assert set(_REACHED) == declared, sorted(declared - set(_REACHED))
    assert all(_REACHED[r] == ROUTES[r][0] for r in _REACHED)
