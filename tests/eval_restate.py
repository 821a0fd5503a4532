"""Per-voxel torch-CPU restatement of the evaluation tables (the layout `SceneEvaluator.add_tables` takes), written from the
metric definitions with `torch.unique` and boolean masks - the checker of the HIP kernels of include/pasco_eval.h.

The second half restates the kernels' own arithmetic in numpy: argmax and bins with torch's semantics, and every floating
sum as the exact integer the fixed-point format of pasco_eval.h adds up (`ssc_exact`, `rows_exact`).  `check_ssc` and
`check_rows` hold a table to them: counts and confidence sums bit for bit, the -log sums to the fp32 log's ulp."""
import math

import numpy as np
import torch

BINS = 16
CONF_SHIFT, NLL_SHIFT = 36, 30      # fixed point of the confidence and -log sums
CONF_LIMIT = 512.0                  # finite confidences saturate here
NLL_ULPS = 2.0                      # device logf against the correctly rounded fp32 log: 2 ulps measured on the MI355X
EDGES = torch.linspace(0, 1, BINS)


def bins_of(conf):
    return (torch.bucketize(conf, torch.linspace(0, 1, BINS), right=True) - 1).clamp_min(0)


def binned(conf, correct):
    b = bins_of(conf)
    count = torch.stack([(b == i).sum() for i in range(BINS)]).numpy()
    cor = torch.stack([(correct & (b == i)).sum() for i in range(BINS)]).numpy()
    csum = np.array([conf[b == i].double().sum().item() for i in range(BINS)])
    return count, cor, csum


def ssc_tables(probs, conf, sem):
    """probs [S, C] fp32, conf [S] fp32, sem [S] uint8 -> cm / unknown / bins / nll."""
    C = probs.shape[1]
    known = sem != 255
    pred = probs.argmax(1)
    g, p = sem[known].long(), pred[known]
    pairs, cnt = torch.unique(g * C + p, return_counts=True)
    cm = np.zeros((C, C), np.int64)
    cm.reshape(-1)[pairs.numpy()] = cnt.numpy()
    out = {"cm": cm, "unknown": int((~known).sum())}
    bc, bk, bs, nll = [], [], [], []
    for grp in (p == 0, p != 0):
        c, k, s = binned(conf[known][grp], (p == g)[grp])
        bc.append(c); bk.append(k); bs.append(s)
        nll.append(float(-torch.log(probs[known][grp].gather(1, g[grp][:, None]) + 1e-12).double().sum()))
    out.update(bin_count=np.stack(bc), bin_correct=np.stack(bk), bin_conf=np.stack(bs), nll=np.array(nll))
    out["exact"] = ssc_exact(probs.numpy(), conf.numpy(), sem.numpy())
    return out


def panoptic_tables(pan, vconf, sem, gt_id, gt_area, infos, n_classes):
    """pan [S] int32 pred ids and vconf [S] fp32 on the dense grid, gt_id [S] (0 at unknown), gt_area [G + 1]."""
    known = sem != 255
    P = max([int(e["id"]) for e in infos] + [int(pan.max()), 0])
    G = gt_area.shape[0] - 1
    pz = torch.where(known, pan, torch.zeros_like(pan)).long()
    area = np.zeros(P + 1, np.int64)
    ids, cnt = torch.unique(pz[known], return_counts=True)
    area[ids.numpy()] = cnt.numpy()
    inter = np.zeros((G + 1, P + 1), np.int64)
    keys, cnt = torch.unique(gt_id[known].long() * (P + 1) + pz[known], return_counts=True)
    inter.reshape(-1)[keys.numpy()] = cnt.numpy()
    mp = np.zeros(P + 1, np.int32)
    for p in range(1, P + 1):
        for g in range(1, G + 1):
            i = inter[g, p]
            if area[p] > 0 and i > 0 and 2 * i > area[p] + gt_area[g] - i:
                mp[p] = g
                break
    mapped = torch.from_numpy(mp).long()[pz]
    sel = (gt_id != 0) & (vconf != 0)
    mc, mk, ms = binned(vconf[sel], mapped[sel] == gt_id[sel].long())
    mex = binned_exact(vconf[sel].numpy(), (mapped[sel] == gt_id[sel].long()).numpy())
    segs = [{"id": int(e["id"]), "category_id": int(e["category_id"]), "confidence": float(e["confidence"]),
             "logp": torch.log(torch.as_tensor(e["all_class_probs"]).float() + 1e-8).numpy()} for e in infos]
    return {"area": area, "inter": inter, "map": mp, "mask_count": mc, "mask_correct": mk, "mask_conf": ms, "segments": segs,
            "mask_conf_fx": mex["conf_fx"][0], "mask_conf_fp64": mex["conf_fp64"][0]}


def scene_tables(probs, conf, sem, pan, vconf, gt_id, gt_area, infos, n_classes=20):
    t = ssc_tables(probs, conf, sem)
    t.update(panoptic_tables(pan, vconf, sem, gt_id, gt_area, infos, n_classes))
    return t


# ---- exact restatement of the kernels' arithmetic ------------------------------------------------------------------------
def argmax_rows(p):
    """torch.argmax(p, 1): the first maximum, a NaN being the maximum (the first NaN wins), -0.0 == +0.0."""
    p = np.asarray(p, np.float32)
    if p.shape[0] == 0:
        return np.zeros(0, np.int64)
    nan = np.isnan(p)
    top = np.where(nan, -np.inf, p).max(1)
    first_max = (p == top[:, None]).argmax(1)
    return np.where(nan.any(1), nan.argmax(1), first_max).astype(np.int64)


def bin_index(conf):
    """(torch.bucketize(conf, EDGES, right=True) - 1).clamp_min(0): NaN past every edge (bin 15), below 0 in bin 0."""
    c = np.asarray(conf, np.float32)
    n = np.searchsorted(EDGES.numpy(), c, side="right")            # edges <= c
    return np.where(np.isnan(c), BINS - 1, np.maximum(n - 1, 0)).astype(np.int64)


def conf_fixed(conf):
    """rint(conf * 2^36) per confidence: NaN / +-inf add 0, finite values saturate at +-CONF_LIMIT.  An fp32 value times a
    power of two is exact in fp64, and np.rint rounds half to even as llrint does."""
    c = np.asarray(conf, np.float32).astype(np.float64)
    c = np.clip(np.where(np.isfinite(c), c, 0.0), -CONF_LIMIT, CONF_LIMIT)
    return np.rint(c * 2.0 ** CONF_SHIFT).astype(np.int64)


def nll_terms(pg):
    """-log(p[g] + 1e-12) per site: the sum in fp32 as on the device, then the log in fp64 rounded to fp32 - the correctly
    rounded fp32 term, which the device logf meets to NLL_ULPS."""
    x = np.asarray(pg, np.float32) + np.float32(1e-12)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (-np.log(x.astype(np.float64))).astype(np.float32)


def nll_fixed(t):
    t = np.asarray(t, np.float32).astype(np.float64)
    return np.rint(np.where(np.isfinite(t), t, 0.0) * 2.0 ** NLL_SHIFT).astype(np.int64)


def keyed_sum(key, v, n):
    """Exact integer sums of int64 `v` per key 0 .. n-1 (Python ints: the total can pass 2^63).  The values are cut in
    16-bit pieces so that every float64 partial sum of np.bincount stays an exact integer."""
    key = np.asarray(key, np.int64)
    v = np.asarray(v, np.int64)
    tot = [0] * n
    for part, sh in ((v >> 32, 32), ((v >> 16) & 0xFFFF, 16), (v & 0xFFFF, 0)):
        s = np.bincount(key, weights=part.astype(np.float64), minlength=n)
        for k in range(n):
            tot[k] += int(s[k]) << sh
    return tot


def fx_value(total, shift):
    """The fp64 a kernel returns for a fixed-point total: rounded to fp64 once, then scaled (exactly) by 2^-shift."""
    return float(total) / 2.0 ** shift


def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def binned_exact(conf, correct, group=None, fp64=True):
    """Counts, correct counts and exact fixed-point confidence sums per (group, bin); `conf_fp64`: the plain fp64 sum
    (math.fsum of the finite, saturated confidences) per bin, None when `fp64` is off."""
    conf = np.asarray(conf, np.float32)
    grp = np.zeros(conf.shape[0], np.int64) if group is None else np.asarray(group, np.int64)
    n_grp = 1 if group is None else 2
    key = grp * BINS + bin_index(conf)
    count = np.bincount(key, minlength=n_grp * BINS).reshape(n_grp, BINS)
    cor = np.bincount(key[np.asarray(correct, bool)], minlength=n_grp * BINS).reshape(n_grp, BINS)
    fx = np.array(keyed_sum(key, conf_fixed(conf), n_grp * BINS), dtype=object).reshape(n_grp, BINS)
    out = {"count": count, "correct": cor, "conf_fx": fx, "conf_fp64": None}
    if fp64:
        c = np.clip(np.where(np.isfinite(conf), conf.astype(np.float64), 0.0), -CONF_LIMIT, CONF_LIMIT)
        order = np.argsort(key, kind="stable")
        cuts = np.searchsorted(key[order], np.arange(n_grp * BINS + 1))
        cs = c[order]
        out["conf_fp64"] = np.array([math.fsum(cs[cuts[k]:cuts[k + 1]].tolist()) for k in range(n_grp * BINS)]).reshape(
            n_grp, BINS)
    return out


def ssc_exact(probs, conf, sem, fp64=True):
    """pe_ssc's tables restated in numpy: probs [S, C] fp32, conf [S] fp32, sem [S] uint8 (labels < C or 255)."""
    p = np.asarray(probs, np.float32)
    cf = np.asarray(conf, np.float32)
    g = np.asarray(sem).astype(np.int64)
    C = p.shape[1]
    known = g != 255
    assert (g[known] < C).all(), "labels >= C are refused by the host"
    pk, gk = p[known], g[known]
    pred = argmax_rows(pk)
    grp = (pred != 0).astype(np.int64)
    b = binned_exact(cf[known], pred == gk, grp, fp64)
    t = nll_terms(pk[np.arange(gk.shape[0]), gk])
    fin = np.isfinite(t)
    return {"cm": np.bincount(gk * C + pred, minlength=C * C).reshape(C, C), "unknown": int((~known).sum()),
            "bin_count": b["count"], "bin_correct": b["correct"], "bin_conf_fx": b["conf_fx"], "bin_conf_fp64": b["conf_fp64"],
            "nll_fx": keyed_sum(grp, nll_fixed(t), 2),
            "nll_n": np.bincount(grp, minlength=2),
            "nll_ulp": np.bincount(grp[fin], weights=ulp32(t[fin]), minlength=2)}


def rows_exact(site, pred, conf, sem, gt_id, gt_area, P, G, fp64=True):
    """pe_panop_pairs / pe_match / pe_mask_ece restated over sparse rows, out-of-range rows as pasco_eval.h says."""
    site = np.asarray(site, np.int64)
    pred = np.asarray(pred, np.int64)
    conf = np.asarray(conf, np.float32)
    sem = np.asarray(sem)
    gt_id = np.asarray(gt_id, np.int64)
    gt_area = np.asarray(gt_area, np.int64)
    S = sem.shape[0]
    ok = (site >= 0) & (site < S)
    s = np.where(ok, site, 0)
    g = gt_id[s]
    row = ok & (sem[s] != 255) & (pred >= 0) & (pred <= P)
    area = np.bincount(pred[row], minlength=P + 1).astype(np.int64)
    pair = row & (g >= 0) & (g <= G)
    inter = np.bincount(g[pair] * (P + 1) + pred[pair], minlength=(G + 1) * (P + 1)).reshape(G + 1, P + 1).astype(np.int64)
    mp = match_exact(area, gt_area, inter)
    sel = ok & (g != 0) & (conf != 0)
    mapped = np.where((pred >= 0) & (pred <= P), mp[np.clip(pred, 0, P)], 0)
    b = binned_exact(conf[sel], mapped[sel] == g[sel], fp64=fp64)
    return {"area": area, "inter": inter, "map": mp, "mask_count": b["count"][0], "mask_correct": b["correct"][0],
            "mask_conf_fx": b["conf_fx"][0], "mask_conf_fp64": None if b["conf_fp64"] is None else b["conf_fp64"][0]}


def match_exact(area, gt_area, inter):
    """map[p] = the first gt id g >= 1 with 2 * inter > area_p + gt_area_g - inter (Python ints: no overflow)."""
    G1, P1 = inter.shape
    mp = np.zeros(P1, np.int32)
    for p in range(1, P1):
        if int(area[p]) <= 0:
            continue
        for g in range(1, G1):
            i = int(inter[g, p])
            if i > 0 and 2 * i > int(area[p]) + int(gt_area[g]) - i:
                mp[p] = g
                break
    return mp


def check_conf_sums(got, fx, fp64, count, what):
    """Bit for bit against the fixed-point total; the fixed-point value against the plain fp64 sum within count * 2^-37
    (the format's cost) plus the fp64 rounding of the two."""
    got = np.asarray(got, np.float64).reshape(-1)
    fx = np.asarray(fx, dtype=object).reshape(-1)
    count = np.asarray(count).reshape(-1)
    for b in range(got.shape[0]):
        exp = fx_value(fx[b], CONF_SHIFT)
        assert got[b] == exp, f"{what}[{b}]: {got[b]!r} != fixed-point {exp!r}"
        if fp64 is not None:
            ref = float(np.asarray(fp64).reshape(-1)[b])
            tol = count[b] * 2.0 ** -(CONF_SHIFT + 1) + 2 * math.ulp(max(abs(ref), abs(exp)))
            assert abs(exp - ref) <= tol, f"{what}[{b}]: fixed point {exp!r} vs fp64 {ref!r}"


def check_ssc(got, ex, nll_ulps=NLL_ULPS):
    """A pe_ssc table (the `add` layout) against `ssc_exact`."""
    for key in ("cm", "bin_count", "bin_correct"):
        assert np.array_equal(np.asarray(got[key]), np.asarray(ex[key])), key
    assert int(got["unknown"]) == ex["unknown"], "unknown"
    check_conf_sums(got["bin_conf"], ex["bin_conf_fx"], ex["bin_conf_fp64"], ex["bin_count"], "bin_conf")
    for k in range(2):
        exp = fx_value(ex["nll_fx"][k], NLL_SHIFT)
        tol = float(ex["nll_n"][k]) * 2.0 ** -NLL_SHIFT + nll_ulps * ex["nll_ulp"][k] + math.ulp(abs(exp))
        assert abs(float(got["nll"][k]) - exp) <= tol, f"nll[{k}]: {float(got['nll'][k])!r} vs {exp!r} (tol {tol:.3g})"


def check_rows(got, ex):
    """pe_panop_pairs / pe_match / pe_mask_ece tables against `rows_exact`."""
    for key in ("area", "inter", "map", "mask_count", "mask_correct"):
        assert np.array_equal(np.asarray(got[key]), np.asarray(ex[key])), key
    check_conf_sums(got["mask_conf"], ex["mask_conf_fx"], ex["mask_conf_fp64"], ex["mask_count"], "mask_conf")
