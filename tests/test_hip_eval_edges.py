"""The four evaluation kernels (include/pasco_eval.h) at their edges and bounds, each table held to the exact restatement
of tests/eval_restate.py: counts and confidence sums bit for bit, -log sums to the fp32 log's ulp.  Class counts 1 .. 32,
argmax ties and NaN, every bin edge, site counts around the launch shape, the PE_MAX_SITES capacity, out-of-range rows,
the IoU = 0.5 match, and a KITTI-360 frame scored end to end on the device."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_restate as R  # noqa: E402
from test_eval_restate_cpu import argmax_rows_cases, edge_confidences  # noqa: E402

DEV = torch.device("cuda")
CHUNK = 2048                 # BLOCK * SITES_PER_THREAD of csrc/eval.hip; MAX_BLOCKS = 1024 -> grid-stride beyond 2^21
MAX_SITES = 1 << 27


def lib():
    from pasco_amd.eval.lib import eval_lib
    return eval_lib()


def run_ssc(probs, conf, sem):
    """pe_ssc on host arrays (or device tensors) -> the table in `SceneEvaluator.add`'s layout."""
    from pasco_amd.eval.lib import SSC_SUMS, ssc_counts
    L = lib()
    p = torch.as_tensor(probs).to(DEV).contiguous()
    S, C = p.shape
    ws = torch.empty(L.ssc_workspace_bytes(S, C) // 8 + 1, dtype=torch.int64, device=DEV)
    out = torch.full((ssc_counts(C) + SSC_SUMS,), -7, dtype=torch.int64, device=DEV)
    L.ssc(p, torch.as_tensor(conf).to(DEV).contiguous(), torch.as_tensor(sem).to(DEV).contiguous(), ws, out.data_ptr(),
          out.data_ptr() + 8 * ssc_counts(C))
    h = out.cpu().numpy()
    n = ssc_counts(C)
    sums = h[n:].view(np.float64)
    return {"cm": h[:C * C].reshape(C, C), "unknown": int(h[C * C]), "bin_count": h[C * C + 1:C * C + 33].reshape(2, 16),
            "bin_correct": h[C * C + 33:n].reshape(2, 16), "bin_conf": sums[:32].reshape(2, 16), "nll": sums[32:]}


def run_rows(site, pred, conf, sem, gt_id, gt_area, P, G):
    """pe_panop_pairs -> pe_match -> pe_mask_ece on host arrays -> area / inter / map / mask tables."""
    L = lib()
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(dt).to(DEV)
    s_d, p_d, c_d = t(site, torch.int64), t(pred, torch.int32), t(conf, torch.float32)
    sem_d, gid_d, ga_d = t(sem, torch.uint8), t(gt_id, torch.int32), t(gt_area, torch.int64)
    area = torch.full((P + 1,), -7, dtype=torch.int64, device=DEV)
    inter = torch.full(((G + 1) * (P + 1),), -7, dtype=torch.int64, device=DEV)
    mp = torch.full((P + 1,), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((32,), -7, dtype=torch.int64, device=DEV)
    sums = torch.full((16,), -7.0, dtype=torch.float64, device=DEV)
    L.panop_pairs(s_d, p_d, sem_d, gid_d, P, G, area.data_ptr(), inter.data_ptr())
    L.match(area.data_ptr(), ga_d, inter.data_ptr(), P, G, mp.data_ptr())
    ws = torch.empty(L.ece_workspace_bytes(s_d.numel()) // 8 + 1, dtype=torch.int64, device=DEV)
    L.mask_ece(s_d, p_d, c_d, gid_d, mp.data_ptr(), P, ws, counts.data_ptr(), sums.data_ptr())
    c = counts.cpu().numpy()
    return {"area": area.cpu().numpy(), "inter": inter.cpu().numpy().reshape(G + 1, P + 1), "map": mp.cpu().numpy(),
            "mask_count": c[:16], "mask_correct": c[16:], "mask_conf": sums.cpu().numpy()}


def random_ssc(S, C, seed, layout="changing"):
    g = np.random.default_rng(seed)
    if layout == "runs":                        # long runs of one (gt, pred, bin) key: empty space
        run = 3000
        n_runs = (S + run - 1) // run
        rp = g.dirichlet(np.ones(C), max(n_runs, 1)).astype(np.float32)
        probs = np.repeat(rp, run, 0)[:S]
        conf = np.repeat(g.random(max(n_runs, 1)).astype(np.float32), run)[:S]
        sem = np.repeat(g.integers(0, C, max(n_runs, 1)), run)[:S].astype(np.uint8)
        sem[np.repeat(g.random(max(n_runs, 1)) < 0.1, run)[:S]] = 255
    else:                                       # a new key at every site
        probs = g.random((S, C), dtype=np.float32)
        conf = g.random(S, dtype=np.float32)
        sem = g.integers(0, C, S).astype(np.uint8)
        sem[g.random(S) < 0.05] = 255
    return probs, conf, sem


@pytest.mark.parametrize("C", [1, 2, 19, 20, 32])
def test_ssc_at_every_class_count(hip, C):
    probs, conf, sem = random_ssc(6001, C, seed=C)
    probs[::7, 0] = 2.0                                              # a populated pred == 0 group at every C
    ex = R.ssc_exact(probs, conf, sem)
    R.check_ssc(run_ssc(probs, conf, sem), ex)


def test_ssc_refuses_class_counts_out_of_range(hip):
    for C in (0, 33):
        with pytest.raises(RuntimeError, match="classes"):
            run_ssc(np.zeros((4, C), np.float32), np.zeros(4, np.float32), np.zeros(4, np.uint8))


def test_argmax_rows_ties_zeros_subnormals_and_nan(hip):
    p = argmax_rows_cases()
    n = p.shape[0]
    # every row under every label: a NaN at p[g] (row 6 label 0, row 7 label 1, ...) among them
    probs = np.repeat(p, 4, 0)
    sem = np.tile(np.arange(4), n).astype(np.uint8)
    conf = np.full(probs.shape[0], 0.5, np.float32)
    ex = R.ssc_exact(probs, conf, sem)
    assert np.array_equal(R.argmax_rows(probs), torch.from_numpy(probs).argmax(1).numpy())
    R.check_ssc(run_ssc(probs, conf, sem), ex)


def test_confidence_bins_at_every_edge_both_groups_and_mask_ece(hip):
    c = edge_confidences()
    n = c.shape[0]
    probs = np.zeros((2 * n, 3), np.float32)
    probs[:n, 0] = 1.0                                               # group 0 (pred == 0)
    probs[n:, 2] = 1.0                                               # group 1 (pred != 0)
    conf = np.concatenate([c, c])
    sem = np.concatenate([np.zeros(n), np.full(n, 2)]).astype(np.uint8)
    ex = R.ssc_exact(probs, conf, sem)
    got = run_ssc(probs, conf, sem)
    R.check_ssc(got, ex)
    assert got["bin_count"][0, 15] == got["bin_count"][1, 15] == ex["bin_count"][0, 15] >= 5    # 1.0, > 1, inf, NaN
    # the mask bins over the same confidences, with the gt_id == 0 and conf == 0 exclusions
    S = 8
    gt_id = np.array([0, 1, 2, 3, 1, 2, 0, 3])
    site = np.arange(2 * n) % S
    pred = np.arange(2 * n) % 4
    conf_r = conf.copy()
    conf_r[::5] = 0.0
    conf_r[1::11] = -0.0
    gt_area = np.array([0, 4, 4, 4])
    ex = R.rows_exact(site, pred, conf_r, np.ones(S, np.uint8), gt_id, gt_area, 3, 3)
    R.check_rows(run_rows(site, pred, conf_r, np.ones(S, np.uint8), gt_id, gt_area, 3, 3), ex)
    assert ex["mask_count"].sum() < (gt_id[site] != 0).sum()


SITE_COUNTS = [0, 1, 255, CHUNK - 1, CHUNK, CHUNK + 1, (1 << 21) - 1, 1 << 21, (1 << 21) + 1]


@pytest.mark.parametrize("layout", ["runs", "changing"])
@pytest.mark.parametrize("S", SITE_COUNTS)
def test_site_counts_around_the_launch_shape(hip, S, layout):
    probs, conf, sem = random_ssc(S, 3, seed=S + (layout == "runs"), layout=layout)
    R.check_ssc(run_ssc(probs, conf, sem), R.ssc_exact(probs, conf, sem, fp64=S <= (1 << 16)))
    # the same count of sparse rows through the row kernels
    g = np.random.default_rng(S)
    n_s = max(S, 1)
    sem_r = np.where(g.random(n_s) < 0.05, 255, 1).astype(np.uint8)
    gt_id = np.repeat(g.integers(0, 6, n_s // 500 + 1), 500)[:n_s] if layout == "runs" else g.integers(0, 6, n_s)
    gt_area = np.bincount(gt_id, minlength=6) + 1
    site = np.arange(S) if layout == "runs" else g.permutation(S)
    pred = (site // 700 % 5).astype(np.int64) if layout == "runs" else g.integers(0, 5, S)
    ex = R.rows_exact(site, pred, conf, sem_r, gt_id, gt_area, 4, 5, fp64=S <= (1 << 16))
    R.check_rows(run_rows(site, pred, conf, sem_r, gt_id, gt_area, 4, 5), ex)


def test_many_grid_stride_passes(hip):
    """About 2^24 sites at C = 2: every thread of the 1024 blocks walks 64 grid-stride passes."""
    S = (1 << 24) + 777
    for layout in ("runs", "changing"):
        probs, conf, sem = random_ssc(S, 2, seed=24, layout=layout)
        R.check_ssc(run_ssc(probs, conf, sem), R.ssc_exact(probs, conf, sem, fp64=False))


def test_capacity_of_the_fixed_point_sums(hip):
    """PE_MAX_SITES sites of conf 1.0 in one bin: the sum is 2^63 in units of 2^-36 (signed int64 overflows there)."""
    n = MAX_SITES
    got = run_ssc(torch.ones(n, 1, device=DEV), torch.ones(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV))
    torch.cuda.empty_cache()
    assert got["cm"][0, 0] == n and got["unknown"] == 0
    assert got["bin_count"][0, 15] == n and got["bin_count"].sum() == n and got["bin_correct"][0, 15] == n
    assert got["bin_conf"][0, 15] == float(n), got["bin_conf"][0, 15]
    assert not got["bin_conf"][0, :15].any() and not got["bin_conf"][1].any()
    assert got["nll"].tolist() == [0.0, 0.0]                          # -log(1 + 1e-12f) = -log(1)

    L = lib()
    site = torch.zeros(n, dtype=torch.int64, device=DEV)
    pred = torch.ones(n, dtype=torch.int32, device=DEV)
    conf = torch.ones(n, device=DEV)
    gt_id = torch.ones(1, dtype=torch.int32, device=DEV)
    mp = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    counts = torch.zeros(32, dtype=torch.int64, device=DEV)
    sums = torch.zeros(16, dtype=torch.float64, device=DEV)
    ws = torch.empty(L.ece_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device=DEV)
    L.mask_ece(site, pred, conf, gt_id, mp.data_ptr(), 1, ws, counts.data_ptr(), sums.data_ptr())
    c, s = counts.cpu().numpy(), sums.cpu().numpy()
    del site, pred, conf
    torch.cuda.empty_cache()
    assert c[15] == n and c[31] == n and c.sum() == 2 * n
    assert s[15] == float(n), s[15]

    # one beyond the bound is refused before any launch (the pointers are never read)
    e = torch.zeros(1, device=DEV)
    p = e.data_ptr()
    assert L.lib.pe_ssc(p, p, p, n + 1, 1, L._edges, p, 1 << 40, p, p, L._stream(e)) != 0
    assert b"at most" in L.lib.pe_last_error()
    assert L.lib.pe_mask_ece(p, p, p, n + 1, p, 1, p, 1, L._edges, p, 1 << 40, p, p, L._stream(e)) != 0
    assert b"at most" in L.lib.pe_last_error()


def test_panoptic_tables_at_zero_and_full_size(hip):
    g = np.random.default_rng(11)
    S = 40000
    sem = np.where(g.random(S) < 0.1, 255, 3).astype(np.uint8)
    for P, G in ((0, 0), (128, 1023)):
        gt_id = g.integers(0, G + 1, S)
        gt_area = np.bincount(gt_id, minlength=G + 1) + 1
        site = g.integers(0, S, 30000)
        pred = g.integers(0, P + 1, 30000)
        conf = g.random(30000).astype(np.float32)
        R.check_rows(run_rows(site, pred, conf, sem, gt_id, gt_area, P, G), R.rows_exact(site, pred, conf, sem, gt_id,
                                                                                        gt_area, P, G))


def test_out_of_range_rows(hip):
    """Site -1 / >= S and pred < 0 / > P are not counted; a gt id > G counts in `area` but in no `inter` cell
    (pasco_eval.h); a pred id outside 0 .. P maps to 0 in the mask bins."""
    S, P, G = 10, 3, 2
    sem = np.array([1, 1, 1, 255, 1, 1, 1, 1, 1, 1], np.uint8)
    gt_id = np.array([1, 1, 2, 0, 5, 2, 1, -3, 2, 1])              # 5 > G, -3 < 0
    site = np.array([0, 1, -1, 10, 11, 2, 4, 4, 7, 3, 5, 6, 8, 9])
    pred = np.array([1, 1, 1, 1, 1, -1, 4, 2, 2, 2, 3, 3, 3, 9])
    conf = np.linspace(0.05, 0.95, site.shape[0]).astype(np.float32)
    gt_area = np.array([0, 4, 3])
    ex = R.rows_exact(site, pred, conf, sem, gt_id, gt_area, P, G)
    got = run_rows(site, pred, conf, sem, gt_id, gt_area, P, G)
    R.check_rows(got, ex)
    assert got["area"].tolist() == [0, 2, 2, 3]                      # gt id 5 and -3 rows (pred 2) in area
    assert got["inter"][:, 2].tolist() == [0, 0, 0] and got["inter"][1, 1] == 2


def test_match_at_iou_one_half_and_beyond_2_31(hip):
    L = lib()
    P, G = 4, 3
    big = 3 << 31
    area = np.array([0, 4, 5, big, big], np.int64)
    gt_area = np.array([0, 2, 3, big, big + 1], np.int64)[:G + 1]
    inter = np.zeros((G + 1, P + 1), np.int64)
    inter[1, 1] = 2          # 2 * 2 == 4 + 2 - 2: IoU exactly 0.5, no match
    inter[2, 2] = 3          # 6 > 5 + 3 - 3: a match one intersection above
    inter[2, 1] = 1
    inter[3, 3] = big        # identical areas beyond 2^31
    inter[3, 4] = big // 2 + 1
    inter[1, 4] = 1
    t = lambda a: torch.as_tensor(a).to(DEV)
    a_d, ga_d, i_d = t(area), t(gt_area), t(inter.reshape(-1))
    mp = torch.full((P + 1,), -1, dtype=torch.int32, device=DEV)
    L.match(a_d.data_ptr(), ga_d, i_d.data_ptr(), P, G, mp.data_ptr())
    got = mp.cpu().numpy()
    assert np.array_equal(got, R.match_exact(area, gt_area, inter))
    assert got.tolist() == [0, 0, 2, 3, 0]
    inter[2, 2] = 2          # 4 < 5 + 3 - 2: below one half
    i_d = t(inter.reshape(-1))
    L.match(a_d.data_ptr(), ga_d, i_d.data_ptr(), P, G, mp.data_ptr())
    assert mp.cpu().tolist() == [0, 0, 0, 3, 0]


def test_device_logf_against_the_correctly_rounded_log(hip):
    """One value per group and call, repeated over 64 sites: the group sum is 64 times one device term, so its distance from
    the correctly rounded term is measured without cancellation.  Terms >= 2^-7 are multiples of 2^-30: the fixed point
    is exact.  The worst distance is the NLL_ULPS of the -log bound."""
    g = np.random.default_rng(7)
    vals = np.concatenate([np.float32(10.0) ** -g.uniform(0.01, 12, 600), g.uniform(0.01, 0.99, 400)]).astype(np.float32)
    worst, at = 0.0, None
    n = 64
    tables = []
    for a, b in zip(vals[0::2], vals[1::2]):
        probs = np.zeros((2 * n, 2), np.float32)
        probs[:n] = [a, 0.0]             # pred 0, label 0: term -log(a)
        probs[n:] = [0.0, b]             # pred 1, label 1: term -log(b)
        sem = np.repeat(np.array([0, 1], np.uint8), n)
        ex = R.ssc_exact(probs, np.full(2 * n, 0.5, np.float32), sem, fp64=False)
        got = run_ssc(probs, np.full(2 * n, 0.5, np.float32), sem)
        for k, v in ((0, a), (1, b)):
            t = R.nll_terms(np.float32([v]))
            d = abs(float(got["nll"][k]) - R.fx_value(ex["nll_fx"][k], R.NLL_SHIFT)) / n / R.ulp32(t)[0]
            if d > worst:
                worst, at = d, float(v)
        tables.append((got, ex))
    print(f"\n[eval] worst device logf distance from the correctly rounded fp32 log: {worst:.3f} ulp (p = {at!r})")
    assert worst <= R.NLL_ULPS
    for got, ex in tables:
        R.check_ssc(got, ex)


def test_evaluator_refuses_a_20_class_grid_at_19_classes(hip):
    from pasco_amd.eval import GroundTruth, SceneEvaluator
    sem = np.full((8, 8, 4), 19, np.uint8)
    gt = GroundTruth.from_labels(sem, np.zeros_like(sem), (1,), device=DEV)
    ev = SceneEvaluator(n_classes=19, thing_ids=(1, 2, 3, 4, 5, 6), n_outputs=1)
    with pytest.raises(ValueError, match="label 19"):
        ev.add([None], [torch.zeros(19, 8, 8, 4, device=DEV)], gt)


def test_kitti360_frame_scored_on_the_device_equals_the_restatement(hip, tmp_path):
    from test_hip_eval import assert_tables_equal, restated_outputs
    from test_kitti360_cpu import FRAME, MINI, SEQ, kitti360_checkpoint, reader
    from pasco_amd.data import net_from_checkpoint
    from pasco_amd.data.kitti360 import THING_IDS
    from pasco_amd.eval import GroundTruth, SceneEvaluator
    from pasco_amd.eval.kitti import subnet_transforms
    import pasco_amd.eval.kitti360 as E
    ck = kitti360_checkpoint(os.path.join(tmp_path, "k360.ckpt"))
    net = net_from_checkpoint(ck, device=DEV, thing_ids=THING_IDS)
    r = reader()
    sem, ins = r.labels(SEQ, FRAME)
    net.ensembler.scene_size = tuple(int(v) for v in sem.shape)
    b = r.batch(SEQ, FRAME, subnet_transforms(net.n_infers), device=DEV)
    with torch.no_grad():
        outs, sem_probs, _ = net.step_inference([t.to(DEV) for t in b["in_feats"]], [t.to(DEV) for t in b["in_coords"]],
                                                [t.to(DEV) for t in b["Ts"]], b["global_min_Cs"], b["global_max_Cs"],
                                                b["min_Cs"], b["max_Cs"])
    assert sem_probs[0].shape[0] == 19
    gt = GroundTruth.from_labels(sem, ins, THING_IDS, device=DEV)
    ev = SceneEvaluator(n_classes=19, thing_ids=THING_IDS, n_outputs=len(outs))
    ev.add(outs, sem_probs, gt)
    for got, exp in zip(ev.last_add_tables, restated_outputs(outs, sem_probs, gt.to("cpu"))):
        assert_tables_equal(got, exp)
    kw = dict(root=MINI, preprocess_root=os.path.join(MINI, "preprocess"), label_root=os.path.join(MINI, "sscbench"),
              match_file=os.path.join(MINI, "match.txt"), ckpt=ck, frames=1)
    a, _ = E.evaluate(device_prep=True, **kw)
    h, _ = E.evaluate(device_prep=False, **kw)
    assert a.tables() == h.tables()
