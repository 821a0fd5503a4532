"""The evaluation kernels (include/pasco_eval.h, csrc/eval.hip) on the MI355X: every case of tests/golden/eval.npz through
`SceneEvaluator.add`, bounds, run-to-run identity, and a full-size S10 MIMO-3 step scored on the device against the torch
restatement of the same outputs on the host."""
import os
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_restate as R  # noqa: E402
from test_eval_cpu import GOLD, GRID, NO, NS, check_stats, gt_of, infos_of, restated_tables  # noqa: E402

INT_KEYS = ("cm", "unknown", "bin_count", "bin_correct", "mask_count", "mask_correct", "map")


class Rows:
    """A panoptic output as the device path holds it: sparse rows + segment table."""

    def __init__(self, pan, vconf, infos, grid, conf, device):
        X, Y, Z = grid
        site = torch.nonzero((pan != 0) | (vconf != 0)).reshape(-1)
        xyz = torch.stack([site // (Y * Z), (site // Z) % Y, site % Z], 1)
        self.coords = torch.cat([torch.zeros_like(xyz[:, :1]), xyz], 1).to(torch.int32).to(device)
        self.pan, self.vconf = pan[site].to(torch.int32).to(device), vconf[site].float().to(device)
        self.grid = grid
        self.d = {"segments_infos": [infos], "ssc_confidence": conf.reshape(grid).to(device)}

    def sparse_rows(self):
        return self.coords, self.grid, torch.zeros(3, dtype=torch.int32, device=self.coords.device), self.pan, self.vconf

    def __getitem__(self, k):
        return self.d[k]


def fixture_scene(k, dev):
    outs, probs = [], []
    for o in range(NO):
        p = torch.from_numpy(GOLD["in_prob"][k, o])
        probs.append(p.to(dev).reshape(GRID + (p.shape[1],)).permute(3, 0, 1, 2))
        outs.append(Rows(torch.from_numpy(GOLD["in_pan"][k, o]), torch.from_numpy(GOLD["in_vconf"][k, o]), infos_of(k, o), GRID,
                         torch.from_numpy(GOLD["in_conf"][k, o]), dev))
    return outs, probs


def assert_tables_equal(got, exp):
    for key in INT_KEYS:
        assert np.array_equal(np.asarray(got[key]), np.asarray(exp[key])), key
    # the kernels count rows; the restatement counts every known site (pred id 0 included): compare the pred ids >= 1
    assert np.array_equal(got["area"][1:], exp["area"][1:])
    assert np.array_equal(got["inter"][:, 1:], exp["inter"][:, 1:])
    # sums per bin and group: confidences bit for bit with the fixed-point expectation, -log to the fp32 log's ulp
    R.check_ssc(got, exp["exact"])
    R.check_conf_sums(got["mask_conf"], exp["mask_conf_fx"], exp["mask_conf_fp64"], exp["mask_count"], "mask_conf")
    for a, b in zip(got["segments"], exp["segments"]):
        assert a["id"] == b["id"] and a["category_id"] == b["category_id"]
        np.testing.assert_allclose(a["logp"], b["logp"], rtol=1e-6, atol=1e-6)


def test_fixture_through_the_kernels(hip):
    from pasco_amd.eval import SceneEvaluator
    dev = torch.device("cuda")
    ev = SceneEvaluator(n_classes=20, thing_ids=GOLD["thing_ids"], n_outputs=NO)
    for k in range(NS):
        outs, probs = fixture_scene(k, dev)
        gt = gt_of(k, device=dev)
        assert torch.equal(gt.panoptic.cpu(), torch.from_numpy(GOLD["gt_pan"][k]))
        ev.add(outs, probs, gt)
        for got, exp in zip(ev.last_add_tables, restated_tables(k, gt_of(k))):
            assert_tables_equal(got, exp)
    check_stats(ev)
    assert ev.tables() == str(GOLD["tables"])


def _random_case(dev, grid, n_pred, n_gt, seed):
    g = torch.Generator().manual_seed(seed)
    X, Y, Z = grid
    S = X * Y * Z
    sem = torch.randint(0, 20, (S,), generator=g).to(torch.uint8)
    sem[torch.rand(S, generator=g) < 0.1] = 255
    gt_id = torch.randint(0, n_gt + 1, (S,), generator=g).to(torch.int32)
    gt_id[sem == 255] = 0
    gt_area = torch.bincount(gt_id.long(), minlength=n_gt + 1)
    gt_area[1::3] += 2                                    # whole-mask areas larger than the known count
    pan = torch.randint(0, n_pred + 1, (S,), generator=g).to(torch.int32)
    pan[torch.rand(S, generator=g) < 0.5] = 0
    pan[torch.randint(0, S, (1,), generator=g)] = n_pred
    vconf = torch.rand(S, generator=g)
    vconf[pan == 0] = 0
    return sem, gt_id, gt_area, pan, vconf


@pytest.mark.parametrize("grid,n_pred,n_gt", [((13, 7, 3), 5, 4), ((33, 31, 17), 128, 1023), ((2, 1, 1), 1, 1)])
def test_row_kernels_odd_sizes_and_bounds(hip, grid, n_pred, n_gt):
    from pasco_amd.eval.lib import ECE_COUNTS, ECE_SUMS, eval_lib
    lib = eval_lib()
    dev = torch.device("cuda")
    sem, gt_id, gt_area, pan, vconf = _random_case(dev, grid, n_pred, n_gt, seed=sum(grid))
    exp = R.panoptic_tables(pan, vconf, sem, gt_id, gt_area.numpy(), [], 20)
    site = torch.nonzero(pan != 0).reshape(-1)
    buf = torch.zeros((n_gt + 1) * (n_pred + 1) + (n_pred + 1) + (n_pred + 2) // 2 + ECE_COUNTS + ECE_SUMS + 8,
                      dtype=torch.int64, device=dev)
    b = buf.data_ptr()
    o_area, o_inter = 0, n_pred + 1
    o_map = o_inter + (n_gt + 1) * (n_pred + 1)
    o_ec = o_map + (n_pred + 2) // 2
    o_es = o_ec + ECE_COUNTS
    s_d, p_d = site.to(dev), pan[site].to(dev).contiguous()
    sem_d, gid_d, ga_d = sem.to(dev), gt_id.to(dev), gt_area.to(dev)
    lib.panop_pairs(s_d, p_d, sem_d, gid_d, n_pred, n_gt, b + 8 * o_area, b + 8 * o_inter)
    lib.match(b + 8 * o_area, ga_d, b + 8 * o_inter, n_pred, n_gt, b + 8 * o_map)
    ws = torch.empty(lib.ece_workspace_bytes(site.numel()) // 8 + 1, dtype=torch.int64, device=dev)
    lib.mask_ece(s_d, p_d, vconf[site].to(dev).contiguous(), gid_d, b + 8 * o_map, n_pred, ws, b + 8 * o_ec, b + 8 * o_es)
    h = buf.cpu().numpy()
    assert np.array_equal(h[o_area + 1:o_inter], exp["area"][1:])
    assert np.array_equal(h[o_inter:o_map].reshape(n_gt + 1, n_pred + 1)[:, 1:], exp["inter"][:, 1:])
    assert np.array_equal(h[o_map:o_ec].view(np.int32)[:n_pred + 1], exp["map"])
    assert np.array_equal(h[o_ec:o_ec + 16], exp["mask_count"]) and np.array_equal(h[o_ec + 16:o_es], exp["mask_correct"])
    R.check_conf_sums(h[o_es:o_es + ECE_SUMS].view(np.float64), exp["mask_conf_fx"], exp["mask_conf_fp64"], exp["mask_count"],
                      "mask_conf")
    # N = 0: empty tables, no launch over rows
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    lib.panop_pairs(empty, empty.to(torch.int32), sem_d, gid_d, n_pred, n_gt, b + 8 * o_area, b + 8 * o_inter)
    assert int(buf[:o_map].abs().sum()) == 0
    # one beyond either bound is refused before any launch
    with pytest.raises(RuntimeError, match="beyond"):
        lib.panop_pairs(s_d, p_d, sem_d, gid_d, 129, n_gt, b, b)
    with pytest.raises(RuntimeError, match="beyond"):
        lib.panop_pairs(s_d, p_d, sem_d, gid_d, n_pred, 1024, b, b)


def test_evaluator_refuses_too_many_gt_segments(hip):
    from pasco_amd.eval import GroundTruth, SceneEvaluator
    ins = np.arange(1, 1025, dtype=np.int64).reshape(16, 16, 4)
    sem = np.ones((16, 16, 4), np.uint8)
    gt = GroundTruth.from_labels(sem, ins, (1,), device="cuda")
    assert gt.n_gt == 1024
    outs, probs = fixture_scene(0, torch.device("cuda"))
    with pytest.raises(ValueError, match="1023"):
        SceneEvaluator(n_outputs=NO).add(outs, [torch.zeros(20, 16, 16, 4, device="cuda")] * NO, gt)


def restated_outputs(outs, sem_probs, gt_cpu):
    """The torch restatement's tables of device outputs moved to the host (dense grids rebuilt from the sparse rows)."""
    exp_tabs = []
    for i, o in enumerate(outs):
        coords, size, min_C, pan, vconf = o.sparse_rows()
        X, Y, Z = size
        c = coords[:, 1:].long().cpu() - min_C.cpu().long().reshape(1, 3)
        inside = (c >= 0).all(1) & (c[:, 0] < X) & (c[:, 1] < Y) & (c[:, 2] < Z)
        c = c[inside]
        site = (c[:, 0] * Y + c[:, 1]) * Z + c[:, 2]
        pan_d = torch.zeros(X * Y * Z, dtype=torch.int32)
        vconf_d = torch.zeros(X * Y * Z)
        pan_d[site] = pan.cpu().to(torch.int32)[inside]
        vconf_d[site] = vconf.cpu().float()[inside]
        probs = sem_probs[i].permute(1, 2, 3, 0).reshape(-1, sem_probs[i].shape[0]).cpu()
        exp_tabs.append(R.scene_tables(probs, o["ssc_confidence"].reshape(-1).cpu(), gt_cpu.semantic, pan_d, vconf_d,
                                       gt_cpu.panoptic, gt_cpu.gt_area.numpy(), o["segments_infos"][0]))
    return exp_tabs


def _s10_step():
    import bench
    from pasco_amd.graph.synth import TeacherKeep, make_scene
    dev = torch.device("cuda", 0)
    net = bench.build_net(3, 283, dev)
    sc = make_scene(seed=0, n_infers=3, in_channels=283).to(dev)
    tk = TeacherKeep(sc, dev)
    with torch.no_grad():
        x = net.prepare_input(sc.in_feats, sc.in_coords)
        ret = net(x, sc.global_min_Cs, sc.global_max_Cs, sc.min_Cs, sc.max_Cs, keep_override=tk)
        conf, sem_probs, panop = net.ensemble(ret, sc.Ts)
        outs = net.panoptic(panop, conf)
    # labels from the scene's occupancy: the ground sheet is "road", everything above it a "car" instance per 32 x 32 column
    # block (the boxes), 5 % of the sites unknown
    occ = torch.from_numpy(sc.occ)
    X, Y, Z = occ.shape
    zz = torch.arange(Z).view(1, 1, Z).expand(X, Y, Z)
    sem = torch.zeros(occ.shape, dtype=torch.uint8)
    ground = occ & (zz <= 12)
    sem[ground] = 9
    sem[occ & ~ground] = 1
    xx = torch.arange(X).view(X, 1, 1).expand(X, Y, Z)
    yy = torch.arange(Y).view(1, Y, 1).expand(X, Y, Z)
    ins = torch.where(occ & ~ground, (xx // 32) * 8 + yy // 32 + 1, torch.zeros_like(xx))
    g = torch.Generator().manual_seed(3)
    sem[torch.rand(occ.shape, generator=g) < 0.05] = 255
    return net, outs, sem_probs, sem, ins


def test_s10_mimo3_step_on_device_equals_the_restatement(hip):
    from pasco_amd.eval import GroundTruth, SceneEvaluator
    from pasco_amd.eval.lib import eval_lib
    from pasco_amd.graph.panoptic import DENSE_KEYS
    net, outs, sem_probs, sem, ins = _s10_step()
    dev = sem_probs[0].device
    gt = GroundTruth.from_labels(sem, ins, net.thing_ids, device=dev)
    ev = SceneEvaluator(n_classes=20, thing_ids=net.thing_ids, n_outputs=len(outs))
    ev.add(outs, sem_probs, gt)
    torch.cuda.synchronize()
    first = ev.last_add_tables
    # nothing dense was made for the scoring
    for o in outs:
        assert not any(dict.__contains__(o, k) for k in DENSE_KEYS + ("vox_all_mask_probs_denses",))
    # bitwise identical on a second run
    ev2 = SceneEvaluator(n_classes=20, thing_ids=net.thing_ids, n_outputs=len(outs))
    ev2.add(outs, sem_probs, gt)
    for a, b in zip(first, ev2.last_add_tables):
        for key in a:
            if key == "segments":
                assert all(np.array_equal(x["logp"], y["logp"]) for x, y in zip(a[key], b[key]))
            else:
                assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    # the same outputs moved to the host, scored by the restatement
    gt_cpu = gt.to("cpu")
    ref = SceneEvaluator(n_classes=20, thing_ids=net.thing_ids, n_outputs=len(outs))
    exp_tabs = restated_outputs(outs, sem_probs, gt_cpu)
    for got, exp in zip(first, exp_tabs):
        assert_tables_equal(got, exp)
    ref.add_tables(exp_tabs, gt_cpu)
    for a, b in zip(ev.stats(), ref.stats()):
        for key in ("precision", "recall", "iou", "iou_ssc_mean", "empty_ece", "nonempty_ece", "empty_nll", "nonempty_nll"):
            assert abs(float(a["ssc"][key]) - float(b["ssc"][key])) <= 1e-6 or (np.isnan(a["ssc"][key]) and np.isnan(b["ssc"][key])), key
        for name in ("All", "Things", "Stuff"):
            for m in ("pq_dagger", "pq", "sq", "rq", "n"):
                assert abs(float(a["pq"][name][m]) - float(b["pq"][name][m])) <= 1e-6
        for key in ("ins_ece", "ins_nll", "count", "mask_ece"):
            assert abs(float(a["uncertainty"][key]) - float(b["uncertainty"][key])) <= 1e-6, key

    # timing: pe_ssc alone (HBM-bound) and the whole add() of the scene
    lib = eval_lib()
    S = gt.semantic.numel()
    probs = sem_probs[-1].permute(1, 2, 3, 0).reshape(-1, 20)
    conf = outs[-1]["ssc_confidence"].reshape(-1).contiguous()
    ws = torch.empty(lib.ssc_workspace_bytes(S, 20) // 8 + 1, dtype=torch.int64, device=dev)
    out = torch.zeros(1024, dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        lib.ssc(probs, conf, gt.semantic, ws, out.data_ptr(), out.data_ptr() + 8 * 600)
    reps = 20
    e0.record()
    for _ in range(reps):
        lib.ssc(probs, conf, gt.semantic, ws, out.data_ptr(), out.data_ptr() + 8 * 600)
    e1.record()
    torch.cuda.synchronize()
    t_ssc = e0.elapsed_time(e1) / reps
    nbytes = S * (20 * 4 + 4 + 1)
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev2.add(outs, sem_probs, gt)
        ts.append(1e3 * (time.perf_counter() - t0))
    print(f"\n[eval] pe_ssc (S10, C=20): {t_ssc * 1e3:.1f} us per output, {nbytes / (t_ssc * 1e-3) / 1e12:.2f} TB/s "
          f"({nbytes / (t_ssc * 1e-3) / 8e12:.2f} of 8 TB/s); SceneEvaluator.add, {len(outs)} outputs: "
          f"median {np.median(ts):.2f} ms per scene")
