"""Evaluation layer on the host (pasco_amd/eval): the torch restatement and SceneEvaluator's bookkeeping against the
reference's own scoring (tests/golden/eval.npz, tests/golden/make_golden_eval.py), GroundTruth, merging, the pe_ ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import eval_restate as R  # noqa: E402

ROOT = os.path.dirname(HERE)
GOLD = np.load(os.path.join(HERE, "golden", "eval.npz"))
NS, NO = int(GOLD["n_scenes"]), int(GOLD["n_out"])
GRID = tuple(int(v) for v in GOLD["grid"])


def gt_of(k, device="cpu"):
    from pasco_amd.eval import GroundTruth
    return GroundTruth.from_labels(GOLD["in_sem"][k].reshape(GRID), GOLD["in_ins"][k].reshape(GRID), GOLD["thing_ids"],
                                   device=device)


def infos_of(k, o):
    return [{"id": int(s[0]), "isthing": bool(s[2]), "category_id": int(s[1]), "confidence": float(GOLD["in_seg_conf"][k, o][j]),
             "all_class_probs": torch.from_numpy(GOLD["in_seg_probs"][k, o][j])}
            for j, s in enumerate(GOLD["in_seg"][k, o]) if s[0] >= 0]


def restated_tables(k, gt):
    return [R.scene_tables(torch.from_numpy(GOLD["in_prob"][k, o]), torch.from_numpy(GOLD["in_conf"][k, o]),
                           torch.from_numpy(GOLD["in_sem"][k]), torch.from_numpy(GOLD["in_pan"][k, o]),
                           torch.from_numpy(GOLD["in_vconf"][k, o]), gt.panoptic.cpu(), gt.gt_area.cpu().numpy(), infos_of(k, o))
            for o in range(NO)]


def check_stats(ev, tol=1e-6):
    """Every statistic of `ev` against the reference's (NaN where the reference has NaN)."""
    st = ev.stats()
    close = lambda a, b: (np.isnan(b) and np.isnan(a)) or abs(float(a) - float(b)) <= tol
    for o in range(NO):
        s = st[o]
        for key in ("precision", "recall", "iou", "iou_ssc_mean", "empty_ece", "nonempty_ece", "empty_nll", "nonempty_nll"):
            assert close(s["ssc"][key], float(GOLD[f"o{o}_ssc_{key}"])), (o, key, s["ssc"][key])
        np.testing.assert_allclose(s["ssc"]["iou_ssc"], GOLD[f"o{o}_ssc_iou_ssc"], atol=tol)
        for name in ("All", "Things", "Stuff"):
            got = [float(s["pq"][name][m]) for m in ("pq_dagger", "pq", "sq", "rq", "n")]
            np.testing.assert_allclose(got, GOLD[f"o{o}_pq_{name}"], atol=tol, err_msg=f"{o} {name}")
        pc = GOLD[f"o{o}_pq_per_class"]
        assert sorted(s["pq"]["per_class"]) == [c for c in range(pc.shape[0]) if pc[c, 0]]
        for c, v in s["pq"]["per_class"].items():
            np.testing.assert_allclose([float(v[m]) for m in ("pq", "sq", "rq")], pc[c, 1:], atol=tol)
        u = s["uncertainty"]
        np.testing.assert_allclose([float(u[k]) for k in ("ins_ece", "ins_nll", "count", "mask_ece")], GOLD[f"o{o}_unc"],
                                   atol=tol)


def restated_evaluator(scenes=range(NS)):
    from pasco_amd.eval import SceneEvaluator
    ev = SceneEvaluator(n_classes=20, thing_ids=GOLD["thing_ids"], n_outputs=NO)
    for k in scenes:
        gt = gt_of(k)
        ev.add_tables(restated_tables(k, gt), gt)
    return ev


def test_ground_truth_matches_the_reference():
    """prepare_mask_label + convert_mask_label_to_panoptic_output, then the unknown zeroing: id grid and segment table
    (stuff first, an instance whose first voxel is stuff merged into that stuff, a class-0 instance skipped, whole-mask
    areas)."""
    for k in range(NS):
        gt = gt_of(k)
        assert torch.equal(gt.panoptic, torch.from_numpy(GOLD["gt_pan"][k])), k
        seg = GOLD["gt_seg"][k]
        seg = seg[seg[:, 0] >= 0]
        assert np.array_equal(gt.seg_id, seg[:, 0]) and np.array_equal(gt.seg_cat, seg[:, 1])
        assert np.array_equal(gt.seg_thing.astype(np.int64), seg[:, 2]) and np.array_equal(gt.seg_area, seg[:, 3])


def test_restatement_reproduces_the_reference_counts():
    ev = restated_evaluator()
    for o in range(NO):
        a = ev.out[o]
        assert np.array_equal(a.tps, GOLD[f"o{o}_acc_tps"]) and np.array_equal(a.fps, GOLD[f"o{o}_acc_fps"])
        assert np.array_equal(a.fns, GOLD[f"o{o}_acc_fns"])
        assert np.array_equal(a.compl, GOLD[f"o{o}_acc_compl"])
        assert np.array_equal(a.n_vox, GOLD[f"o{o}_acc_nvox"])
        cats = GOLD[f"o{o}_pq_cats"].tolist()
        assert sorted(a.pq) == cats
        got = np.array([[a.pq[c].tp, a.pq[c].fp, a.pq[c].fn, a.pq[c].all_n] for c in cats], np.float64)
        assert np.array_equal(got, GOLD[f"o{o}_pq_tpfpfn"])


def test_host_finish_reproduces_every_stat_and_the_table_text():
    ev = restated_evaluator()
    check_stats(ev)
    assert ev.tables() == str(GOLD["tables"])
    # the fixture holds the cases it promises
    assert np.isnan(ev.stats()[1]["ssc"]["empty_ece"])                       # an empty pred == 0 group
    assert (GOLD["in_seg"][1, 2][:, 0] < 0).all()                             # an output without segments


def test_iou_of_exactly_one_half_is_not_a_match():
    gt = gt_of(0)
    t = restated_tables(0, gt)[0]
    g = int(gt.panoptic[-4])                                                  # the 2-voxel instance
    p = int(GOLD["in_pan"][0, 0][-1])                                         # the 4-voxel segment over it
    assert t["inter"][g, p] == 2 and t["area"][p] == 4 and gt.gt_area[g] == 2
    assert t["map"][p] == 0


def test_merged_evaluators_equal_one_evaluator():
    a = restated_evaluator(range(0, 2))
    b = restated_evaluator(range(2, NS))
    a += b
    assert a.scenes == NS
    check_stats(a)
    assert a.tables() == str(GOLD["tables"])


def test_step_time_fills_the_inference_time_column():
    ev = restated_evaluator(range(1))
    line = ev.tables(step_time=21.5).strip().splitlines()[-1]
    assert line.startswith("ensemble,") and line.endswith(", 21.50")


def _exports(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path], text=True)
    return {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW"}


def test_library_exports_exactly_the_eval_header():
    from pasco_amd.build import CSRC, build_hip
    src = open(os.path.join(ROOT, "include", "pasco_eval.h")).read()
    declared = {"pe_" + n for n in re.findall(r"PE_FN\((\w+)\)\s*\(", src)}
    assert {"pe_ssc", "pe_panop_pairs", "pe_match", "pe_mask_ece", "pe_abi_version"} <= declared
    lib = build_hip(verbose=False)
    assert {s for s in _exports(lib) if s.startswith("pe_")} == declared
    h = ctypes.CDLL(lib)
    h.pe_abi_version.restype = ctypes.c_int
    from pasco_amd.eval.lib import PE_ABI_VERSION
    assert h.pe_abi_version() == PE_ABI_VERSION == 1
    assert "getenv(" not in open(os.path.join(CSRC, "eval.hip")).read()
    from pasco_amd.me import backend
    assert not any(k in backend._SIGNATURES for k in ("ssc", "panop_pairs", "match", "mask_ece"))


def test_evaluator_refuses_bounds_it_cannot_hold():
    from pasco_amd.eval import GroundTruth, SceneEvaluator
    sem = np.zeros((4, 4, 2), np.uint8)
    ins = np.zeros((4, 4, 2), np.uint8)
    gt = GroundTruth.from_labels(sem, ins, (1,))
    ev = SceneEvaluator(n_outputs=2)
    with pytest.raises(ValueError):
        ev.add([None], [torch.zeros(20, 4, 4, 2)], gt)
