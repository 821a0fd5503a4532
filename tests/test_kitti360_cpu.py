"""KITTI-360 data layer on the host: the restatement against the reference's own `Kitti360Dataset`
(tests/golden/kitti360_items.npz, tests/golden/make_golden_kitti360.py), the match file and frame listing, a
`Net_kitti360`-shaped checkpoint with thing ids 1..6, and the mini frame through the graph on the CPU oracle."""
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
MINI = os.path.join(GOLD, "kitti360_mini")
SEQ, FRAME = "2013_05_28_drive_0009_sync", "000042"


def gold():
    return np.load(os.path.join(GOLD, "kitti360_items.npz"))


def reader():
    from pasco_amd.data import Kitti360FrameReader
    return Kitti360FrameReader(MINI, os.path.join(MINI, "preprocess"), os.path.join(MINI, "sscbench"),
                               os.path.join(MINI, "match.txt"))


def test_host_restatement_equals_the_reference_bit_for_bit():
    """Identity, the eval table's transforms and a flipped rigid one: features, coordinates, bounds, xyz."""
    g = gold()
    r = reader()
    tags = [str(t) for t in g["tags"]]
    assert {"eye", "table1", "table2", "rigid"} <= set(tags)
    for tag in tags:
        b = r.batch(SEQ, FRAME, [torch.from_numpy(g[f"{tag}_T"])])
        assert b["in_feats"][0].dtype == torch.float32 and b["in_feats"][0].shape[1] == 8
        assert torch.equal(b["in_feats"][0], torch.from_numpy(g[f"{tag}_in_feat"])), tag
        assert torch.equal(b["in_coords"][0], torch.from_numpy(g[f"{tag}_in_coord"])), tag
        assert torch.equal(b["min_Cs"][0], torch.from_numpy(g[f"{tag}_min_C"])), tag
        assert torch.equal(b["max_Cs"][0], torch.from_numpy(g[f"{tag}_max_C"])), tag
        assert np.array_equal(b["xyz"][0], g[f"{tag}_xyz"]), tag


def test_crop_keeps_the_reference_precisions():
    """Lower bound compared in fp64, upper bound in fp32: a point 1 fp32 ulp below y = -25.6 in fp32 but above the fp64
    bound is the case where the two differ."""
    from pasco_amd.data.kitti360 import build_item_kitti360
    sem = np.zeros((8, 8, 8), np.uint8)
    ins = np.zeros_like(sem)
    y = np.float32(-25.6)                           # fp32(-25.6) < -25.6 (fp64): dropped by the fp64 comparison
    hi = np.nextafter(np.float32(51.2), np.float32(0))
    pc = np.array([[1.0, y, 0.0, 0.5], [1.0, np.nextafter(y, np.float32(0)), 0.0, 0.5], [hi, 0.0, 0.0, 0.5],
                   [np.float32(51.2), 0.0, 0.0, 0.5]], np.float32)
    it = build_item_kitti360(pc, sem, ins)
    assert it["in_feat"].shape[0] == 2
    assert float(it["in_feat"][0, 6]) == float(np.nextafter(y, np.float32(0))) and float(it["in_feat"][1, 5]) == float(hi)


def test_match_file_and_frame_listing():
    from pasco_amd.data import read_match_file
    m = read_match_file(os.path.join(MINI, "match.txt"))
    assert m[SEQ][FRAME] == "0000000137" and m["2013_05_28_drive_0000_sync"]["000000"] == "0000000009"
    r = reader()
    assert r.frames("test") == [(SEQ, FRAME)] and r.frames("val") == []
    with pytest.raises(ValueError):
        r.frames("train")
    lab, pc = r.paths(SEQ, FRAME)
    assert pc.endswith(os.path.join("velodyne_points", "data", "0000000137.bin")) and os.path.exists(pc)
    sem, ins = r.labels(SEQ, FRAME)
    assert sem.dtype == np.uint8 and sem.shape == (64, 64, 16) and ins.shape == sem.shape


def kitti360_checkpoint(path):
    """A Lightning-layout checkpoint with the state-dict keys and shapes of a reduced reference `Net_kitti360`."""
    k = np.load(os.path.join(GOLD, "kitti360_net_keys.npz"))
    n_classes, n_infers, in_ch, f, nq = (int(v) for v in k["hyper"])
    g = torch.Generator().manual_seed(360)
    sd = {}
    tp = {}
    for key, shp, dt in zip(k["keys"], k["shapes"], k["dtypes"]):
        shape = [int(s) for s in shp if s >= 0]
        dtype = getattr(torch, str(dt))
        tail = key.split("transformer_predictor.", 1)[-1] if "transformer_predictor." in key else None
        if tail is not None and tail in tp:
            sd[str(key)] = tp[tail]
            continue
        if dtype.is_floating_point:
            v = torch.randn(shape, generator=g) * 0.1
            if key.endswith("running_var"):
                v = v.abs() + 0.5
        else:
            v = torch.zeros(shape, dtype=dtype)
        sd[str(key)] = v.to(dtype)
        if tail is not None:
            tp[tail] = sd[str(key)]
    torch.save({"state_dict": sd, "hyper_parameters": {"n_classes": n_classes, "n_infers": n_infers, "in_channels": in_ch,
                                                       "f": f, "num_queries": nq, "heavy_decoder": False}}, path)
    return path


def test_kitti360_checkpoint_loads_with_its_thing_ids(tmp_path):
    from pasco_amd.data import net_from_checkpoint
    from pasco_amd.data.kitti360 import THING_IDS
    p = kitti360_checkpoint(os.path.join(tmp_path, "k360.ckpt"))
    net = net_from_checkpoint(p, thing_ids=THING_IDS)
    assert net.thing_ids == (1, 2, 3, 4, 5, 6) and net.n_classes == 19 and net.feat.PPmodel[1].in_features == 8
    # the default stays SemanticKITTI's, and an override in **kwargs is no longer the only (dropped) way in
    assert net_from_checkpoint(p).thing_ids == (1, 2, 3, 4, 5, 6, 7, 8)


def test_mini_frame_runs_through_the_graph_and_scores_with_19_names(tmp_path, oracle_registered):
    from pasco_amd.data import net_from_checkpoint
    from pasco_amd.data.kitti360 import CLASS_NAMES, THING_IDS
    from pasco_amd.eval import SceneEvaluator
    from pasco_amd.eval.kitti import subnet_transforms
    net = net_from_checkpoint(kitti360_checkpoint(os.path.join(tmp_path, "k360.ckpt")), thing_ids=THING_IDS)
    b = reader().batch(SEQ, FRAME, subnet_transforms(net.n_infers))
    ext = (b["global_max_Cs"] - b["global_min_Cs"] + 1).tolist()
    net.ensembler.scene_size = tuple(int(v) for v in ext)
    with torch.no_grad():
        x = net.prepare_input(b["in_feats"], b["in_coords"])
        ret = net(x, b["global_min_Cs"], b["global_max_Cs"], b["min_Cs"], b["max_Cs"])
    assert len(ret["panop_predictions"]) == 2 and ret["sem_logits_at_scales"][1][0].F.shape[1] == 19
    ev = SceneEvaluator(n_classes=19, thing_ids=THING_IDS, n_outputs=3, class_names=CLASS_NAMES)
    assert ev.class_names[7:9] == ("road", "parking") and len(ev.class_names) == 19


def test_eval_cli_parses_the_kitti360_arguments():
    import pasco_amd.eval.kitti360 as E
    with pytest.raises(SystemExit):
        E.main(["--help"])
    assert "--device-prep" in open(os.path.join(os.path.dirname(HERE), "pasco_amd", "eval", "kitti.py")).read()
