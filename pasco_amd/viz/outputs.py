"""Saved frame outputs: `<dir>/<frame>_<i>.pkl`, one per output of a step (the subnets, then the ensemble), with the keys and
shapes the reference's own saving script writes, so that its drawing script - and `python -m pasco_amd.viz` - can read them."""
from __future__ import annotations

import os
import pickle
from typing import Sequence

import numpy as np

KEYS = ("ssc_pred", "pred_panoptic_seg", "pred_segments_info", "vox_confidence_denses", "instance_confidence_denses", "xyz",
        "gt_panoptic_seg", "gt_segments_info", "semantic_label_origin", "instance_label_origin")


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else v


def frame_record(ssc_pred, panoptic, segments_info: Sequence[dict], vox_confidence, instance_confidence, xyz, gt_panoptic,
                 gt_segments_info: Sequence[dict], semantic_label, instance_label) -> dict:
    """Grids are [X, Y, Z] (tensors or arrays).  Shapes written: ssc_pred int64 [1, X, Y, Z]; pred_panoptic_seg int32
    [1, X, Y, Z]; pred_segments_info [list of dict] (one scene); both confidences fp32 [1, X, Y, Z]; xyz fp32 [P, 3];
    gt_panoptic_seg int32 [X, Y, Z]; the label grids as given."""
    grid = lambda v, dt: np.ascontiguousarray(_host(v)).astype(dt)
    infos = [{k: _host(v) for k, v in s.items()} for s in segments_info]
    return {
        "ssc_pred": grid(ssc_pred, np.int64)[None],
        "pred_panoptic_seg": grid(panoptic, np.int32)[None],
        "pred_segments_info": [infos],
        "vox_confidence_denses": grid(vox_confidence, np.float32)[None],
        "instance_confidence_denses": grid(instance_confidence, np.float32)[None],
        "xyz": np.zeros((0, 3), np.float32) if xyz is None else grid(xyz, np.float32),
        "gt_panoptic_seg": grid(gt_panoptic, np.int32),
        "gt_segments_info": [dict(s) for s in gt_segments_info],
        "semantic_label_origin": np.ascontiguousarray(_host(semantic_label)),
        "instance_label_origin": np.ascontiguousarray(_host(instance_label)),
    }


def write_record(directory: str, frame: str, i: int, record: dict) -> str:
    assert tuple(record) == KEYS
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"{frame}_{i}.pkl")
    with open(path, "wb") as f:
        pickle.dump(record, f)
    return path


def save_step_outputs(directory: str, frame: str, outs, sem_probs, gt, semantic_label, instance_label, xyz=None):
    """Every output of one `step_inference` (`outs`, `sem_probs` as `SceneEvaluator.add` takes them, `gt` the frame's
    `GroundTruth`) -> its pickle.  Returns the paths."""
    shape = tuple(int(v) for v in sem_probs[0].shape[1:])
    gt_infos = [{"id": int(i), "isthing": bool(t), "category_id": int(c), "area": int(a)}
                for i, t, c, a in zip(gt.seg_id, gt.seg_thing, gt.seg_cat, gt.seg_area)]
    paths = []
    for i, (out, probs) in enumerate(zip(outs, sem_probs)):
        conf = out["ssc_confidence"] if "ssc_confidence" in out else out["vox_confidence_denses"][0]
        rec = frame_record(probs.argmax(dim=0), out["panoptic_seg_denses"][0].reshape(shape), out["segments_infos"][0],
                           conf.reshape(shape), out["ins_uncertainty_denses"][0].reshape(shape), xyz,
                           gt.panoptic.reshape(shape), gt_infos, semantic_label, instance_label)
        paths.append(write_record(directory, frame, i, rec))
    return paths
