"""SSCBench-KITTI-360 / PaSCo on-disk formats -> the a0 input contract of the inference path.

Restates, for inference only, what the reference's KITTI-360 data layer does (no augmentation sampling, no label
pyramids, one scan per frame: n_fuse_scans = 1; the caller passes the rigid transform T of each subnet):

  frame list          pasco/data/kitti360/kitti360_dataset.py:66-100 (splits; frames from <label_root>/labels/<seq>/*_1_1.npy)
  match file          kitti360_dataset.py:585-614 (`sequence raw_id sscbench_id` per line, extensions dropped)
  velodyne points     kitti360_dataset.py:287-288 (float32 x, y, z, intensity; no WaffleIron embedding)
  instance labels     kitti360_dataset.py:279-284 (the pickle `read_instance_label_pickle` reads)
  frame -> item       kitti360_dataset.py:289-370 (extent crop, radius, voxelise, transform) and :108-175 (min_C / max_C)

Features are [intensity, radius, dx, dy, dz, x, y, z] (8 channels).  Two precisions differ from SemanticKITTI and are kept:
the crop's lower bound is an fp64 array (fp64 comparison under NumPy >= 2) while its upper bound is a tuple of Python floats
(fp32 comparison), and the voxel centre is computed in fp64 (`astype(float)`).

`Kitti360FrameReader.batch(..., device=None)` runs this host restatement; with a GPU device it runs the `pf_*` kernels
(`data.device_prep`), bit-equal.  Pickles are Python pickles: load them only from sources you trust."""
from __future__ import annotations

import glob
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .semantic_kitti import collate, read_instance_label_pickle, transform_coords, transformed_labels

VOX_ORIGIN = np.array([0, -25.6, -2])
VOXEL_SIZE = 0.2
MAX_EXTENT = (51.2, 25.6, 4.4)                 # a tuple of Python floats: compared in fp32
MIN_EXTENT = np.array([0, -25.6, -2.0])        # an fp64 array: compared in fp64
N_CLASSES = 19
THING_IDS = (1, 2, 3, 4, 5, 6)                 # pasco/data/kitti360/params.py
CLASS_NAMES = ("empty", "car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "road", "parking", "sidewalk",
               "other-ground", "building", "fence", "vegetation", "terrain", "pole", "traffic-sign", "other-structure",
               "other-object")
IN_CHANNELS = 8
SPLITS = {"val": ("2013_05_28_drive_0006_sync",), "test": ("2013_05_28_drive_0009_sync",)}


def read_match_file(path: str) -> Dict[str, Dict[str, str]]:
    """-> {sequence: {sscbench frame id: raw velodyne id}} (lines `sequence raw_id[.ext] sscbench_id[.ext]`; other lines
    are skipped, as the reference does)."""
    out: Dict[str, Dict[str, str]] = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if len(parts) != 3:
                continue
            seq, raw, ssc = parts
            out.setdefault(seq, {})[ssc.rsplit(".", 1)[0]] = raw.rsplit(".", 1)[0]
    return out


def read_velodyne(path: str) -> np.ndarray:
    """data_3d_raw/<seq>/velodyne_points/data/<raw>.bin -> float32 [N, 4] = x, y, z, intensity."""
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)


def build_item_kitti360(pc: np.ndarray, semantic_label: np.ndarray, instance_label: np.ndarray,
                        T: Optional[torch.Tensor] = None, complete_scale: int = 8) -> Dict:
    """The inference-side fields of `Kitti360Dataset.get_individual` for one subnet: point features [P, 8], integer voxel
    coordinates under T, the transform and the completion bounds min_C / max_C."""
    T = torch.eye(4) if T is None else T
    xyz, intensity = pc[:, :3], pc[:, 3:]
    keep = ((xyz[:, 0] < MAX_EXTENT[0]) & (xyz[:, 0] >= MIN_EXTENT[0]) & (xyz[:, 1] < MAX_EXTENT[1])
            & (xyz[:, 1] >= MIN_EXTENT[1]) & (xyz[:, 2] < MAX_EXTENT[2]) & (xyz[:, 2] >= MIN_EXTENT[2]))
    xyz, intensity = xyz[keep], intensity[keep]
    *_, min_c, max_c = transformed_labels(semantic_label, instance_label, T, complete_scale)
    radius = np.linalg.norm(xyz, axis=1)[..., np.newaxis]
    feat = np.concatenate((intensity, radius), axis=1)
    origin = VOX_ORIGIN.reshape(1, 3)
    coords = (xyz - origin) // VOXEL_SIZE
    centres = (coords.astype(float) + 0.5) * VOXEL_SIZE + origin
    return_xyz = np.concatenate((xyz - centres, xyz), axis=1)
    in_feat = torch.from_numpy(np.concatenate([feat, return_xyz], axis=1)).float()
    in_coord = transform_coords(torch.from_numpy(coords), T).long()
    return {"in_feat": in_feat, "in_coord": in_coord, "T": T, "min_C": min_c, "max_C": max_c, "xyz": xyz - origin,
            "input_pcd_instance_label": None}


def prepare_kitti360_on_device(pc: np.ndarray, semantic_label: np.ndarray, instance_label: np.ndarray,
                               Ts: Sequence[torch.Tensor], device, complete_scale: int = 8) -> Dict:
    """`collate([build_item_kitti360(...) for T in Ts])` through the pf_* kernels on `device`."""
    from . import device_prep as DP
    from .frame_lib import _seg
    pts = DP.upload(np.ascontiguousarray(pc, dtype=np.float32), device)
    sem, ins = DP.upload(semantic_label, device), DP.upload(instance_label, device)
    return DP.prepare(pts, sem, ins, Ts, lo=MIN_EXTENT, hi=MAX_EXTENT, lo_fp64=(1, 1, 1), hi_fp64=(0, 0, 0),
                      origin=VOX_ORIGIN, voxel=VOXEL_SIZE, centre_fp64=True, pre=[_seg(pts[:, 3:], 1, 4, 1)],
                      complete_scale=complete_scale)


class Kitti360FrameReader:
    """Directory layout of the reference's KITTI-360 setup:
        <root>/data_3d_raw/<seq>/velodyne_points/data/<raw_id:010d>.bin
        <preprocess_root>/instance_labels_v2/<seq>/<frame>_1_1.pkl
        <label_root>/labels/<seq>/<frame>_1_1.npy            (only listed: it names the labelled frames)
    and the match file `sequence raw_id sscbench_id`, whose path the caller passes.  `batch(seq, frame, Ts)` returns the
    collated a0 contract for len(Ts) subnets, each fed the same frame under its own transform."""

    def __init__(self, root: str, preprocess_root: str, label_root: str, match_file: str, complete_scale: int = 8,
                 instances: str = "file", label_device="cuda"):
        """`instances="file"` reads the label grids from the instance pickle; `"device"` builds them from
        `<label_root>/labels/<seq>/<frame>_1_1.npy` with the pl_* kernels on `label_device` (`data.instances`)."""
        if instances not in ("file", "device"):
            raise ValueError(f"instances={instances!r}: 'file' or 'device'")
        self.root, self.preprocess_root, self.label_root = root, preprocess_root, label_root
        self.complete_scale = complete_scale
        self.instances, self.label_device, self._last = instances, label_device, (None, None)
        self.match = read_match_file(match_file)

    def frames(self, split: str) -> List[tuple]:
        """-> [(sequence, frame id)] of a split, sorted."""
        if split not in SPLITS:
            raise ValueError(f"split {split!r}: one of {sorted(SPLITS)}")
        out = []
        for seq in SPLITS[split]:
            names = glob.glob(os.path.join(self.label_root, "labels", seq, "*_1_1.npy"))
            out += [(seq, fid) for fid in sorted(os.path.splitext(os.path.basename(p))[0][:6] for p in names)]
        return out

    def paths(self, sequence: str, frame_id: str):
        raw = self.match[sequence][frame_id]
        return (os.path.join(self.preprocess_root, "instance_labels_v2", sequence, f"{frame_id}_1_1.pkl"),
                os.path.join(self.root, "data_3d_raw", sequence, "velodyne_points", "data", f"{int(raw):010d}.bin"))

    def labels(self, sequence: str, frame_id: str):
        """The frame's origin label grids (semantic uint8, 255 = unknown; instance ids) for `GroundTruth.from_labels`."""
        if self.instances == "device":
            from . import instances as I
            if self._last[0] != (sequence, frame_id):       # labels() and batch() of one frame share one run
                grid = np.load(os.path.join(self.label_root, "labels", sequence, f"{frame_id}_1_1.npy")).astype(np.uint8)
                ins, sem, _ = I.instance_labels(grid, THING_IDS, I.MIN_SIZE, self.label_device)
                self._last = ((sequence, frame_id), I.as_label_pair(ins, sem))
            return self._last[1]
        return read_instance_label_pickle(self.paths(sequence, frame_id)[0])

    def batch(self, sequence: str, frame_id: str, Ts: Sequence[torch.Tensor], device=None) -> Dict:
        _, pcp = self.paths(sequence, frame_id)
        sem, ins = self.labels(sequence, frame_id)
        pc = read_velodyne(pcp)
        if device is not None and torch.device(device).type == "cuda":
            return prepare_kitti360_on_device(pc, sem, ins, Ts, device, self.complete_scale)
        return collate([build_item_kitti360(pc, sem, ins, T, self.complete_scale) for T in Ts], self.complete_scale)
