"""Ground truth of one scene for the panoptic metrics: the reference builds it with `KittiDataset.prepare_mask_label`
(kitti_dataset.py:594-664, one [K, X, Y, Z] boolean mask per stuff class and per instance) and
`convert_mask_label_to_panoptic_output` (panoptic_quality.py:365-390, a Python walk that paints the masks in order).
Here the same id grid and segment table come from a few vectorised passes over the grid."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import numpy as np
import torch

UNKNOWN = 255


@dataclass
class GroundTruth:
    semantic: torch.Tensor      # [S] uint8, 255 = unknown
    panoptic: torch.Tensor      # [S] int32 segment id, 0 at unknown sites and where no segment is
    seg_id: np.ndarray          # [K] int64, ascending - segments present after the unknown zeroing
    seg_cat: np.ndarray         # [K] int64
    seg_thing: np.ndarray       # [K] bool
    seg_area: np.ndarray        # [K] int64: voxels of the mask that opened the segment (unknown ones included)
    gt_area: torch.Tensor       # [G + 1] int64 by id (0 for absent ids), on the device of the grids
    shape: tuple
    max_label: int = -1         # largest semantic label other than 255 (-1: every site unknown)

    @property
    def n_gt(self) -> int:
        """Largest segment id (G)."""
        return int(self.gt_area.numel()) - 1

    @classmethod
    def from_labels(cls, semantic, instance, thing_ids: Sequence[int], device=None) -> "GroundTruth":
        """`semantic` / `instance`: the origin grids of one frame ([X, Y, Z], as `read_instance_label_pickle` returns them).

        Segments are made as the reference makes them: stuff classes in ascending order, then instance ids in ascending
        order; an instance takes the class of its first voxel in flat order; class 0 is skipped; an instance of a stuff
        class paints over that class's segment instead of opening one; later masks overwrite earlier ones.  The area of a
        segment is the count of the mask that opened it - not recounted after overwrites or the unknown zeroing - and
        segments with no voxel left after the zeroing are dropped."""
        sem = torch.as_tensor(np.asarray(semantic) if not torch.is_tensor(semantic) else semantic)
        ins = torch.as_tensor(np.asarray(instance) if not torch.is_tensor(instance) else instance)
        shape = tuple(sem.shape)
        if tuple(ins.shape) != shape:
            raise ValueError(f"semantic grid {shape} and instance grid {tuple(ins.shape)} differ")
        dev = torch.device(device) if device is not None else sem.device
        sem = sem.to(dev).reshape(-1).to(torch.uint8)
        ins = ins.to(dev).reshape(-1).to(torch.int64)
        if int(ins.min()) < 0 if ins.numel() else False:
            raise ValueError("negative instance id")
        S = sem.numel()
        things = set(int(t) for t in thing_ids)
        sem_l = sem.to(torch.int64)
        # per-class and per-instance voxel counts, first voxel of every instance: one pass each
        cls_count = torch.bincount(sem_l, minlength=256)
        n_ins = int(ins.max()) + 1 if S else 1
        ins_count = torch.bincount(ins, minlength=n_ins)
        first = torch.full((n_ins,), S, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, ins, torch.arange(S, device=dev), reduce="amin")
        host = torch.cat([cls_count, ins_count]).cpu().numpy()
        cls_count_h, ins_count_h = host[:256], host[256:]
        ins_ids = np.flatnonzero(ins_count_h)
        ins_ids = ins_ids[ins_ids != 0]
        ins_cat = sem_l[first[torch.as_tensor(ins_ids, device=dev)]].cpu().numpy() if ins_ids.size else np.zeros(0, np.int64)

        # segment ids in the reference's order (tables of at most 256 + n_instance entries: host)
        stuff = [c for c in np.flatnonzero(cls_count_h) if c not in (0, UNKNOWN) and int(c) not in things]
        lut_cls = np.zeros(256, np.int64)          # stuff class -> segment id
        lut_ins = np.zeros(n_ins, np.int64)        # instance id -> segment id it paints (0 = none)
        ids, cats, isthing, areas = [], [], [], []
        memory = {}
        for c in stuff:
            ids.append(len(ids) + 1)
            cats.append(int(c)); isthing.append(False); areas.append(int(cls_count_h[c]))
            memory[int(c)] = ids[-1]
            lut_cls[c] = ids[-1]
        for i, c in zip(ins_ids.tolist(), ins_cat.tolist()):
            if c == 0:
                continue
            th = c in things
            if not th and c in memory:
                lut_ins[i] = memory[c]
                continue
            ids.append(len(ids) + 1)
            cats.append(int(c)); isthing.append(th); areas.append(int(ins_count_h[i]))
            if not th:
                memory[c] = ids[-1]
            lut_ins[i] = ids[-1]
        lut_cls_t = torch.as_tensor(lut_cls, device=dev)
        lut_ins_t = torch.as_tensor(lut_ins, device=dev)
        by_ins = lut_ins_t[ins]
        pan = torch.where(by_ins != 0, by_ins, lut_cls_t[sem_l])
        pan = torch.where(sem == UNKNOWN, torch.zeros_like(pan), pan).to(torch.int32)
        n_ids = len(ids)
        present = torch.bincount(pan.to(torch.int64), minlength=n_ids + 1).cpu().numpy()[1:] > 0 if n_ids else np.zeros(0, bool)
        ids_a = np.asarray(ids, np.int64)
        gt_area = np.zeros(n_ids + 1, np.int64)
        gt_area[ids_a[present]] = np.asarray(areas, np.int64)[present]
        labels = np.flatnonzero(cls_count_h[:UNKNOWN])
        return cls(semantic=sem, panoptic=pan, seg_id=ids_a[present], seg_cat=np.asarray(cats, np.int64)[present],
                   seg_thing=np.asarray(isthing, bool)[present], seg_area=np.asarray(areas, np.int64)[present],
                   gt_area=torch.as_tensor(gt_area, device=dev), shape=shape,
                   max_label=int(labels[-1]) if labels.size else -1)

    def to(self, device) -> "GroundTruth":
        return GroundTruth(self.semantic.to(device), self.panoptic.to(device), self.seg_id, self.seg_cat, self.seg_thing,
                           self.seg_area, self.gt_area.to(device), self.shape, self.max_label)
