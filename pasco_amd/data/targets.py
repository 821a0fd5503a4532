"""The training batch's label targets on the device (include/pasco_target.h).

`build_train_item` (data/semantic_kitti.py) resamples both label grids into sparse samples, builds 21-channel one-hot
tensors of the scene and pools them three times per scale, all on the host.  Here the two grids go up once; `pt_resample`
writes the surviving samples of all M subnets as bytes over each subnet's box, `pt_crop_bounds` (training crop only)
reduces what the crop window keeps, and `pt_labels` writes every grid of every subnet in one launch together with the
presence tables the mask targets are made of.  Host reads per batch: the bounds, the cropped bounds when cropping, the
tables - three at most.  Everything is integer and equals the host path bit for bit (tests/test_hip_targets.py).

The masks [T, X, Y, Z] are not built unless asked for: `TargetMasks["masks"]` makes them with `pt_masks` on first access,
and `TargetMasks.pack` gives the criterion its packed words straight from the two label grids (`pt_target_pack`)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .frame_lib import box_upper_bound
from .semantic_kitti import SCALES, collate_train, completion_bounds, compute_scene_size, crop_window_from_bounds, in_window
from .target_lib import BOUNDS, CROP_BOUNDS, TABLE, target_lib

INT32_MAX = 2 ** 31 - 1


def targets_from_table(table: torch.Tensor, thing_ids):
    """One presence table (host int32 [768]) -> (labels uint8 [T], cls_slot int32 [256], ins_slot int32 [256]): the stuff
    classes present (ascending; not 0, not 255, not a thing), then the instance ids present (ascending, not 0) with the class
    at their first voxel."""
    t = table.tolist()
    labels, cls_slot, ins_slot = [], [-1] * 256, [-1] * 256
    for c in range(1, 255):
        if t[c] and c not in thing_ids:
            cls_slot[c] = len(labels)
            labels.append(c)
    for i in range(1, 256):
        if t[256 + i] != INT32_MAX:
            ins_slot[i] = len(labels)
            labels.append(t[512 + i])
    return (torch.tensor(labels, dtype=torch.uint8), torch.tensor(cls_slot, dtype=torch.int32),
            torch.tensor(ins_slot, dtype=torch.int32))


class TargetMasks(dict):
    """The reference's `mask_label` dict: `["labels"]` uint8 [T] is there from the start, `["masks"]` bool [T, X, Y, Z] is made by
    `pt_masks` on first access and is an ordinary key from then on; until then it still shows in `in`, `get`, `keys`, `items`.
    `pack(coords, unknown, origin)` gives the criterion's `PackedTargets` without the masks."""

    def __init__(self, labels: torch.Tensor, semantic: torch.Tensor, instance: torch.Tensor, cls_slot: torch.Tensor,
                 ins_slot: torch.Tensor):
        super().__init__(labels=labels)
        self._grids = (semantic, instance, cls_slot, ins_slot)

    @property
    def t(self) -> int:
        return int(dict.__getitem__(self, "labels").shape[0])

    def __missing__(self, key):
        if key != "masks":
            raise KeyError(key)
        semantic, instance, cls_slot, ins_slot = self._grids
        val = target_lib().masks(semantic, instance, cls_slot, ins_slot, self.t)
        self[key] = val
        return val

    def pack(self, coords: torch.Tensor, unknown: Optional[torch.Tensor] = None, origin=(0, 0, 0)):
        """coords int [N, 4] (column 0 ignored), unknown [X, Y, Z] | None -> `grad.criterion.PackedTargets`, bit-equal to
        `pack_targets(self["masks"], unknown, coords, origin)`."""
        from ..grad.criterion import PackedTargets, _check_counts
        t = self.t
        _check_counts(1, t)
        semantic, instance, cls_slot, ins_slot = self._grids
        dev = coords.device
        if t == 0:
            n = int(coords.shape[0])
            return PackedTargets(torch.zeros((n, 4), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev),
                                 torch.zeros(1, dtype=torch.int32, device=dev), 0)
        u = None if unknown is None else (unknown if unknown.dtype == torch.uint8 else (unknown != 0).to(torch.uint8)).contiguous()
        tbits, flags, oob = target_lib().target_pack(semantic, instance, cls_slot, ins_slot, u,
                                                     coords.to(torch.int32).contiguous(), t, [int(o) for o in origin])
        return PackedTargets(tbits, flags, oob, t)

    def _lazy_keys(self):
        return () if dict.__contains__(self, "masks") else ("masks",)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._lazy_keys()

    def get(self, key, default=None):
        return self[key] if key in self else default

    def keys(self):
        return list(dict.keys(self)) + list(self._lazy_keys())

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return dict.__len__(self) + len(self._lazy_keys())

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def __reduce__(self):          # pickling / copying: a plain dict with the masks built
        return (dict, (dict(self.items()),))


def _mask_label(table_host: torch.Tensor, semantic: torch.Tensor, instance: torch.Tensor, thing_ids) -> TargetMasks:
    labels, cls_slot, ins_slot = targets_from_table(table_host, thing_ids)
    dev = semantic.device
    return TargetMasks(labels.to(dev), semantic, instance, cls_slot.to(dev), ins_slot.to(dev))


def _union(lo_a, hi_a, lo_b, hi_b):
    """Bounds of the semantic samples with those of the instance samples, if there are any."""
    if int(lo_b.max()) == INT32_MAX:
        return lo_a.clone(), hi_a.clone()
    return torch.min(lo_a, lo_b), torch.max(hi_a, hi_b)


def prepare_targets(sem: torch.Tensor, ins: torch.Tensor, Ts: Sequence[torch.Tensor], *, thing_ids, n_classes: int = 20,
                    complete_scale: int = 8, crop_u=None, origin_masks: bool = False) -> List[Dict]:
    """sem / ins uint8 [X, Y, Z] on the device (255 = unknown / no label), one transform per subnet; `crop_u` None (the
    reference's split="val") or M x 3 numbers in [0, 1) (the training crop of each subnet).  -> one dict per subnet:
    "min_C" / "max_C" (host, as `build_train_item` makes them), "semantic_label", "instance_label", "geo_labels",
    "sem_labels", "mask_label" (a `TargetMasks`), "window" (fp64 [4] on the host or None: what `in_window` filters the point
    rows with); with `origin_masks` the first dict also carries "mask_label_origin" of the untransformed grids."""
    if complete_scale % 4 != 0:
        raise ValueError(f"prepare_targets: complete_scale {complete_scale} must be a multiple of 4")
    assert sem.is_cuda and sem.dtype == torch.uint8 and ins.dtype == torch.uint8 and sem.shape == ins.shape and sem.dim() == 3
    lib, dev, M = target_lib(), sem.device, len(Ts)
    sem, ins = sem.contiguous(), ins.contiguous()
    Ts = [torch.as_tensor(T).float().cpu() for T in Ts]
    ub = box_upper_bound(tuple(sem.shape), Ts)
    stride = int((ub[:, 3:] - ub[:, :3] + 1).long().prod(dim=1).max())
    stride = (stride + 15) // 16 * 16
    sem_box = torch.empty((M, stride), dtype=torch.uint8, device=dev)
    ins_box = torch.empty((M, stride), dtype=torch.uint8, device=dev)
    bounds = torch.empty((M, BOUNDS), dtype=torch.int32, device=dev)
    lib.resample(sem, ins, Ts, [torch.inverse(T) for T in Ts], ub, sem_box, ins_box, bounds)
    hb = bounds.cpu()                                                           # host read 1
    for m in range(M):
        if int(hb[m, 0]) == INT32_MAX or int(hb[m, 6]) == INT32_MAX:
            raise ValueError("frame has no known voxel that survives the resampling under T (the host path fails there too)")
        if bool((hb[m, 0:3] < ub[m, 0:3]).any()) or bool((hb[m, 3:6] > ub[m, 3:6]).any()):
            raise RuntimeError(f"prepare_targets: the sample box of subnet {m} {hb[m, :6].tolist()} leaves its host-side bound "
                               f"{ub[m].tolist()}")
    windows = None
    sem_lo, sem_hi, ins_lo, ins_hi = hb[:, 6:9], hb[:, 9:12], hb[:, 12:15], hb[:, 15:18]
    if crop_u is not None:
        crop_u = np.asarray(crop_u, dtype=np.float64).reshape(M, 3)
        windows = torch.stack([crop_window_from_bounds(sem_lo[m], sem_hi[m], crop_u[m]) for m in range(M)])
        cb = torch.empty((M, CROP_BOUNDS), dtype=torch.int32, device=dev)
        lib.crop_bounds(sem_box, ins_box, ub, windows, cb)
        hc = cb.cpu()                                                           # host read 2
        sem_lo, sem_hi, ins_lo, ins_hi = hc[:, 0:3], hc[:, 3:6], hc[:, 6:9], hc[:, 9:12]
        if int(sem_lo.max()) == INT32_MAX:
            raise ValueError("the training crop keeps no semantic sample (the host path fails there too)")
    outs, items = [], []
    for m in range(M):
        lo, hi = _union(sem_lo[m], sem_hi[m], ins_lo[m], ins_hi[m])
        min_c, max_c = completion_bounds(lo, hi, complete_scale)
        scene = [int(v) for v in compute_scene_size(min_c, max_c, scale=complete_scale)]
        n1 = scene[0] * scene[1] * scene[2]
        buf = torch.empty(3 * n1 + 2 * (n1 // 8) + 2 * (n1 // 64), dtype=torch.uint8, device=dev)    # one allocation per subnet
        cut = [n1, n1, n1, n1 // 8, n1 // 8, n1 // 64, n1 // 64]
        parts = torch.split(buf, cut)
        shape = lambda s: (scene[0] // s, scene[1] // s, scene[2] // s)
        o = {"semantic": parts[0].view(shape(1)), "instance": parts[1].view(shape(1)), "geo_1": parts[2].view(shape(1)),
             "geo_2": parts[3].view(shape(2)), "sem_2": parts[4].view(shape(2)), "geo_4": parts[5].view(shape(4)),
             "sem_4": parts[6].view(shape(4)), "min_C": min_c.tolist(), "scene": scene}
        outs.append(o)
        items.append({"min_C": min_c, "max_C": max_c, "semantic_label": o["semantic"], "instance_label": o["instance"],
                      "geo_labels": {"1_1": o["geo_1"], "1_2": o["geo_2"], "1_4": o["geo_4"]},
                      "sem_labels": {"1_1": o["semantic"], "1_2": o["sem_2"], "1_4": o["sem_4"]},
                      "window": None if windows is None else windows[m]})
    tables = torch.empty((M + 1, TABLE), dtype=torch.int32, device=dev)
    lib.labels(sem_box, ins_box, ub, windows, outs, n_classes, tables)
    if origin_masks:
        lib.presence(sem, ins, tables[M])
    ht = tables.cpu() if origin_masks else tables[:M].cpu()                    # host read 3
    for m in range(M):
        items[m]["mask_label"] = _mask_label(ht[m], outs[m]["semantic"], outs[m]["instance"], thing_ids)
    if origin_masks:
        items[0]["mask_label_origin"] = _mask_label(ht[M], sem, ins, thing_ids)
    return items


def assemble_train_batch(base: Dict, sem: torch.Tensor, ins: torch.Tensor, *, thing_ids, n_classes: int = 20,
                         complete_scale: int = 8, crop_u=None, frame_id=None, sequence=None) -> Dict:
    """`base`: the inference batch of `device_prep.prepare` (its tensors on the device of sem / ins).  -> the dict
    `collate_train` returns: the point rows of each subnet filtered by its crop window, the bounds of what the crop keeps,
    and the targets of `prepare_targets`."""
    Ts = base["Ts"]
    tg = prepare_targets(sem, ins, Ts, thing_ids=thing_ids, n_classes=n_classes, complete_scale=complete_scale, crop_u=crop_u,
                         origin_masks=True)
    items = []
    for m, t in enumerate(tg):
        feat, coord = base["in_feats"][m], base["in_coords"][m]
        if t["window"] is not None:
            keep = in_window(coord, t["window"])
            feat, coord = feat[keep], coord[keep]
        items.append({"in_feat": feat, "in_coord": coord, "T": Ts[m], "min_C": t["min_C"], "max_C": t["max_C"],
                      "xyz": base["xyz"][m], "input_pcd_instance_label": base["input_pcd_instance_label"][m],
                      "frame_id": frame_id, "sequence": sequence, "semantic_label": t["semantic_label"],
                      "instance_label": t["instance_label"], "geo_labels": t["geo_labels"], "sem_labels": t["sem_labels"],
                      "mask_label": t["mask_label"], "semantic_label_origin": sem, "instance_label_origin": ins,
                      "mask_label_origin": tg[0]["mask_label_origin"]})
    return collate_train(items, complete_scale)


assert SCALES == (1, 2, 4)      # pt_labels writes exactly these
