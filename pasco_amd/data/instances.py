"""Panoptic instance labels from the ground-truth completion grid: what `instance_labels_v2/<seq>/<frame>_1_1.pkl` holds.

Restates the reference's generator (label_gen/gen_instance_labels.py:77-122 and its KITTI-360 twin; lookup table
pasco/data/semantic_kitti/io_data.py:174-194).  Input: a semantic grid L[X, Y, Z] (0 = empty, 1..C-1 classes, 255 =
unknown), the thing ids, min_size = 8.  With site index x*Y*Z + y*Z + z:

  1. for each t in thing_ids, in list order, the voxels with L == t split into 26-connected components;
  2. components are ordered by (position of their class in thing_ids, smallest site index of the component);
  3. a component of fewer than min_size voxels is dropped: instance 0 and semantic 255 on its voxels;
  4. the survivors are numbered 1..n in that order; every other voxel has instance 0 and keeps its semantic value.

The reference reaches the same grids with a raster scan and a voxel-by-voxel flood fill per class.  Two corners of that
program are not reproduced: it applies the size rule to the background id 0 as well, and it numbers from 0 when no voxel
at all has instance 0.  Neither occurs on a real frame.

`device=None` runs the numpy restatement below; a GPU device runs the pl_* kernels (include/pasco_label.h), equal in every
integer.  Pickles are Python pickles: load them only from sources you trust."""
from __future__ import annotations

import os
import pickle
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

KITTI_GRID = (256, 256, 32)
MIN_SIZE = 8

# the 13 neighbour offsets that come earlier in site order (the other 13 are their negatives)
_BACK = [(dx, dy, dz) for dx in (-1, 0) for dy in (-1, 0, 1) for dz in (-1, 0, 1)
         if (dx, dy, dz) < (0, 0, 0)]


def _on_gpu(device) -> bool:
    return device is not None and torch.device(device).type == "cuda"


# ---- SemanticKITTI: raw voxel labels -> semantic grid ----------------------------------------------------------------
def remap_lut(config_path: str) -> np.ndarray:
    """`learning_map` of a SemanticKITTI yaml -> uint8 lookup table (io_data.py:174-194): length max key + 100, every 0
    entry becomes 255 (unknown), then entry 0 is set back to 0 (empty)."""
    import yaml
    with open(config_path) as f:
        learning_map = yaml.safe_load(f)["learning_map"]
    keys = np.array(list(learning_map.keys()), dtype=np.int64)
    vals = np.array(list(learning_map.values()), dtype=np.int64)
    if keys.min() < 0 or vals.min() < 0 or vals.max() > 255:
        raise ValueError(f"{config_path}: learning_map keys must be >= 0 and values must fit uint8")
    lut = np.zeros(int(keys.max()) + 100, dtype=np.int64)
    lut[keys] = vals
    lut[lut == 0] = 255
    lut[0] = 0
    return lut.astype(np.uint8)


def read_raw_voxels(label_path: str, invalid_path: str) -> Tuple[np.ndarray, np.ndarray]:
    """voxels/<frame>.label (uint16 per voxel) and voxels/<frame>.invalid (bit-packed) as stored."""
    return np.fromfile(label_path, dtype=np.uint16), np.fromfile(invalid_path, dtype=np.uint8)


def semantic_grid_from_raw(raw: np.ndarray, invalid_bits: np.ndarray, lut: np.ndarray, grid=KITTI_GRID, device=None):
    """raw uint16 [S], packed invalid bits uint8 [S / 8] -> semantic uint8 [X, Y, Z]: lut[raw], 255 where the invalid bit
    (most significant first) is set (gen_instance_labels.py:77-86).  numpy on the host, a device tensor on a GPU."""
    S = int(np.prod(grid))
    if raw.size != S or invalid_bits.size * 8 != S:
        raise ValueError(f"grid {tuple(grid)} has {S} voxels; got {raw.size} labels and {invalid_bits.size} mask bytes")
    if _on_gpu(device):
        from .label_lib import label_lib, STATUS_RAW_RANGE
        dev = torch.device(device)
        sem, status = label_lib().semantic_grid(torch.from_numpy(np.ascontiguousarray(raw)).to(dev),
                                                torch.from_numpy(np.ascontiguousarray(invalid_bits)).to(dev),
                                                torch.from_numpy(np.ascontiguousarray(lut, dtype=np.uint8)).to(dev))
        if int(status.item()) & STATUS_RAW_RANGE:
            raise ValueError(f"a raw label is outside the lookup table of {lut.size} entries")
        return sem.reshape(tuple(grid))
    if raw.size and int(raw.max()) >= lut.size:
        raise ValueError(f"a raw label is outside the lookup table of {lut.size} entries")
    sem = np.asarray(lut, dtype=np.uint8)[raw]
    sem[np.unpackbits(invalid_bits) == 1] = 255
    return sem.reshape(tuple(grid))


def semantic_grid(label_path: str, invalid_path: str, lut: np.ndarray, device=None, grid=KITTI_GRID):
    raw, inv = read_raw_voxels(label_path, invalid_path)
    return semantic_grid_from_raw(raw, inv, lut, grid, device)


# ---- connected components on the host ---------------------------------------------------------------------------------
def _roots_scipy(sem: np.ndarray, thing_ids: Sequence[int], ndimage):
    """-> (site, root, class position) of every thing voxel; root = smallest site of the voxel's component."""
    sites, roots, cpos = [], [], []
    structure = np.ones((3, 3, 3), dtype=bool)
    for p, t in enumerate(thing_ids):
        lab, n = ndimage.label(sem == t, structure=structure)
        if n == 0:
            continue
        flat = lab.ravel()
        site = np.flatnonzero(flat)
        comp = flat[site]
        first = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(first, comp, site)      # site is ascending, so this is the first raster site of each component
        sites.append(site)
        roots.append(first[comp])
        cpos.append(np.full(site.size, p, dtype=np.int64))
    if not sites:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    return np.concatenate(sites), np.concatenate(roots), np.concatenate(cpos)


def _roots_numpy(sem: np.ndarray, thing_ids: Sequence[int]):
    """The same without scipy: edges between equal thing voxels over the 13 earlier neighbours, then rounds of "hang the
    larger root under the smaller" and pointer jumping until no edge joins two roots."""
    X, Y, Z = sem.shape
    pos = np.full(256, -1, dtype=np.int64)
    for p, t in enumerate(thing_ids):
        pos[int(t)] = p
    cls = pos[sem]
    site = np.flatnonzero(cls.ravel() >= 0)
    if site.size == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    compact = np.full(sem.size, -1, dtype=np.int64)
    compact[site] = np.arange(site.size)
    compact = compact.reshape(sem.shape)
    us, vs = [], []
    for dx, dy, dz in _BACK:
        def span(d, n):
            return (slice(max(0, -d), n - max(0, d)), slice(max(0, d), n - max(0, -d)))
        (ax, bx), (ay, by), (az, bz) = span(dx, X), span(dy, Y), span(dz, Z)
        a, b = cls[ax, ay, az], cls[bx, by, bz]           # b is a's neighbour at (dx, dy, dz)
        m = (a >= 0) & (a == b)
        us.append(compact[ax, ay, az][m])
        vs.append(compact[bx, by, bz][m])
    u, v = np.concatenate(us), np.concatenate(vs)
    parent = np.arange(site.size)
    while True:
        pu, pv = parent[u], parent[v]
        diff = pu != pv
        if not diff.any():
            break
        u, v = u[diff], v[diff]
        np.minimum.at(parent, np.maximum(pu[diff], pv[diff]), np.minimum(pu[diff], pv[diff]))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return site, site[parent], cls.ravel()[site]


def _have_scipy():
    try:
        from scipy import ndimage
        return ndimage
    except Exception:
        return None


def instance_labels_host(sem: np.ndarray, thing_ids: Sequence[int], min_size: int = MIN_SIZE, use_scipy: Optional[bool] = None):
    """The four rules of the module header in numpy -> (instance int32 grid, semantic uint8 grid, info).  scipy's
    `ndimage.label` does the components when it imports (`use_scipy=False` forces the plain numpy form; both agree)."""
    sem = np.ascontiguousarray(sem, dtype=np.uint8)
    if sem.ndim != 3:
        raise ValueError("semantic grid must be [X, Y, Z]")
    ids = _check_things(thing_ids)
    ndimage = _have_scipy() if use_scipy in (None, True) else None
    if use_scipy and ndimage is None:
        raise RuntimeError("scipy does not import")
    site, root, cpos = _roots_scipy(sem, ids, ndimage) if ndimage is not None else _roots_numpy(sem, ids)
    instance = np.zeros(sem.size, dtype=np.int32)
    out = sem.reshape(-1).copy()
    comp_root, inverse, count = np.unique(root, return_inverse=True, return_counts=True)
    comp_cls = np.zeros(comp_root.size, dtype=np.int64)
    comp_cls[inverse] = cpos
    order = np.lexsort((comp_root, comp_cls))                # by class position, then by smallest site
    keep = count[order] >= min_size
    new_id = np.zeros(comp_root.size, dtype=np.int32)
    new_id[order[keep]] = np.arange(1, int(keep.sum()) + 1, dtype=np.int32)
    vox_id = new_id[inverse]
    instance[site] = vox_id
    out[site[vox_id == 0]] = 255
    sizes = count[order[keep]].astype(np.int32)
    info = _info(int(keep.sum()), int((~keep).sum()), int(count[order[~keep]].sum()), sizes)
    return instance.reshape(sem.shape), out.reshape(sem.shape), info


def _check_things(thing_ids: Sequence[int]):
    ids = [int(t) for t in thing_ids]
    if len(ids) > 32 or len(set(ids)) != len(ids) or any(t < 1 or t > 254 for t in ids):
        raise ValueError(f"thing ids {ids}: up to 32 distinct values in 1..254")
    return ids


def _info(n: int, dropped: int, unknown: int, sizes) -> Dict:
    """`over_uint8`: both readers of the pickle cast the instance grid to uint8 (kitti_dataset.py:329-339), so ids above
    255 wrap there; that is the reference's limit and is only recorded here."""
    return {"n_instances": n, "n_dropped": dropped, "n_unknown": unknown, "sizes": sizes, "over_uint8": n > 255}


def instance_labels(sem, thing_ids: Sequence[int], min_size: int = MIN_SIZE, device=None):
    """-> (instance int32 [X, Y, Z], semantic uint8 [X, Y, Z], info).  `device=None` (or a CPU device): numpy arrays from
    the host restatement.  A GPU device: device tensors from the pl_* kernels; `sem` may already be a tensor there.  `info`
    holds n_instances, n_dropped, n_unknown, sizes (voxels of instance i at [i - 1]) and over_uint8."""
    if not _on_gpu(device):
        if isinstance(sem, torch.Tensor):
            sem = sem.cpu().numpy()
        return instance_labels_host(sem, thing_ids, min_size)
    from .label_lib import label_lib, REC_DROPPED, REC_INSTANCES, REC_STATUS, REC_UNKNOWN
    ids = _check_things(thing_ids)
    dev = torch.device(device)
    if not isinstance(sem, torch.Tensor):
        sem = torch.from_numpy(np.ascontiguousarray(sem, dtype=np.uint8))
    sem = sem.to(dev).contiguous()
    cap = sem.numel() // max(int(min_size), 1) + 1
    ins, out, rec, sizes = label_lib().instances(sem, ids, min_size, sizes_cap=cap)
    r = rec.cpu().tolist()
    if r[REC_STATUS] != 0:
        raise RuntimeError(f"pl_instances: status {r[REC_STATUS]} (a union loop hit its cap)")
    return ins, out, _info(r[REC_INSTANCES], r[REC_DROPPED], r[REC_UNKNOWN], sizes[:r[REC_INSTANCES]])


# ---- the pickle ------------------------------------------------------------------------------------------------------
def write_instance_pickle(path: str, instance, semantic, semantic_dtype=np.float32) -> None:
    """The reference's file: `instance_labels` float64 and `semantic_labels` [X, Y, Z] (float32 for SemanticKITTI, the dtype
    of the source .npy for KITTI-360: the reference copies the grid it read).  Written to a temporary name first."""
    def host(a):
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    data = {"instance_labels": host(instance).astype(np.float64),
            "semantic_labels": host(semantic).astype(semantic_dtype)}
    tmp = f"{path}.tmp{os.getpid()}"
    with open(tmp, "wb") as f:
        pickle.dump(data, f)
    os.replace(tmp, path)


def as_label_pair(instance, semantic) -> Tuple[np.ndarray, np.ndarray]:
    """What `read_instance_label_pickle` returns for the file `write_instance_pickle` would write: (semantic uint8, instance
    uint8) on the host."""
    def host(a):
        return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return host(semantic).astype(np.uint8), host(instance).astype(np.float64).astype(np.uint8)
