"""One vote of a scan -> the network's inputs: features, per-grid cells with their CSR, the 16 neighbours of every kept point and,
for every original point, its nearest kept point (`upsample`).

Reading the scan, building the input features and the test-time augmentation are numpy on the host, with the reference's
dtypes.  Everything after that runs on the device through the pw_* kernels (`prepare_device`) or through their restatement
(`prepare_host`); the two give equal integer arrays.

Test-time augmentation: the reference draws a rotation about z, a flip of x or y with probability 2/3 and a scale in
[0.9, 1.1] from torch's unseeded global generator for every vote, so there is no draw of the reference's to reproduce.  Here
the parameters are explicit (`tta_params`), drawn from `numpy.random.default_rng((seed, frame, vote))`, and, as in the
reference, applied only when more than one vote is asked for.  As there, they move the coordinate columns 0 .. 2 only: the
"xyz" copy among the features keeps the scan's own coordinates."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np

from . import host

PLANE_OF_AXIS = {0: (1, 2), 1: (0, 2), 2: (0, 1)}      # the projection along axis a keeps these two coordinates
EPS = 1e-4


def load_config(path: str) -> Dict:
    import yaml
    with open(path, "r") as f:
        cfg = yaml.safe_load(f)
    return settings(cfg)


def settings(cfg: Dict) -> Dict:
    """The fields of a WaffleIron yaml that inference reads."""
    w, e = cfg["waffleiron"], cfg["embedding"]
    fov = np.array([list(w["fov_xyz"][0]), list(w["fov_xyz"][1])])          # integers stay integers, as in the reference
    return {"fov": fov, "dim_proj": [int(d) for d in w["dim_proj"]], "grids": [tuple(int(v) for v in g) for g in w["grids_size"]],
            "input_feat": list(e["input_feat"]), "voxel_size": float(e["voxel_size"]), "neighbors": int(e["neighbors"]),
            "channels": int(w["nb_channels"]), "depth": int(w["depth"]), "classes": int(cfg["classif"]["nb_class"])}


def input_features(scan: np.ndarray, input_feat: Sequence[str]) -> np.ndarray:
    """float32 [P, 4] (x, y, z, intensity) -> float32 [P, 3 + F]: the coordinates, then the features in the config's order."""
    cols = [scan[:, :3]]
    for name in input_feat:
        if name == "intensity":
            cols.append(scan[:, 3:])
        elif name == "height":
            cols.append(scan[:, 2:3])
        elif name == "radius":
            cols.append(np.linalg.norm(scan[:, :3], axis=1, keepdims=True))
        elif name == "xyz":
            cols.append(scan[:, :3])
        else:
            raise ValueError(f"unknown input feature {name!r}")
    return np.concatenate(cols, 1)


def tta_params(seed: int, frame: int, vote: int) -> Dict:
    rng = np.random.default_rng((int(seed), int(frame), int(vote)))
    theta = float((2.0 * rng.random() - 1.0) * np.pi)
    flip = bool(rng.random() < 2.0 / 3.0)
    axis = int(rng.integers(0, 2))
    scale = float(1.0 + (2.0 * rng.random() - 1.0) * 0.1)
    return {"theta": theta, "flip": flip, "axis": axis, "scale": scale}


def augment(pc: np.ndarray, p: Optional[Dict]) -> np.ndarray:
    """Rotation about z, flip, scale on a copy of `pc` (float32 [P, 3 + F]); `p` = None: the copy unchanged."""
    pc = pc.copy()
    if p is None:
        return pc
    c, s = np.cos(p["theta"]), np.sin(p["theta"])
    rot = np.array([[c, s], [-s, c]])
    pc[:, (0, 1)] = pc[:, (0, 1)] @ rot                 # fp64 product, rounded into the fp32 columns
    if p["flip"]:
        pc[:, p["axis"]] *= -1.0
    pc[:, (0, 1, 2)] *= p["scale"]
    return pc


def _grid_geometry(cfg: Dict):
    fov = cfg["fov"]
    for dim, shape in zip(cfg["dim_proj"], cfg["grids"]):
        dims = PLANE_OF_AXIS[dim]
        res = (fov[1, dims] - fov[0, dims]) / np.array(shape)              # fp64, as the reference's
        yield dims, [float(v) for v in fov[0, dims]], [float(v) for v in res], shape


def _refuse(status: int, what: str):
    if status:
        raise ValueError(f"{what}: status {status}" + (" - a point falls off the grid" if status & host.STATUS_OFF_GRID else ""))


def prepare_host(pc: np.ndarray, cfg: Dict, search_h: float = 0.5) -> Dict:
    """`pc` float32 [P, 3 + F] (after augmentation) -> numpy arrays: feat [N, F], kept [N] (indices into pc), cells (per grid:
    cell, start, order, shape), knn [N, k], upsample [P]."""
    assert pc.dtype == np.float32
    mn = pc[:, :3].min(0)
    key, st = host.voxel_keys(pc, mn, cfg["voxel_size"])
    _refuse(st, "voxel keys")
    first = host.first_of_keys(key)
    vox = pc[first]
    keep = host.crop_mask(vox, cfg["fov"], EPS)
    kept = first[keep]
    cur = np.ascontiguousarray(pc[kept])
    k = cfg["neighbors"]
    if cur.shape[0] <= k:
        raise ValueError(f"{cur.shape[0]} points after voxelisation and crop: more than {k} are needed")
    cells = []
    for dims, lo, res, shape in _grid_geometry(cfg):
        cell, st = host.cell_index(cur, dims, lo, res, shape)
        _refuse(st, f"grid {shape}")
        start, order, st = host.cells_build(cell, shape[0] * shape[1])
        _refuse(st, f"grid {shape} CSR")
        cells.append((cell, start, order, shape))
    g = host.SearchGrid.around(cur[:, :3].min(0), cur[:, :3].max(0), search_h)
    scell, st = host.grid_cells(cur, g)
    _refuse(st, "search grid")
    sstart, sorder, st = host.cells_build(scell, g.ncell)
    _refuse(st, "search CSR")
    return {"feat": np.ascontiguousarray(cur[:, 3:]), "kept": kept.astype(np.int64), "cells": cells,
            "knn": host.knn(cur, sstart, sorder, g, k), "upsample": host.nearest(cur, sstart, sorder, g, pc), "grid": g}


def prepare_device(pc: np.ndarray, cfg: Dict, device, search_h: float = 0.5) -> Dict:
    """The same through the pw_* kernels; every array of the result is a tensor on `device`.  Two host reads: the status word
    and the kept cloud's bounding box (the search grid's extent is a host-side number)."""
    import torch
    from .lib import waffle_lib
    L = waffle_lib()
    assert pc.dtype == np.float32
    dev = torch.device(device)
    d_pc = torch.from_numpy(np.ascontiguousarray(pc)).to(dev)
    status = L.new_status(dev)
    mn = d_pc[:, :3].amin(0).contiguous()
    key = L.voxel_keys(d_pc, mn, cfg["voxel_size"], status).long()
    flat = (key[:, 0] << 42) | (key[:, 1] << 21) | key[:, 2]                # keys are below 2^21: lexicographic as one integer
    s, perm = torch.sort(flat, stable=True)
    is_first = torch.ones_like(s, dtype=torch.bool)
    is_first[1:] = s[1:] != s[:-1]
    first = perm[is_first]
    vox = d_pc[first]
    fov = cfg["fov"]
    keep = torch.ones(vox.shape[0], dtype=torch.bool, device=dev)
    for a in range(3):
        lo = torch.tensor(np.float32(fov[0][a] + EPS), device=dev)
        hi = torch.tensor(np.float32(fov[1][a] - EPS), device=dev)
        keep &= (vox[:, a] > lo) & (vox[:, a] < hi)
    kept = first[keep]
    cur = d_pc[kept].contiguous()
    k = cfg["neighbors"]
    if cur.shape[0] <= k:
        raise ValueError(f"{cur.shape[0]} points after voxelisation and crop: more than {k} are needed")
    cells = []
    for dims, lo, res, shape in _grid_geometry(cfg):
        cell = L.cell_index(cur, dims, lo, res, shape, status)
        start, order = L.cells_build(cell, shape[0] * shape[1], status)
        cells.append((cell, start, order, shape))
    box = torch.stack((cur[:, :3].amin(0), cur[:, :3].amax(0))).cpu().numpy()
    g = host.SearchGrid.around(box[0], box[1], search_h)
    scell = L.grid_cells(cur, g, status)
    sstart, sorder = L.cells_build(scell, g.ncell, status)
    knn = L.knn(cur, sstart, sorder, g, k)
    upsample = L.nearest(cur, sstart, sorder, g, d_pc)
    _refuse(int(status.item()), "preparation")
    return {"feat": cur[:, 3:].contiguous(), "kept": kept, "cells": cells, "knn": knn, "upsample": upsample, "grid": g}
