"""SemanticKITTI / PaSCo on-disk formats -> the a0 input contract of the inference path.

Restates, file format by file format, what the reference's data layer reads, and the training-side targets it builds from
them (`build_train_item`; the caller passes the transform T of each subnet and the crop's draw - `data.augment` samples T):

  bit-packed voxel grids   pasco/data/semantic_kitti/io_data.py:11-24 (unpack), :35-45 (pack),
                           :114-138 (.bin occupancy, .label uint16, .invalid / .occluded)
  velodyne points          io_data.py:146-150 (float32 x, y, z, remission)
  per-point labels         pasco/data/semantic_kitti/kitti_dataset.py:318-328 (int32, low 16 bits = class)
  WaffleIron features      kitti_dataset.py:290-303 (pickle: embedding [E, 256, P], coords [P, 4], vote [P, V])
  instance labels          kitti_dataset.py:329-339 (pickle: semantic_labels / instance_labels uint8 grids)
  frame -> subnet item     kitti_dataset.py:339-455 (extent crop, radius, voxelise, transform) and :150-175
                           (min_C floored to the completion scale, max_C)
  items -> batch           pasco/data/semantic_kitti/collate.py:76-105 (global bounds rounded up to the scale)
  training targets         kitti_dataset.py:142-288 (dense grids, multi-scale labels), :463-490 (crop), :594-664 (mask targets)
  rigid transforms         pasco/models/transform_utils.py:60-74 (`transform`), :123-161 (`transform_scene`)

Pickles are Python pickles: load them only from sources you trust (the reference's own preprocessing output).
"""
from __future__ import annotations

import os
import pickle
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

VOX_ORIGIN = np.array([0.0, -25.6, -2.0])
VOXEL_SIZE = 0.2
MAX_EXTENT = (51.2, 25.6, 4.4)          # kitti_dataset.py:58 (sic: 4.4, not 4.0)
MIN_EXTENT = (0.0, -25.6, -2.0)


# ---- bit-packed voxel files ---------------------------------------------------------------------------
def unpack_bits(compressed: np.ndarray) -> np.ndarray:
    """uint8 [n] -> uint8 [8 n] of 0 / 1, most significant bit first (io_data.py:11-24)."""
    return np.unpackbits(np.ascontiguousarray(compressed, dtype=np.uint8))


def pack_bits(array: np.ndarray) -> np.ndarray:
    """0 / 1 array -> bitwise uint8, most significant bit first (io_data.py:35-45); the size must divide by 8."""
    flat = np.asarray(array).reshape(-1)
    if flat.size % 8 != 0:
        raise ValueError("pack_bits: number of voxels must be a multiple of 8")
    return np.packbits(flat.astype(bool).astype(np.uint8))


def _read(path: str, dtype, do_unpack: bool) -> np.ndarray:
    raw = np.fromfile(path, dtype=dtype)
    return unpack_bits(raw) if do_unpack else raw


def read_occupancy(path: str) -> np.ndarray:
    """voxels/*.bin: bit-packed occupancy -> float32 [X*Y*Z] (io_data.py:136-138)."""
    return _read(path, np.uint8, True).astype(np.float32)


def read_label(path: str) -> np.ndarray:
    """voxels/*.label: uint16 per voxel -> float32 (io_data.py:121-123)."""
    return _read(path, np.uint16, False).astype(np.float32)


def read_invalid(path: str) -> np.ndarray:
    """voxels/*.invalid: bit-packed mask -> uint8 (io_data.py:126-128)."""
    return _read(path, np.uint8, True)


def read_occluded(path: str) -> np.ndarray:
    """voxels/*.occluded: bit-packed mask -> uint8 (io_data.py:131-133)."""
    return _read(path, np.uint8, True)


def read_pointcloud(path: str) -> np.ndarray:
    """velodyne/*.bin -> float32 [N, 4] = x, y, z, remission (io_data.py:146-150)."""
    return _read(path, np.float32, False).reshape(-1, 4)


def read_point_instance_labels(path: str) -> np.ndarray:
    """labels/*.label: int32 per point, low 16 bits kept -> int32 [N, 1] (kitti_dataset.py:318-328)."""
    return (np.fromfile(path, dtype=np.int32).reshape(-1, 1) & 0xFFFF)


# ---- pickles ---------------------------------------------------------------------------------------------
def read_waffleiron_features(path: str, embedding_index: Optional[int] = None,
                             rng: Optional[np.random.Generator] = None):
    """seg_feats_tta/*.pkl -> (xyz [P,3], vote [P,V], intensity [P,1], embedding [P,256]) (kitti_dataset.py:290-303).
    The file holds E test-time-augmented embeddings; the reference draws one at random per call - pass
    `embedding_index` for a reproducible choice, or an `rng`.  `path` may be the already loaded dictionary (the three
    arrays computed by `pasco_amd.waffle.Extractor` instead of read from a file)."""
    data = path if isinstance(path, dict) else _load_pickle(path)
    emb = data["embedding"]
    if embedding_index is None:
        embedding_index = int((rng or np.random.default_rng()).integers(0, emb.shape[0]))
    embedding = emb[embedding_index].T
    xyz_density = data["coords"]
    return xyz_density[:, :3], data["vote"], xyz_density[:, 3:], embedding


def _load_pickle(path: str):
    with open(path, "rb") as f:
        return pickle.load(f)


def read_instance_label_pickle(path: str):
    """instance_labels_v2/<seq>/<frame>_1_<down>.pkl -> (semantic uint8 grid, instance uint8 grid)
    (kitti_dataset.py:329-339)."""
    with open(path, "rb") as f:
        data = pickle.load(f)
    return data["semantic_labels"].astype(np.uint8), data["instance_labels"].astype(np.uint8)


# ---- rigid transforms on the voxel lattice --------------------------------------------------------------
def transform_coords(coords: torch.Tensor, T: torch.Tensor, resolution: float = 0.2) -> torch.Tensor:
    """Voxel indices -> metres (voxel centres) -> T -> voxel indices, rounded to nearest even like torch.round
    (transform_utils.py:60-74).  Returns int32."""
    min_bound = torch.tensor([0, -25.6, -2]).reshape(1, 3).to(coords.device)
    pts = coords * resolution + resolution / 2
    pts = min_bound + pts
    hom = torch.cat([pts, torch.ones(pts.shape[0], 1, device=pts.device)], dim=1).type_as(T)
    new = (T @ hom.T).T[:, :3]
    new = (new - min_bound - resolution / 2) / resolution
    return torch.round(new).int()


def transform_scene(from_coords: torch.Tensor, T: torch.Tensor, voxel_features: torch.Tensor, to_coords_bnd=None):
    """Resample a labelled grid under T without holes (transform_utils.py:123-161): the bounding box of the
    transformed coordinates is sampled densely, every sample is projected back with T^-1 and reads the source
    voxel it lands in (zero outside).  The reference does the read with `grid_sample(mode="nearest",
    align_corners=True)` on integer coordinates, which is plain indexing - done here as such.
    voxel_features [F, H, W, D] -> (features [N, F], coords int32 [N, 3], (min, max))."""
    if to_coords_bnd is None:
        to = transform_coords(from_coords, T)
        to_coords_bnd = (to.min(0)[0], to.max(0)[0])
    mn, mx = to_coords_bnd
    size = (mx - mn + 1).tolist()
    # the reference enumerates np.meshgrid(x, y, z) with the default 'xy' indexing: y outermost, then x, then z
    gx, gy, gz = np.meshgrid(np.arange(size[0]), np.arange(size[1]), np.arange(size[2]))
    grid = torch.from_numpy(np.stack([gx.ravel(), gy.ravel(), gz.ravel()], axis=1).astype(float)).type_as(from_coords)
    to_coords = grid + mn.reshape(1, 3)
    back = transform_coords(to_coords, torch.inverse(T)).long()
    Fch, H, W, D = voxel_features.shape
    ok = (back[:, 0] >= 0) & (back[:, 0] < H) & (back[:, 1] >= 0) & (back[:, 1] < W) & (back[:, 2] >= 0) & (back[:, 2] < D)
    out = torch.zeros((back.shape[0], Fch), dtype=torch.float32)
    b = back[ok]
    out[ok] = voxel_features[:, b[:, 0], b[:, 1], b[:, 2]].T.float()
    return out, to_coords.int(), to_coords_bnd


def compute_scene_size(min_c: torch.Tensor, max_c: torch.Tensor, scale: int = 1) -> torch.Tensor:
    """pasco/models/misc.py:30-32."""
    return (torch.ceil((max_c - min_c + 1) / scale) * scale).int()


# ---- one frame -> one subnet item ---------------------------------------------------------------------------
def completion_bounds(min_c: torch.Tensor, max_c: torch.Tensor, complete_scale: int = 8):
    """min_C floored to the completion scale, max_C as it is (kitti_dataset.py:150-175)."""
    return (torch.floor(min_c.float() / complete_scale) * complete_scale).int(), torch.ceil(max_c)


def transformed_labels(semantic_label: np.ndarray, instance_label: np.ndarray, T: torch.Tensor, complete_scale: int = 8):
    """The label grids resampled under T (kitti_dataset.py:373-395) and the completion bounds taken from them:
    -> (sem_sparse, sem_coords, ins_sparse, ins_coords, min_C, max_C).  `ins + 1` is uint8 arithmetic, so every sample
    that lands on an instance id other than 255 survives the `!= 0` filter, id 0 included."""
    sem = torch.from_numpy(semantic_label)
    sem_coords = torch.nonzero(sem != 255)
    sem_sparse, sem_coords, bnd = transform_scene(sem_coords, T, sem.unsqueeze(0) + 1)
    nz = sem_sparse.sum(dim=1) != 0
    sem_sparse, sem_coords = sem_sparse[nz] - 1, sem_coords[nz]
    ins = torch.from_numpy(instance_label)
    ins_coords = torch.nonzero(ins)
    if ins_coords.shape[0] > 0:
        ins_sparse, ins_coords, _ = transform_scene(ins_coords, T, ins.unsqueeze(0) + 1, to_coords_bnd=bnd)
    else:
        ins_sparse, ins_coords = torch.zeros((0, 1)), torch.zeros((0, 3)).long()
    nz = ins_sparse.sum(dim=1) != 0
    ins_sparse, ins_coords = ins_sparse[nz] - 1, ins_coords[nz]
    min_c, max_c = sem_coords.min(dim=0)[0], sem_coords.max(dim=0)[0]
    if ins_coords.shape[0] > 0:
        min_c = torch.min(min_c, ins_coords.min(dim=0)[0])
        max_c = torch.max(max_c, ins_coords.max(dim=0)[0])
    min_c, max_c = completion_bounds(min_c, max_c, complete_scale)
    return sem_sparse, sem_coords, ins_sparse, ins_coords, min_c, max_c


def build_item(xyz: np.ndarray, vote: np.ndarray, intensity: np.ndarray, embedding: np.ndarray,
               semantic_label: np.ndarray, instance_label: np.ndarray, T: Optional[torch.Tensor] = None,
               complete_scale: int = 8, point_labels: Optional[np.ndarray] = None) -> Dict:
    """The inference-side fields of `KittiDataset.get_individual` (kitti_dataset.py:339-455,150-175) for one
    subnet: point features [P, V + 1 + 1 + 256 + 6] (votes, intensity, radius, embedding, offset to the voxel
    centre, xyz), integer voxel coordinates under T, the transform, and the completion bounds min_C / max_C taken
    from the transformed label grids."""
    T = torch.eye(4) if T is None else T
    keep = ((xyz[:, 0] < MAX_EXTENT[0]) & (xyz[:, 0] >= MIN_EXTENT[0]) & (xyz[:, 1] < MAX_EXTENT[1])
            & (xyz[:, 1] >= MIN_EXTENT[1]) & (xyz[:, 2] < MAX_EXTENT[2]) & (xyz[:, 2] >= MIN_EXTENT[2]))
    xyz = xyz[keep]
    vote_intensity = np.concatenate((vote, intensity), axis=1)[keep]
    embedding = embedding[keep]
    if point_labels is not None:
        point_labels = point_labels[keep]

    sem_sparse, sem_coords, ins_sparse, ins_coords, min_c, max_c = transformed_labels(semantic_label, instance_label, T,
                                                                                      complete_scale)

    radius = np.linalg.norm(xyz, axis=1)[..., np.newaxis]
    feat = np.concatenate((vote_intensity, radius, embedding), axis=1)
    origin = VOX_ORIGIN.reshape(1, 3)
    coords = (xyz - origin) // VOXEL_SIZE
    centres = (coords.astype(np.float32) + 0.5) * VOXEL_SIZE + origin
    return_xyz = np.concatenate((xyz - centres, xyz), axis=1)
    in_feat = torch.from_numpy(np.concatenate([feat, return_xyz], axis=1)).float()
    in_coord = transform_coords(torch.from_numpy(coords), T).long()

    return {"in_feat": in_feat, "in_coord": in_coord, "T": T, "min_C": min_c, "max_C": max_c,
            "xyz": xyz - origin, "semantic_label_sparse": (sem_sparse.to(torch.uint8), sem_coords),
            "instance_label_sparse": (ins_sparse.to(torch.uint8), ins_coords),
            "input_pcd_instance_label": None if point_labels is None else torch.from_numpy(point_labels)}


def collate(items: Sequence[Dict], complete_scale: int = 8) -> Dict:
    """Subnet items -> the batch `Net.step_inference` consumes (collate.py:76-105): per-subnet lists plus the global
    bounds, the extent rounded up to a multiple of the completion scale."""
    min_cs = [it["min_C"] for it in items]
    max_cs = [it["max_C"] for it in items]
    gmin = torch.min(torch.stack(min_cs), dim=0)[0]
    gmax = torch.max(torch.stack(max_cs), dim=0)[0]
    gmax = gmin + compute_scene_size(gmin, gmax, scale=complete_scale) - 1     # inclusive
    return {"in_feats": [it["in_feat"] for it in items], "in_coords": [it["in_coord"] for it in items],
            "Ts": [it["T"] for it in items], "min_Cs": min_cs, "max_Cs": max_cs,
            "global_min_Cs": gmin, "global_max_Cs": gmax, "xyz": [it["xyz"] for it in items],
            "input_pcd_instance_label": [it.get("input_pcd_instance_label") for it in items]}


# ---- the training-side targets (host restatement; the device path is data/targets.py) ---------------------
SCALES = (1, 2, 4)
SEMANTIC_KITTI_THING_IDS = (1, 2, 3, 4, 5, 6, 7, 8)


def crop_window_from_bounds(lo: torch.Tensor, hi: torch.Tensor, u) -> torch.Tensor:
    """The training crop's window (kitti_dataset.py:463-471) from the bounds of the semantic samples -> fp64 [4] = (min x,
    max x, min y, max y); a coordinate c is kept iff min <= c < max.  The dtypes are those of the reference's expression: the
    0.8 extent and the slack are fp32 (an int32 tensor times a Python float), the product with `u` and everything after it
    fp64.  `u`: three numbers in [0, 1); z is not cropped."""
    lo, hi = lo.int(), hi.int()
    size = (hi - lo) * 0.8
    new_lo = lo + (hi - lo - size) * torch.as_tensor(np.asarray(u, dtype=np.float64).reshape(3))
    new_hi = new_lo + size
    return torch.stack([new_lo[0], new_hi[0], new_lo[1], new_hi[1]]).double()


def crop_window(sem_coords: torch.Tensor, u) -> torch.Tensor:
    return crop_window_from_bounds(sem_coords.min(dim=0)[0], sem_coords.max(dim=0)[0], u)


def in_window(coords: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    w = window.to(coords.device)
    return (coords[:, 0] >= w[0]) & (coords[:, 0] < w[1]) & (coords[:, 1] >= w[2]) & (coords[:, 1] < w[3])


def dense_labels(sem_sparse, sem_coords, ins_sparse, ins_coords, min_c, scene_size):
    """The sparse samples written into grids of origin min_C (kitti_dataset.py:179-198): semantic filled with 255,
    instance with 0."""
    shape = [int(v) for v in scene_size]
    sem = torch.full(shape, 255, dtype=torch.uint8)
    c = (sem_coords - min_c).long()
    sem[c[:, 0], c[:, 1], c[:, 2]] = sem_sparse.reshape(-1).to(torch.uint8)
    ins = torch.zeros(shape, dtype=torch.uint8)
    if ins_coords.shape[0] > 0:
        c = (ins_coords - min_c).long()
        ins[c[:, 0], c[:, 1], c[:, 2]] = ins_sparse.reshape(-1).to(torch.uint8)
    return sem, ins


def _blocks(grid: torch.Tensor, s: int) -> torch.Tensor:
    X, Y, Z = grid.shape
    return grid.reshape(X // s, s, Y // s, s, Z // s, s).permute(0, 2, 4, 1, 3, 5).reshape(X // s, Y // s, Z // s, s ** 3)


def multiscale_labels(semantic_label: torch.Tensor, n_classes: int = 20):
    """geo_labels / sem_labels at scales 1, 2, 4 (kitti_dataset.py:205-266) as integer rules over the s^3 blocks, equal to
    the reference's one-hot poolings:
      sem  the most frequent class of 1..n_classes-1 in the block (lowest index on a tie); without any, 0 if ALL voxels are
           255, else 255 (sic: a block of empties, or of empties and unknowns, reads 255)
      geo  255 if all voxels are 255, else 1 if any is in 1..254, else 0"""
    sem = semantic_label
    geo1 = torch.where(sem == 255, sem, (sem > 0).to(torch.uint8))
    geo, lab = {"1_1": geo1}, {"1_1": sem}
    for s in SCALES[1:]:
        b = _blocks(sem, s)
        counts = torch.stack([(b == c).sum(dim=-1) for c in range(1, n_classes)], dim=-1)
        best = counts.argmax(dim=-1) + 1
        any_class = counts.max(dim=-1)[0] > 0
        all_unknown = (b == 255).all(dim=-1)
        lab[f"1_{s}"] = torch.where(any_class, best, torch.where(all_unknown, 0, 255)).to(torch.uint8)
        occupied = ((b > 0) & (b < 255)).any(dim=-1)
        geo[f"1_{s}"] = torch.where(all_unknown, 255, occupied.long()).to(torch.uint8)
    return geo, lab


def mask_targets(semantic_label: torch.Tensor, instance_label: torch.Tensor, thing_ids=SEMANTIC_KITTI_THING_IDS):
    """`prepare_mask_label` (kitti_dataset.py:594-664): the stuff classes present (ascending; not 0, not 255, not a thing),
    then one entry per instance id present (ascending, not 0) whose class is the semantic label at the instance's first voxel
    in row-major order.  -> {"labels": uint8 [T], "masks": bool [T, X, Y, Z]}.  Edge: a frame with no entry gives T = 0
    (labels [0], masks [0, X, Y, Z]) where the reference's `torch.stack([])` raises."""
    sem, ins = semantic_label, instance_label
    labels, masks = [], []
    for c in torch.unique(sem).tolist():
        if c not in (0, 255) and c not in thing_ids:
            labels.append(c)
            masks.append(sem == c)
    for i in torch.unique(ins).tolist():
        if i != 0:
            m = ins == i
            labels.append(int(sem[m][0]))
            masks.append(m)
    if not masks:
        return {"labels": torch.zeros(0, dtype=torch.uint8), "masks": torch.zeros((0,) + tuple(sem.shape), dtype=torch.bool)}
    return {"labels": torch.tensor(labels, dtype=torch.uint8), "masks": torch.stack(masks)}


def build_train_item(xyz: np.ndarray, vote: np.ndarray, intensity: np.ndarray, embedding: np.ndarray,
                     semantic_label: np.ndarray, instance_label: np.ndarray, T: Optional[torch.Tensor] = None,
                     complete_scale: int = 8, point_labels: Optional[np.ndarray] = None, *, crop_u=None,
                     thing_ids=SEMANTIC_KITTI_THING_IDS, n_classes: int = 20, frame_id: Optional[str] = None,
                     sequence: Optional[str] = None) -> Dict:
    """The whole of `KittiDataset.get_individual` (kitti_dataset.py:142-288) for one subnet, on the host: `build_item` plus
    the training crop (`crop_u` = the three numbers in [0, 1) the reference draws with np.random.rand(3); None = no crop,
    the reference's split="val"), the bounds of what the crop keeps, the dense label grids, the multi-scale labels and the
    mask targets.  Returns the reference's keys."""
    it = build_item(xyz, vote, intensity, embedding, semantic_label, instance_label, T, complete_scale, point_labels)
    sem_f, sem_c = it["semantic_label_sparse"]
    ins_f, ins_c = it["instance_label_sparse"]
    in_feat, in_coord, plab = it["in_feat"], it["in_coord"], it["input_pcd_instance_label"]
    if crop_u is not None:
        w = crop_window(sem_c, crop_u)
        keep_in, keep_sem, keep_ins = in_window(in_coord, w), in_window(sem_c, w), in_window(ins_c, w)
        in_feat, in_coord = in_feat[keep_in], in_coord[keep_in]
        sem_f, sem_c, ins_f, ins_c = sem_f[keep_sem], sem_c[keep_sem], ins_f[keep_ins], ins_c[keep_ins]
    min_c, max_c = sem_c.min(dim=0)[0], sem_c.max(dim=0)[0]
    if ins_c.shape[0] > 0:
        min_c = torch.min(min_c, ins_c.min(dim=0)[0])
        max_c = torch.max(max_c, ins_c.max(dim=0)[0])
    min_c, max_c = completion_bounds(min_c, max_c, complete_scale)
    scene = compute_scene_size(min_c, max_c, scale=complete_scale)
    sem, ins = dense_labels(sem_f, sem_c, ins_f, ins_c, min_c, scene)
    geo, lab = multiscale_labels(sem, n_classes)
    sem_o, ins_o = torch.from_numpy(semantic_label).to(torch.uint8), torch.from_numpy(instance_label).to(torch.uint8)
    return {"xyz": it["xyz"], "frame_id": frame_id, "sequence": sequence, "in_feat": in_feat, "in_coord": in_coord,
            "T": it["T"], "min_C": min_c, "max_C": max_c, "semantic_label": sem, "instance_label": ins,
            "mask_label": mask_targets(sem, ins, thing_ids), "geo_labels": geo, "sem_labels": lab,
            "semantic_label_origin": sem_o, "instance_label_origin": ins_o,
            "mask_label_origin": mask_targets(sem_o, ins_o, thing_ids), "input_pcd_instance_label": plab}


def collate_train(items: Sequence[Dict], complete_scale: int = 8) -> Dict:
    """Training items -> the reference's training batch (collate.py:11-107): `collate`'s keys plus the per-subnet label
    lists, geo_labels / sem_labels as dicts of lists, and the stacked origin grids."""
    out = collate(items, complete_scale)
    out.update({"frame_id": [it["frame_id"] for it in items], "sequence": [it["sequence"] for it in items],
                "geo_labels": {f"1_{s}": [it["geo_labels"][f"1_{s}"] for it in items] for s in SCALES},
                "sem_labels": {f"1_{s}": [it["sem_labels"][f"1_{s}"] for it in items] for s in SCALES},
                "semantic_label": [it["semantic_label"] for it in items],
                "instance_label": [it["instance_label"] for it in items],
                "semantic_label_origin": torch.stack([it["semantic_label_origin"] for it in items]),
                "instance_label_origin": torch.stack([it["instance_label_origin"] for it in items]),
                "mask_label": [it["mask_label"] for it in items],
                "mask_label_origin": [it["mask_label_origin"] for it in items]})
    return out


class FrameReader:
    """Directory layout of the reference's SemanticKITTI setup (kitti_dataset.py:100-112,344-370):
        <root>/dataset/sequences/<seq>/labels/<frame>.label
        <preprocess_root>/instance_labels_v2/<seq>/<frame>_1_1.pkl
        <preprocess_root>/waffleiron_v2/sequences/<seq>/seg_feats_tta/<frame>.pkl
    With `features=` a `pasco_amd.waffle.Extractor` the last file is not read: its three arrays are computed from
    `<root>/dataset/sequences/<seq>/velodyne/<frame>.bin`.
    `batch(seq, frame, Ts)` returns the collated a0 contract for len(Ts) subnets (the reference's validation loader
    feeds every subnet the same frame under its own transform)."""

    def __init__(self, root: str, preprocess_root: str, complete_scale: int = 8, instances: str = "file",
                 config: Optional[str] = None, grid=(256, 256, 32), thing_ids=(1, 2, 3, 4, 5, 6, 7, 8), label_device="cuda",
                 features=None):
        """`instances="file"` reads the label grids from the instance pickle; `"device"` builds them from the dataset's own
        `voxels/<frame>.label` / `.invalid` with the pl_* kernels on `label_device` (`data.instances`; `config` is the
        dataset's semantic-kitti.yaml), so no instance_labels_v2 directory is needed."""
        if instances not in ("file", "device"):
            raise ValueError(f"instances={instances!r}: 'file' or 'device'")
        if instances == "device" and config is None:
            raise ValueError("instances='device' needs the dataset's semantic-kitti.yaml (config=...)")
        self.root, self.preprocess_root, self.complete_scale = root, preprocess_root, complete_scale
        self.instances, self.grid, self.thing_ids, self.label_device = instances, tuple(grid), tuple(thing_ids), label_device
        self._lut, self._config, self._last = None, config, (None, None)
        self.features = features

    def paths(self, sequence: str, frame_id: str):
        return (os.path.join(self.preprocess_root, "instance_labels_v2", sequence, f"{frame_id}_1_1.pkl"),
                os.path.join(self.preprocess_root, "waffleiron_v2/sequences", sequence, "seg_feats_tta", f"{frame_id}.pkl"),
                os.path.join(self.root, "dataset", "sequences", sequence, "labels", f"{frame_id}.label"))

    def _device_labels(self, sequence: str, frame_id: str):
        from . import instances as I
        if self._last[0] != (sequence, frame_id):       # labels() and batch() of one frame share one run
            if self._lut is None:
                self._lut = I.remap_lut(self._config)
            vox = os.path.join(self.root, "dataset", "sequences", sequence, "voxels")
            sem = I.semantic_grid(os.path.join(vox, frame_id + ".label"), os.path.join(vox, frame_id + ".invalid"),
                                  self._lut, self.label_device, self.grid)
            ins, sem, _ = I.instance_labels(sem, self.thing_ids, I.MIN_SIZE, self.label_device)
            self._last = ((sequence, frame_id), I.as_label_pair(ins, sem))
        return self._last[1]

    def labels(self, sequence: str, frame_id: str):
        """The frame's origin label grids (semantic uint8 with 255 = unknown, instance ids): what the reference's
        `semantic_label_origin` / `mask_label_origin` are built from; `pasco_amd.eval.GroundTruth.from_labels` takes them."""
        if self.instances == "device":
            return self._device_labels(sequence, frame_id)
        return read_instance_label_pickle(self.paths(sequence, frame_id)[0])

    def batch(self, sequence: str, frame_id: str, Ts: Sequence[torch.Tensor], embedding_index: int = 0,
              device=None) -> Dict:
        """`device=None` (or a CPU device) runs the host restatement `build_item`; a GPU device runs the same preparation
        through the pf_* kernels (`data.device_prep`), bit-equal, with the batch's tensors left on that device."""
        _, feats, pts = self.paths(sequence, frame_id)
        if self.features is not None:
            scan = read_pointcloud(os.path.join(self.root, "dataset", "sequences", sequence, "velodyne", f"{frame_id}.bin"))
            feats = self.features.frame(scan, int(frame_id))
        sem, ins = self.labels(sequence, frame_id)
        if device is not None and torch.device(device).type == "cuda":
            plab = read_point_instance_labels(pts) if os.path.exists(pts) else None
            return prepare_semantic_kitti_on_device(feats, sem, ins, Ts, device, embedding_index, self.complete_scale, plab)
        xyz, vote, intensity, emb = read_waffleiron_features(feats, embedding_index=embedding_index)
        plab = read_point_instance_labels(pts) if os.path.exists(pts) else None
        items = [build_item(xyz, vote, intensity, emb, sem, ins, T, self.complete_scale, plab) for T in Ts]
        return collate(items, self.complete_scale)

    def train_batch(self, sequence: str, frame_id: str, Ts: Sequence[torch.Tensor], crop_u=None, embedding_index: int = 0,
                    device=None, n_classes: int = 20) -> Dict:
        """The batch `Net.step` consumes: `batch`'s keys plus the label targets of every subnet under its transform (`Ts`, e.g.
        from `data.augment.random_transformation`) and its training crop (`crop_u`: len(Ts) x 3 numbers in [0, 1), what the
        reference draws with np.random.rand(3) per item; None = no crop, the reference's validation items).  `device=None` (or
        a CPU device) runs the host restatement `build_train_item`; a GPU device runs the pf_* kernels for the points and the
        pt_* kernels for the targets (`data.targets`), bit-equal, with the tensors left on that device."""
        _, feats, pts = self.paths(sequence, frame_id)
        if self.features is not None:
            scan = read_pointcloud(os.path.join(self.root, "dataset", "sequences", sequence, "velodyne", f"{frame_id}.bin"))
            feats = self.features.frame(scan, int(frame_id))
        sem, ins = self.labels(sequence, frame_id)
        us = None if crop_u is None else np.asarray(crop_u, dtype=np.float64).reshape(len(Ts), 3)
        plab = read_point_instance_labels(pts) if os.path.exists(pts) else None
        if device is not None and torch.device(device).type == "cuda":
            from . import device_prep as DP
            from .targets import assemble_train_batch
            base = prepare_semantic_kitti_on_device(feats, sem, ins, Ts, device, embedding_index, self.complete_scale, plab)
            return assemble_train_batch(base, DP.upload(sem, device), DP.upload(ins, device), thing_ids=self.thing_ids,
                                        n_classes=n_classes, complete_scale=self.complete_scale, crop_u=us, frame_id=frame_id,
                                        sequence=sequence)
        xyz, vote, intensity, emb = read_waffleiron_features(feats, embedding_index=embedding_index)
        items = [build_train_item(xyz, vote, intensity, emb, sem, ins, T, self.complete_scale, plab,
                                  crop_u=None if us is None else us[m], thing_ids=self.thing_ids, n_classes=n_classes,
                                  frame_id=frame_id, sequence=sequence) for m, T in enumerate(Ts)]
        return collate_train(items, self.complete_scale)


def prepare_semantic_kitti_on_device(feats_path: str, semantic_label: np.ndarray, instance_label: np.ndarray,
                                     Ts: Sequence[torch.Tensor], device, embedding_index: int = 0, complete_scale: int = 8,
                                     point_labels: Optional[np.ndarray] = None) -> Dict:
    """`collate([build_item(...) for T in Ts])` through the pf_* kernels on `device`.  The WaffleIron arrays go up as they
    are stored (the embedding as [256, P], read transposed by the kernel) - no host-side concatenation."""
    from . import device_prep as DP
    from .frame_lib import _seg, segment
    data = feats_path if isinstance(feats_path, dict) else _load_pickle(feats_path)
    pts = DP.upload(np.ascontiguousarray(data["coords"]), device)
    vote = DP.upload(np.ascontiguousarray(data["vote"]), device).contiguous()
    emb = DP.upload(np.ascontiguousarray(data["embedding"][embedding_index]), device).contiguous()    # [256, P]
    sem, ins = DP.upload(semantic_label, device), DP.upload(instance_label, device)
    n = int(pts.shape[0])
    plab = None if point_labels is None else DP.upload(point_labels, device)
    return DP.prepare(pts, sem, ins, Ts, lo=MIN_EXTENT, hi=MAX_EXTENT, lo_fp64=(0, 0, 0), hi_fp64=(0, 0, 0),
                      origin=VOX_ORIGIN, voxel=VOXEL_SIZE, centre_fp64=False,
                      pre=[segment(vote), _seg(pts[:, 3:], 1, 4, 1)], post=[_seg(emb, int(emb.shape[0]), 1, n)],
                      complete_scale=complete_scale, point_labels=plab)
