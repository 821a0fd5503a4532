"""Fixtures for the point-feature stage (pasco_amd/waffle), produced by the REFERENCE's own modules on the CPU in fp32.

Runs only where the reference tree is present.  It imports the reference's `Segmenter`, `Voxelize`, `Crop` and
`PCDataset.get_occupied_2d_cells`, gives two small nets seeded random weights with non-trivial running statistics (every value
exactly representable in float16, so the weights can be stored in half the bytes), and records

    waffle_mini_c256_embed.npz / waffle_mini_c256_mix.npz / waffle_mini_c32.npz
        the nets' state dicts under the reference's key names, float16 (num_batches_tracked int64); the C = 256 net is split
        in two files to keep each one small.  tests/waffle_cases.py puts them back together as a reference-format checkpoint.
    waffle.npz       the synthetic scan, the reference's preparation outputs for it and for the kitti_mini scan under both
                     settings files, and the C = 32 net's fp32 (embedding, tokens, logits) on both
    waffle_c256.npz  the C = 256 net's fp32 results on both, every ROW_STEP-th row

    python tests/golden/make_golden_waffle.py <reference root>
"""
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1]
sys.path.insert(0, os.path.join(REF, "WaffleIron_mod"))
ROW_STEP = 4


def synthetic_scan(seed=11):
    """~1500 points: a ground sheet that reaches past the field of view on every side, two walls, three dense clusters (many
    points per 0.1 m voxel), a few isolated points high up and far out."""
    rng = np.random.default_rng(seed)
    ground = np.stack([rng.uniform(-62, 62, 700), rng.uniform(-62, 62, 700), rng.normal(-1.7, 0.03, 700)], 1)
    wall_a = np.stack([rng.uniform(5, 25, 200), np.full(200, 12.0) + rng.normal(0, 0.02, 200), rng.uniform(-1.7, 1.5, 200)], 1)
    wall_b = np.stack([np.full(150, -20.0) + rng.normal(0, 0.02, 150), rng.uniform(-30, 10, 150), rng.uniform(-1.7, 1.0, 150)], 1)
    clusters = [c + rng.normal(0, s, (150, 3)) for c, s in (((3.0, 1.0, -1.0), 0.05), ((-8.0, 6.0, -0.5), 0.2),
                                                             ((30.0, -30.0, 0.0), 0.4))]
    lone = np.array([[0.0, 0.0, 1.9], [49.0, 49.0, 1.5], [-49.5, 10.0, -2.9], [70.0, 0.0, 0.0], [0.0, -80.0, 3.0],
                     [10.0, 10.0, 6.0], [10.0, 10.0, -6.0]])
    xyz = np.concatenate([ground, wall_a, wall_b, *clusters, lone], 0)
    xyz = xyz[rng.permutation(xyz.shape[0])]
    return np.concatenate([xyz, rng.random((xyz.shape[0], 1))], 1).astype(np.float32)


def random_state(net, seed):
    g = torch.Generator().manual_seed(seed)
    state = net.state_dict()
    for k, v in state.items():
        if k.endswith("num_batches_tracked"):
            v.fill_(100)
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))
        elif k.endswith("running_mean"):
            v.copy_(0.3 * torch.randn(v.shape, generator=g))
        elif ".norm." in k or ".conv2.0." in k or ".conv2.2." in k:        # BatchNorm weight / bias
            v.copy_(1.0 + 0.2 * torch.randn(v.shape, generator=g) if k.endswith("weight") else 0.1 * torch.randn(v.shape, generator=g))
        elif ".scale." in k:
            v.copy_(0.5 + 0.25 * torch.randn(v.shape, generator=g))
        elif k.endswith("bias"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        else:                                                               # keep the module's own initial weights' spread
            v.copy_(v.std() * torch.randn(v.shape, generator=g) if v.numel() > 1 else v)
        if v.is_floating_point():
            v.copy_(v.half().float())
    net.load_state_dict(state)
    return state


def as_arrays(state):
    return {k: (v.numpy().astype(np.float16) if v.is_floating_point() else v.numpy()) for k, v in state.items()}


def reference_prep(scan, cfg):
    """What `PCDataset.__getitem__` does for phase "val" without test-time augmentation, on an in-memory scan."""
    from datasets.pc_dataset import PCDataset
    w, e = cfg["waffleiron"], cfg["embedding"]
    ds = PCDataset(rootdir=None, phase="val", input_feat=e["input_feat"], voxel_size=e["voxel_size"],
                   dim_proj=w["dim_proj"], grids_shape=w["grids_size"], fov_xyz=w["fov_xyz"], num_neighbors=e["neighbors"])
    from scipy.spatial import cKDTree
    pc_orig = ds.prepare_input_features(scan)
    labels = np.zeros(pc_orig.shape[0], np.int64)
    vox, _ = ds.downsample(pc_orig, labels)
    pc, _ = ds.crop_to_fov(vox, np.zeros(vox.shape[0], np.int64))
    cell_ind = ds.get_occupied_2d_cells(pc)
    tree = cKDTree(pc[:, :3])
    _, neigh = tree.query(pc[:, :3], k=e["neighbors"] + 1)
    _, up = tree.query(pc_orig[:, :3], k=1)
    return {"pc_orig": pc_orig, "vox": vox, "pc": pc, "cell_ind": cell_ind.astype(np.int32), "neigh": neigh.T.astype(np.int32),
            "upsample": up.astype(np.int32)}


def reference_net(net, prep):
    feat = torch.from_numpy(prep["pc"][:, 3:].T[None]).float()
    cell = torch.from_numpy(prep["cell_ind"][None]).long()
    occ = torch.ones((1, feat.shape[-1]))
    neigh = torch.from_numpy(prep["neigh"][None]).long()
    with torch.no_grad():
        emb, tok, logits = net(feat, cell, occ, neigh)
    return [t[0].T.contiguous().numpy() for t in (emb, tok, logits)]


def main():
    from waffleiron import Segmenter
    scans = {"synth": synthetic_scan(),
             "mini": np.fromfile(os.path.join(HERE, "kitti_mini", "dataset", "sequences", "08", "velodyne", "000005.bin"),
                                 dtype=np.float32).reshape(-1, 4)}
    small, wide = {"scan_synth": scans["synth"]}, {"row_step": np.int64(ROW_STEP)}
    for name, seed in (("c256", 256), ("c32", 32)):
        with open(os.path.join(HERE, f"waffle_{name}.yaml")) as f:
            cfg = yaml.safe_load(f)
        w = cfg["waffleiron"]
        net = Segmenter(cfg["embedding"]["size_input"], w["nb_channels"], cfg["classif"]["nb_class"], w["depth"],
                        w["grids_size"]).eval()
        arrays = as_arrays(random_state(net, seed))
        if name == "c256":
            np.savez(os.path.join(HERE, "waffle_mini_c256_embed.npz"), **{k: v for k, v in arrays.items() if not k.startswith("waffleiron.")})
            np.savez(os.path.join(HERE, "waffle_mini_c256_mix.npz"), **{k: v for k, v in arrays.items() if k.startswith("waffleiron.")})
        else:
            np.savez(os.path.join(HERE, "waffle_mini_c32.npz"), **arrays)
        for sname, scan in scans.items():
            prep = reference_prep(scan, cfg)
            emb, tok, logits = reference_net(net, prep)
            tag = f"{sname}_{name}"
            small[f"{tag}_cell_ind"] = prep["cell_ind"]
            if name == "c32":                       # the cloud, the neighbours and upsample do not depend on the grids
                for k in ("vox", "pc", "neigh", "upsample"):
                    small[f"{sname}_{k}"] = prep[k]
                small.update({f"{tag}_embedding": emb, f"{tag}_tokens": tok, f"{tag}_logits": logits})
            else:
                wide.update({f"{tag}_embedding": emb[::ROW_STEP], f"{tag}_tokens": tok[::ROW_STEP], f"{tag}_logits": logits[::ROW_STEP]})
            print(tag, "points", prep["pc"].shape[0], "of", scan.shape[0], "max |tokens|", float(np.abs(tok).max()))
    np.savez(os.path.join(HERE, "waffle.npz"), **small)
    np.savez(os.path.join(HERE, "waffle_c256.npz"), **wide)


if __name__ == "__main__":
    main()
