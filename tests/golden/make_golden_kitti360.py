"""Fixtures for the KITTI-360 data layer, produced by the REFERENCE's own dataset (modelled on make_golden_io.py).

Runs only in the build container (needs /root/reference).  Step 1 writes a tiny synthetic SSCBench-KITTI-360 tree under
tests/golden/kitti360_mini/ (data generated with numpy - not reference code): one velodyne scan, one instance-label pickle,
an SSCBench `*_1_1.npy` placeholder (only so that the frame listing finds the frame) and a match file.  Step 2 runs the
reference's `Kitti360Dataset.get_individual` on that tree, its transform draw patched to return fixed transforms, and
stores in_feat / in_coord / min_C / max_C in tests/golden/kitti360_items.npz.  Step 3 stores the state-dict key / shape list
of a reduced `Net_kitti360`-shaped module tree (the reference's own `CylinderFeat`, `UNet3DV2`, `TransformerPredictorV2`
at 19 classes and 8 input channels, under the attribute names `Net_kitti360.__init__` gives them); the tests build a
checkpoint from it.

    python tests/golden/make_golden_kitti360.py
"""
import os
import pickle
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up sys.path, the MinkowskiEngine alias and the inert stubs)

MINI = os.path.join(HERE, "kitti360_mini")
GRID = (64, 64, 16)
SEQ, FRAME, RAW = "2013_05_28_drive_0009_sync", "000042", "0000000137"


def edge_points(rng):
    """Points on and next to (+-1 fp32 ulp) every extent bound and the voxel boundary x = 1.0."""
    lo, hi = (0.0, -25.6, -2.0), (51.2, 25.6, 4.4)
    rows = []
    for d in range(3):
        for b in (lo[d], hi[d], 1.0 if d == 0 else 0.2 * 3 + lo[d]):
            f = np.float32(b)
            for v in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))):
                p = np.array([5.0, -3.0, 0.5, 0.25], np.float32)
                p[d] = v
                rows.append(p)
    return np.stack(rows)


def write_inputs():
    rng = np.random.default_rng(360)
    velo = os.path.join(MINI, "data_3d_raw", SEQ, "velodyne_points", "data")
    ins = os.path.join(MINI, "preprocess", "instance_labels_v2", SEQ)
    lab = os.path.join(MINI, "sscbench", "labels", SEQ)
    for d in (velo, ins, lab):
        os.makedirs(d, exist_ok=True)
    sem = np.full(GRID, 255, np.uint8)
    sem[2:62, 4:60, :] = 0
    sem[2:62, 4:60, 2:4] = 7
    sem[10:20, 12:22, 4:9] = 1
    sem[40:46, 30:34, 4:8] = 6
    sem[30:34, 40:50, 4:12] = 11
    inst = np.zeros(GRID, np.uint8)
    inst[10:20, 12:22, 4:9] = 1
    inst[40:46, 30:34, 4:8] = 2
    inst[44:46, 30:31, 4:5] = 255          # a few voxels without an instance id
    with open(os.path.join(ins, f"{FRAME}_1_1.pkl"), "wb") as f:
        pickle.dump({"semantic_labels": sem, "instance_labels": inst}, f)
    np.save(os.path.join(lab, f"{FRAME}_1_1.npy"), np.zeros(1, np.uint8))
    P = 700
    xyz = np.stack([rng.uniform(-2, 14, P), rng.uniform(-27, -10, P), rng.uniform(-2.5, 1.5, P)], 1)
    pts = np.concatenate([xyz, rng.random((P, 1))], 1).astype(np.float32)
    pts = np.concatenate([pts, edge_points(rng)]).astype(np.float32)
    pts.tofile(os.path.join(velo, f"{RAW}.bin"))
    with open(os.path.join(MINI, "match.txt"), "w") as f:
        f.write(f"2013_05_28_drive_0000_sync 0000000009.png 000000.png\n{SEQ} 0000000130.png 000041.png\n"
                f"{SEQ} {RAW}.png {FRAME}.png\n{SEQ} 0000000141.png 000043.png\n")


def fixed_transforms():
    from pasco.models.transform_utils import generate_transformation
    sys.path.insert(0, G.ROOT)
    from pasco_amd.eval.kitti import subnet_transforms
    Ts = {"eye": torch.eye(4)}
    for i, T in enumerate(subnet_transforms(3)[1:], 1):
        Ts[f"table{i}"] = T
    Ts["rigid"] = torch.as_tensor(generate_transformation(rot=17.0, translation=(0.4, -0.3, 0.1), flip_dim=1,
                                                          scale=1.0)).float()
    return Ts


def golden_items():
    import pasco.data.kitti360.kitti360_dataset as KD
    out = {}
    for tag, T in fixed_transforms().items():
        ds = object.__new__(KD.Kitti360Dataset)
        ds.kitti360_root = MINI
        ds.kitti360_preprocess_root = os.path.join(MINI, "preprocess")
        ds.kitti360_label_root = os.path.join(MINI, "sscbench")
        ds.instance_label_root = os.path.join(ds.kitti360_preprocess_root, "instance_labels_v2")
        ds.label_root = os.path.join(ds.kitti360_label_root, "labels")
        ds.complete_scale = 8
        ds.data_aug = True
        ds.max_angle, ds.scale_range, ds.max_translation = 0.0, 0.0, np.zeros(3)
        ds.split, ds.n_subnets, ds.n_fuse_scans, ds.n_classes, ds.overfit = "test", 1, 1, 19, False
        ds.max_extent = (51.2, 25.6, 4.4)
        ds.min_extent = np.array([0, -25.6, -2.0])
        ds.vox_origin = np.array([0, -25.6, -2])
        ds.voxel_size = 0.2
        ds.thing_ids = KD.thing_ids
        ds.scans = [{"sequence": SEQ, "frame_id": FRAME, "original_id": RAW}]
        KD.generate_random_transformation = lambda _T=T, **kw: _T
        item = ds.get_individual(0)
        out.update({f"{tag}_T": T, f"{tag}_in_feat": item["in_feat"], f"{tag}_in_coord": item["in_coord"],
                    f"{tag}_min_C": item["min_C"], f"{tag}_max_C": item["max_C"], f"{tag}_xyz": item["xyz"]})
    out["tags"] = np.array(list(fixed_transforms()))
    G.save("kitti360_items.npz", **out)


def golden_net_keys():
    """Key / shape list of a reduced `Net_kitti360` (net_panoptic_sparse_kitti360.py: same module tree as `Net`)."""
    from pasco.models.unet3d_sparse_v2 import UNet3DV2, CylinderFeat
    from pasco.models.transformer.transformer_predictor_v2 import TransformerPredictorV2
    f, n_infers, nq, in_ch, n_classes = 8, 2, 6, 8, 19
    tp = TransformerPredictorV2(dropout=0.0, num_classes=n_classes, nheads=8, hidden_dim=48, enc_layers=0, num_queries=nq, dim_feedforward=96,
                                dec_layers=1, aux_loss=False, mask_dim=f, n_infers=n_infers, query_sample_ratio=1.0,
                                in_channels=[f * 4, f * 2, f])
    unet = UNet3DV2(heavy_decoder=False, drop_path_rate=0.0, n_classes=n_classes, in_channels=f * n_infers,
                    transformer_predictor=tp, f_maps=[f, f * 2, f * 4, f * 4], dense3d_dropout=0.0, n_infers=n_infers,
                    decoder_dropouts=[0.0] * 3, num_queries=nq, query_sample_ratio=1.0, encoder_dropouts=[0.0] * 3,
                    use_se_layer=False)
    feat = CylinderFeat(fea_dim=in_ch, out_pt_fea_dim=f)

    class NetShell(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.transformer_predictor = tp
            self.unet3d = unet
            self.feat = feat
            self.criterion = torch.nn.Module()
            self.criterion.register_buffer("empty_weight", torch.ones(n_classes + 1))

    sd = NetShell().state_dict()
    keys = np.array(list(sd))
    shapes = np.zeros((len(keys), 6), np.int64) - 1
    dtypes = np.array([str(v.dtype).replace("torch.", "") for v in sd.values()])
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = v.shape
    G.save("kitti360_net_keys.npz", keys=keys, shapes=shapes, dtypes=dtypes,
           hyper=np.array([n_classes, n_infers, in_ch, f, nq]))


if __name__ == "__main__":
    write_inputs()
    golden_items()
    golden_net_keys()
