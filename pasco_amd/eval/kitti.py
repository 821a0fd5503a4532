"""Score a trained checkpoint on a SemanticKITTI tree and print the reference's three result tables.

    python -m pasco_amd.eval.kitti --root <kitti root> --preprocess-root <preprocess root> --ckpt <model.ckpt> [--frames N]
                                   [--device-prep] [--instances-on-device --config <semantic-kitti.yaml>]
                                   [--save-outputs DIR]
                                   [--features-on-device --waffle-ckpt <ckpt_last.pth> --waffle-config <yaml> [--num-votes V]]

Per frame: `FrameReader.batch` -> `net_from_checkpoint(...).step_inference` -> `SceneEvaluator.add` with the frame's
`GroundTruth`.  Subnet transforms: subnet 0 sees the frame as it is, subnet i >= 1 under the fixed rotation / translation
table of the synthetic benchmark (theta_i in (0, 10, -10, 20, -20, 30, -30, 5) degrees,
t_i = ((i mod 3 - 1) 0.2, (floor(i / 3) mod 3 - 1) 0.2, 0) m).  This is NOT the reference's validation draw, which samples a
random transform per subnet and frame, so subnet rows can differ from the paper's by that draw.  The "inference time" column
is the measured mean wall time of `step_inference` in milliseconds (the reference prints 0.00 there: its caller passes 0).
`--device-prep` prepares each frame with the pf_* kernels (`FrameReader.batch(device=...)`, bit-equal) instead of on the host.
`--instances-on-device` builds the panoptic ground truth from the dataset's own `voxels/<frame>.label` / `.invalid` with the
pl_* kernels (`data.instances`) instead of reading `instance_labels_v2/*.pkl`; frames are then listed from the dataset tree
(`float(frame) % 5 == 0`, as the reference's generator selects them).
`--save-outputs DIR` also writes `DIR/<frame>_<i>.pkl` for every output i of a frame (the subnets, then the ensemble) with the
keys the reference's saving script writes; `python -m pasco_amd.viz` draws them.  Off by default; scoring is unchanged by it.
`--features-on-device` computes the WaffleIron point features of every frame from `velodyne/<frame>.bin` with the pw_* kernels
(`pasco_amd.waffle`) instead of reading `waffleiron_v2/.../seg_feats_tta/<frame>.pkl`: no waffleiron_v2 folder is needed.
"""
from __future__ import annotations

import argparse
import os
import time

import numpy as np
import torch

from ..data import FrameReader, net_from_checkpoint
from ..graph.synth import THETAS_DEG, generate_transformation
from .gt import GroundTruth
from .metrics import SceneEvaluator


def subnet_transforms(m: int):
    Ts = [torch.eye(4)]
    for i in range(1, m):
        t = np.array([((i % 3) - 1) * 0.2, (((i // 3) % 3) - 1) * 0.2, 0.0])
        Ts.append(torch.from_numpy(generate_transformation(THETAS_DEG[i % len(THETAS_DEG)], t)).float())
    return Ts


def frames_of(preprocess_root: str, sequence: str, root: str = None, frame_interval: int = 5):
    """Labelled frames of a sequence: from the instance pickles, or (with `root`) from the dataset tree itself."""
    if root is not None:
        from ..data.gen_instances import kitti_frames
        return kitti_frames(root, sequence, frame_interval)
    d = os.path.join(preprocess_root, "instance_labels_v2", sequence)
    return sorted(f[:-len("_1_1.pkl")] for f in os.listdir(d) if f.endswith("_1_1.pkl"))


def evaluate(root: str, preprocess_root: str, ckpt: str, sequence: str = "08", frames: int = 0, device: str = "cuda",
             device_prep: bool = False, instances: str = "file", config: str = None, grid=(256, 256, 32),
             save_outputs: str = None, features: str = "file", waffle_ckpt: str = None, waffle_config: str = None,
             num_votes: int = 10):
    """-> (SceneEvaluator, mean step time in ms)."""
    dev = torch.device(device)
    net = net_from_checkpoint(ckpt, device=dev)
    extractor = None
    if features == "device":
        if not (waffle_ckpt and waffle_config):
            raise ValueError("features='device' needs the WaffleIron checkpoint and its yaml (waffle_ckpt=, waffle_config=)")
        from ..waffle import Extractor
        extractor = Extractor(waffle_ckpt, waffle_config, dev, num_votes=num_votes)
    elif features != "file":
        raise ValueError(f"features={features!r}: 'file' or 'device'")
    if instances == "device":
        reader = FrameReader(root, preprocess_root, instances="device", config=config, grid=grid,
                             thing_ids=net.thing_ids, label_device=dev, features=extractor)
        ids = frames_of(preprocess_root, sequence, root=root)
    else:
        reader = FrameReader(root, preprocess_root, features=extractor)
        ids = frames_of(preprocess_root, sequence)
    if frames:
        ids = ids[:frames]
    if not ids:
        raise FileNotFoundError(f"no labelled frame of sequence {sequence} under {preprocess_root}")
    Ts = subnet_transforms(net.n_infers)
    ev = SceneEvaluator(n_classes=net.n_classes, thing_ids=net.thing_ids, n_outputs=net.n_infers + 1)
    times = []
    for fid in ids:
        sem, ins = reader.labels(sequence, fid)
        net.ensembler.scene_size = tuple(int(v) for v in sem.shape)
        b = reader.batch(sequence, fid, Ts, device=dev if device_prep else None)
        with torch.no_grad():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            outs, sem_probs, _ = net.step_inference([t.to(dev) for t in b["in_feats"]], [t.to(dev) for t in b["in_coords"]],
                                                    [t.to(dev) for t in b["Ts"]], b["global_min_Cs"], b["global_max_Cs"],
                                                    b["min_Cs"], b["max_Cs"])
            torch.cuda.synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
            gt = GroundTruth.from_labels(sem, ins, net.thing_ids, device=dev)
            ev.add(outs, sem_probs, gt)
            if save_outputs:
                from ..viz.outputs import save_step_outputs
                save_step_outputs(save_outputs, fid, outs, sem_probs, gt, sem, ins, xyz=b["xyz"][0] if "xyz" in b else None)
    return ev, float(np.mean(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", required=True)
    ap.add_argument("--preprocess-root", required=True)
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--sequence", default="08")
    ap.add_argument("--frames", type=int, default=0, help="first N labelled frames (0 = all)")
    ap.add_argument("--device-prep", action="store_true", help="prepare frames with the pf_* kernels on the device")
    ap.add_argument("--instances-on-device", action="store_true",
                    help="build the instance labels from the dataset's voxel files with the pl_* kernels (needs --config)")
    ap.add_argument("--config", help="the dataset's semantic-kitti.yaml (learning_map), for --instances-on-device")
    ap.add_argument("--grid", default="256,256,32", help="X,Y,Z of a voxel file, for --instances-on-device")
    ap.add_argument("--save-outputs", metavar="DIR", help="also write <frame>_<i>.pkl per output, for python -m pasco_amd.viz")
    ap.add_argument("--features-on-device", action="store_true",
                    help="compute the WaffleIron point features from velodyne/ with the pw_* kernels (needs --waffle-ckpt, --waffle-config)")
    ap.add_argument("--waffle-ckpt", help="the WaffleIron checkpoint (ckpt_last.pth), for --features-on-device")
    ap.add_argument("--waffle-config", help="the WaffleIron yaml, for --features-on-device")
    ap.add_argument("--num-votes", type=int, default=10, help="test-time augmentations per frame, for --features-on-device")
    a = ap.parse_args(argv)
    if a.instances_on_device and not a.config:
        ap.error("--instances-on-device needs --config")
    if a.features_on_device and not (a.waffle_ckpt and a.waffle_config):
        ap.error("--features-on-device needs --waffle-ckpt and --waffle-config")
    ev, step_ms = evaluate(a.root, a.preprocess_root, a.ckpt, a.sequence, a.frames, device_prep=a.device_prep,
                           instances="device" if a.instances_on_device else "file", config=a.config,
                           grid=tuple(int(v) for v in a.grid.split(",")), save_outputs=a.save_outputs,
                           features="device" if a.features_on_device else "file", waffle_ckpt=a.waffle_ckpt,
                           waffle_config=a.waffle_config, num_votes=a.num_votes)
    print(ev.tables(step_time=step_ms), end="")


if __name__ == "__main__":
    main()
