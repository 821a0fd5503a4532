"""Score a trained `Net_kitti360` checkpoint on an SSCBench-KITTI-360 tree and print the reference's three result tables.

    python -m pasco_amd.eval.kitti360 --root <KITTI-360 root> --preprocess-root <preprocess root> --label-root <SSCBench root>
                                      --match-file <kitti_360_match.txt> --ckpt <model.ckpt> [--split val|test] [--frames N]
                                      [--host-prep] [--instances-on-device] [--save-outputs DIR]

Per frame: `Kitti360FrameReader.batch` -> `net_from_checkpoint(..., thing_ids=(1..6)).step_inference` -> `SceneEvaluator.add`
with the frame's `GroundTruth`, under the 19 KITTI-360 class names.  Frames are prepared on the device by default (the pf_*
kernels, bit-equal to the host restatement; `--host-prep` runs that restatement instead).  Subnet transforms: the fixed table
of `eval.kitti` (subnet 0 sees the frame as it is).  This is NOT the reference's validation draw, which samples a random
rotation of up to 10 degrees, a translation and flips per subnet and frame, so subnet rows can differ from the paper's by that
draw.  The "inference time" column is the measured mean wall time of `step_inference` in milliseconds.
`--instances-on-device` builds the panoptic ground truth from `<label-root>/labels/<seq>/<frame>_1_1.npy` with the pl_* kernels
(`data.instances`) instead of reading `instance_labels_v2/*.pkl`.
`--save-outputs DIR` also writes `DIR/<frame>_<i>.pkl` per output of a frame, as `eval.kitti` does; off by default.
"""
from __future__ import annotations

import argparse
import time

import numpy as np
import torch

from ..data import Kitti360FrameReader, net_from_checkpoint
from ..data.kitti360 import CLASS_NAMES, THING_IDS
from .gt import GroundTruth
from .kitti import subnet_transforms
from .metrics import SceneEvaluator


def evaluate(root: str, preprocess_root: str, label_root: str, match_file: str, ckpt: str, split: str = "test",
             frames: int = 0, device: str = "cuda", device_prep: bool = True, instances: str = "file",
             save_outputs: str = None):
    """-> (SceneEvaluator, mean step time in ms)."""
    dev = torch.device(device)
    net = net_from_checkpoint(ckpt, device=dev, thing_ids=THING_IDS)
    if net.n_classes != len(CLASS_NAMES):
        raise ValueError(f"{ckpt}: {net.n_classes} classes, a KITTI-360 checkpoint has {len(CLASS_NAMES)}")
    reader = Kitti360FrameReader(root, preprocess_root, label_root, match_file, instances=instances, label_device=dev)
    ids = reader.frames(split)
    if frames:
        ids = ids[:frames]
    if not ids:
        raise FileNotFoundError(f"no labelled frame of split {split} under {label_root}")
    Ts = subnet_transforms(net.n_infers)
    ev = SceneEvaluator(n_classes=net.n_classes, thing_ids=net.thing_ids, n_outputs=net.n_infers + 1,
                        class_names=CLASS_NAMES)
    times = []
    for seq, fid in ids:
        sem, ins = reader.labels(seq, fid)
        net.ensembler.scene_size = tuple(int(v) for v in sem.shape)
        b = reader.batch(seq, fid, Ts, device=dev if device_prep else None)
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
    ap.add_argument("--root", required=True, help="KITTI-360 root (data_3d_raw/...)")
    ap.add_argument("--preprocess-root", required=True, help="PaSCo preprocess root (instance_labels_v2/...)")
    ap.add_argument("--label-root", required=True, help="SSCBench-KITTI-360 root (labels/<seq>/*_1_1.npy)")
    ap.add_argument("--match-file", required=True, help="`sequence raw_id sscbench_id` per line")
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--split", default="test", choices=("val", "test"))
    ap.add_argument("--frames", type=int, default=0, help="first N labelled frames (0 = all)")
    ap.add_argument("--host-prep", action="store_true", help="prepare frames on the host instead of with the pf_* kernels")
    ap.add_argument("--instances-on-device", action="store_true",
                    help="build the instance labels from the label .npy files with the pl_* kernels")
    ap.add_argument("--save-outputs", metavar="DIR", help="also write <frame>_<i>.pkl per output, for python -m pasco_amd.viz")
    a = ap.parse_args(argv)
    ev, step_ms = evaluate(a.root, a.preprocess_root, a.label_root, a.match_file, a.ckpt, a.split, a.frames,
                           device_prep=not a.host_prep, instances="device" if a.instances_on_device else "file",
                           save_outputs=a.save_outputs)
    print(ev.tables(step_time=step_ms), end="")


if __name__ == "__main__":
    main()
