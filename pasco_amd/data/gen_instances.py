"""Write `<preprocess_root>/instance_labels_v2/<seq>/<frame>_1_1.pkl` for a whole dataset tree: the files both scoring
CLIs and the frame readers need, in the reference's format (label_gen/gen_instance_labels.py and its KITTI-360 twin).

    python -m pasco_amd.data.gen_instances --root <kitti> --preprocess-root <out> --config <semantic-kitti.yaml>
                                           [--sequences 08,00,...] [--frame-interval 5] [--device cuda|cpu]
    python -m pasco_amd.data.gen_instances --kitti360 --label-root <SSCBench-KITTI-360> --preprocess-root <out>
                                           [--sequences ...] [--device cuda|cpu]

SemanticKITTI: every `<root>/dataset/sequences/<seq>/voxels/<frame>.label` with `float(frame) % frame_interval == 0`, the
grid built from the .label / .invalid pair through the yaml's `learning_map`, thing ids 1..8.  KITTI-360: every
`<label_root>/labels/<seq>/*_1_1.npy` as stored, thing ids 1..6.  A file that exists is skipped.  The next frame's files are
read on a host thread while the device works on the current one.  `--device cuda` (default) runs the pl_* kernels, `--device
cpu` the numpy restatement of `data.instances`; the files are the same.
"""
from __future__ import annotations

import argparse
import glob
import os
import time
from concurrent.futures import ThreadPoolExecutor
from typing import List, Tuple

import numpy as np
import torch

from . import instances as I
from .kitti360 import THING_IDS as KITTI360_THING_IDS

KITTI_SEQUENCES = ("08", "00", "01", "02", "03", "04", "05", "06", "07", "09", "10")
KITTI360_SEQUENCES = ("2013_05_28_drive_0004_sync", "2013_05_28_drive_0000_sync", "2013_05_28_drive_0010_sync",
                      "2013_05_28_drive_0002_sync", "2013_05_28_drive_0003_sync", "2013_05_28_drive_0005_sync",
                      "2013_05_28_drive_0007_sync", "2013_05_28_drive_0006_sync", "2013_05_28_drive_0009_sync")
KITTI_THING_IDS = (1, 2, 3, 4, 5, 6, 7, 8)


def kitti_frames(root: str, sequence: str, frame_interval: int = 5) -> List[str]:
    """Frame ids of a SemanticKITTI sequence that carry a voxel label and pass the reference's `% frame_interval` rule."""
    names = sorted(glob.glob(os.path.join(root, "dataset", "sequences", sequence, "voxels", "*.label")))
    ids = [os.path.splitext(os.path.basename(p))[0] for p in names]
    return [f for f in ids if float(f) % frame_interval == 0]


def kitti360_frames(label_root: str, sequence: str) -> List[str]:
    names = sorted(glob.glob(os.path.join(label_root, "labels", sequence, "*_1_1.npy")))
    return [os.path.splitext(os.path.basename(p))[0].split("_")[0] for p in names]


def out_path(preprocess_root: str, sequence: str, frame_id: str) -> str:
    return os.path.join(preprocess_root, "instance_labels_v2", sequence, f"{frame_id}_1_1.pkl")


def _jobs(a) -> List[Tuple[str, str, str]]:
    """-> [(sequence, frame id, output path)] still to be written."""
    jobs = []
    seqs = a.sequences.split(",") if a.sequences else (KITTI360_SEQUENCES if a.kitti360 else KITTI_SEQUENCES)
    for seq in seqs:
        ids = kitti360_frames(a.label_root, seq) if a.kitti360 else kitti_frames(a.root, seq, a.frame_interval)
        if ids:
            os.makedirs(os.path.dirname(out_path(a.preprocess_root, seq, ids[0])), exist_ok=True)
        jobs += [(seq, f, out_path(a.preprocess_root, seq, f)) for f in ids]
    return [j for j in jobs if not os.path.exists(j[2])]


def _read(a, seq: str, frame_id: str):
    """The frame's files as stored (host thread)."""
    if a.kitti360:
        return np.load(os.path.join(a.label_root, "labels", seq, f"{frame_id}_1_1.npy"))
    vox = os.path.join(a.root, "dataset", "sequences", seq, "voxels")
    return I.read_raw_voxels(os.path.join(vox, frame_id + ".label"), os.path.join(vox, frame_id + ".invalid"))


def generate(a) -> dict:
    """Run the jobs of parsed arguments `a` -> {"frames", "seconds", "over_uint8"}."""
    device = None if a.device == "cpu" else torch.device(a.device)
    if device is not None and not torch.cuda.is_available():
        raise RuntimeError("--device cuda needs a GPU; --device cpu runs the host restatement")
    grid = tuple(int(v) for v in a.grid.split(","))
    lut = None if a.kitti360 else I.remap_lut(a.config)
    things = KITTI360_THING_IDS if a.kitti360 else KITTI_THING_IDS
    jobs = _jobs(a)
    over = []
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=1) as pool:
        nxt = pool.submit(_read, a, jobs[0][0], jobs[0][1]) if jobs else None
        for k, (seq, fid, path) in enumerate(jobs):
            data = nxt.result()
            nxt = pool.submit(_read, a, jobs[k + 1][0], jobs[k + 1][1]) if k + 1 < len(jobs) else None
            if a.kitti360:
                sem, dtype = data.astype(np.uint8), data.dtype
            else:
                sem, dtype = I.semantic_grid_from_raw(data[0], data[1], lut, grid, device), np.float32
            ins, sem_out, info = I.instance_labels(sem, things, I.MIN_SIZE, device)
            if info["over_uint8"]:
                over.append((seq, fid, info["n_instances"]))
            I.write_instance_pickle(path, ins, sem_out, dtype)
    return {"frames": len(jobs), "seconds": time.perf_counter() - t0, "over_uint8": over}


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", help="SemanticKITTI root (dataset/sequences/...)")
    ap.add_argument("--preprocess-root", required=True, help="output root (instance_labels_v2/... is created below it)")
    ap.add_argument("--config", help="semantic-kitti.yaml (learning_map)")
    ap.add_argument("--kitti360", action="store_true", help="SSCBench-KITTI-360 instead of SemanticKITTI")
    ap.add_argument("--label-root", help="SSCBench-KITTI-360 root (labels/<seq>/*_1_1.npy)")
    ap.add_argument("--sequences", default="", help="comma-separated; default: the reference's list")
    ap.add_argument("--frame-interval", type=int, default=5)
    ap.add_argument("--grid", default="256,256,32", help="X,Y,Z of a SemanticKITTI voxel file")
    ap.add_argument("--device", default="cuda", help="cuda[:n] (the pl_* kernels) or cpu (the numpy restatement)")
    return ap


def main(argv=None):
    ap = parser()
    a = ap.parse_args(argv)
    if a.kitti360 and not a.label_root:
        ap.error("--kitti360 needs --label-root")
    if not a.kitti360 and not (a.root and a.config):
        ap.error("SemanticKITTI needs --root and --config")
    r = generate(a)
    for seq, fid, n in r["over_uint8"]:
        print(f"note: {seq}/{fid} has {n} instances; the readers cast the grid to uint8 (ids above 255 wrap)")
    rate = r["frames"] / r["seconds"] if r["frames"] else 0.0
    print(f"{r['frames']} frames in {r['seconds']:.2f} s ({rate:.2f} frames/s)")


if __name__ == "__main__":
    main()
