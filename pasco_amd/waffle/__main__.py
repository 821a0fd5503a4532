"""Write `<result-folder>/sequences/<seq>/seg_feats_tta/<frame>.pkl` for a SemanticKITTI tree: the point features both scoring
commands read, in the reference's format (WaffleIron_mod/extract_point_features.py).

    python -m pasco_amd.waffle --root <kitti> --ckpt <ckpt_last.pth> --config <WaffleIron yaml>
                               --result-folder <preprocess>/waffleiron_v2 [--sequences 08] [--frame-interval 5]
                               [--num-votes 10] [--seed 0] [--half] [--device cpu]

Every `<root>/dataset/sequences/<seq>/velodyne/<frame>.bin` with `float(frame) % frame_interval == 0`.  The pickle holds
`embedding` [V, C, P] (the embedding layer's output of every vote, gathered back to the scan's points), `coords` [P, 4] (the
scan as read) and `vote` [P, classes] (the mean over votes of the class probabilities).  `--half` stores the embedding as
float16.  `--device cuda` (default) runs the pw_* kernels, `--device cpu` their restatement in `pasco_amd.waffle.host`.
"""
from __future__ import annotations

import argparse
import glob
import os
import pickle

from ..data.semantic_kitti import read_pointcloud
from . import Extractor


def scan_frames(root: str, sequence: str, frame_interval: int = 5):
    names = sorted(glob.glob(os.path.join(root, "dataset", "sequences", sequence, "velodyne", "*.bin")))
    ids = [os.path.splitext(os.path.basename(p))[0] for p in names]
    return [f for f in ids if float(f) % frame_interval == 0]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--root", required=True)
    ap.add_argument("--ckpt", required=True)
    ap.add_argument("--config", required=True)
    ap.add_argument("--result-folder", required=True)
    ap.add_argument("--sequences", default="08")
    ap.add_argument("--frame-interval", type=int, default=5)
    ap.add_argument("--num-votes", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--half", action="store_true")
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    a = ap.parse_args(argv)
    ex = Extractor(a.ckpt, a.config, a.device, a.num_votes, a.seed, a.half)
    for seq in a.sequences.split(","):
        out_dir = os.path.join(a.result_folder, "sequences", seq, "seg_feats_tta")
        os.makedirs(out_dir, exist_ok=True)
        for fid in scan_frames(a.root, seq, a.frame_interval):
            scan = read_pointcloud(os.path.join(a.root, "dataset", "sequences", seq, "velodyne", fid + ".bin"))
            item = ex.frame(scan, int(fid))
            path = os.path.join(out_dir, fid + ".pkl")
            with open(path, "wb") as f:
                pickle.dump(item, f)
            print(f"saved to {path}")


if __name__ == "__main__":
    main()
