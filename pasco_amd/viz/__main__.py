"""Draw saved frame outputs as PNG images.

    python -m pasco_amd.viz --outputs DIR --config <semantic-kitti.yaml> --save-folder OUT
                            [--views semantic,panoptic,mask,vox_conf,ins_conf] [--scales 1,2,4] [--camera behind|top|oblique]
                            [--size 1400] [--supersample 2] [--filter median|max|avg|raw] [--device cuda|cpu] [--method NAME]

DIR holds `<frame>_<i>.pkl` as `python -m pasco_amd.eval.kitti --save-outputs DIR` writes them.  `--device cuda` renders with
the pv_* kernels, `--device cpu` with their numpy restatement; both write the same files, byte for byte.
"""
from __future__ import annotations

import argparse
import os
import pickle
import re

from .camera import PRESETS
from .frames import VIEW_NAMES, DeviceOps, HostOps, frame_images
from .palette import label_palette, ramp_palette
from .png import write_png


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--outputs", required=True, help="directory of <frame>_<i>.pkl")
    ap.add_argument("--config", required=True, help="the dataset yaml (color_map, learning_map_inv)")
    ap.add_argument("--save-folder", required=True)
    ap.add_argument("--views", default=",".join(VIEW_NAMES))
    ap.add_argument("--scales", default="1,2,4")
    ap.add_argument("--camera", default="behind", choices=PRESETS)
    ap.add_argument("--size", type=int, default=1400)
    ap.add_argument("--supersample", type=int, default=2)
    ap.add_argument("--filter", default="median", choices=("median", "max", "avg", "raw"))
    ap.add_argument("--device", default="cuda", choices=("cuda", "cpu"))
    ap.add_argument("--method", default="pasco_single", help="the prefix of the file names")
    a = ap.parse_args(argv)
    views = [v for v in a.views.split(",") if v]
    scales = [int(s) for s in a.scales.split(",") if s]
    if any(v not in VIEW_NAMES for v in views):
        ap.error(f"--views: any of {', '.join(VIEW_NAMES)}")
    if any(s not in (1, 2, 4, 8) for s in scales):
        ap.error("--scales: any of 1, 2, 4, 8")
    ops = (DeviceOps if a.device == "cuda" else HostOps)(label_palette(a.config), ramp_palette())
    os.makedirs(a.save_folder, exist_ok=True)
    names = sorted(f for f in os.listdir(a.outputs) if re.fullmatch(r".+_\d+\.pkl", f))
    if not names:
        raise FileNotFoundError(f"no <frame>_<i>.pkl under {a.outputs}")
    for name in names:
        frame, i = name[:-len(".pkl")].rsplit("_", 1)
        with open(os.path.join(a.outputs, name), "rb") as f:
            pred = pickle.load(f)
        for out_name, img in frame_images(pred, ops, a.method, frame, int(i), views, scales, a.camera, a.size, a.supersample,
                                          a.filter):
            write_png(os.path.join(a.save_folder, out_name), img)
            print(os.path.join(a.save_folder, out_name))


if __name__ == "__main__":
    main()
