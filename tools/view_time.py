"""Time the drawing of one full-size frame (all five views, three scales) on the device and, on request, on the host.

    python tools/view_time.py [--repeats 10] [--size 1400] [--supersample 2] [--cpu-size N] [--out profiles/view_time.json]

(i)   every pv_* kernel alone on the frame's grids: device events, 3 warm-up calls + `--repeats` timed ones, median (min - max);
(ii)  the whole frame through `viz.frame_images` on the device: a host clock around work that ends in the device-to-host copy
      of each image, 1 warm-up frame + `--repeats` timed ones;
(iii) with `--cpu-size N`, the same frame at N x N pixels without supersampling through the numpy restatement, once, and
      through the device at that size for the comparison (the restatement walks every ray in numpy: minutes at full size).
The frame is the seeded blob scene of tests/view_cases.py with 128 segments.  Needs the MI355X; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CONFIG = os.path.join(ROOT, "tests", "golden", "semantic-kitti.yaml")


def frame(shape=(256, 256, 32), n_seg=128):
    import view_cases as VC
    from pasco_amd import viz
    rng = np.random.default_rng(0)
    sem = VC.blob_labels(11, shape, unknown=0.0)
    pan = (rng.integers(1, n_seg + 1, shape) * ((sem > 0) & (sem < 9))).astype(np.int32)
    infos = [{"id": s + 1, "isthing": True, "category_id": 1 + s % 8, "confidence": float(rng.random())} for s in range(n_seg)]
    return viz.frame_record(sem, pan, infos, rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32), None,
                            pan, [], VC.blob_labels(12, shape), pan)


def timed(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--size", type=int, default=1400)
    ap.add_argument("--supersample", type=int, default=2)
    ap.add_argument("--cpu-size", type=int, default=0, help="also run the frame at N x N through the numpy restatement")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("view_time.py needs the MI355X")
    from pasco_amd import viz
    from pasco_amd.viz.frames import BACKGROUND, FACE_FACTORS, segment_table
    from pasco_amd.viz.lib import view_lib
    lib, dev = view_lib(), torch.device("cuda", 0)
    rec = frame()
    shape = rec["pred_panoptic_seg"].shape[1:]
    sem = torch.from_numpy(rec["ssc_pred"][0].astype(np.uint8)).to(dev)
    pan = torch.from_numpy(rec["pred_panoptic_seg"][0]).to(dev)
    conf = torch.from_numpy(rec["vox_confidence_denses"][0]).to(dev)
    seg = torch.from_numpy(segment_table(rec["pred_segments_info"][0])).to(dev)
    pal = torch.from_numpy(viz.label_palette(CONFIG)).to(dev)
    n = a.size * a.supersample
    cam = torch.from_numpy(viz.preset("behind", shape, n, n)).to(dev)
    colour = lib.compose("panoptic", shape, panoptic=pan, seg=seg, sem=sem)
    bits = lib.bricks(colour)
    rgb = lib.render(colour, bits, cam, n, n, pal, FACE_FACTORS, BACKGROUND)[2]
    res = {"grid": list(shape), "image": [n, n], "supersample": a.supersample, "repeats": a.repeats, "kernels": {}}
    k = res["kernels"]
    for kk in (2, 4):
        k[f"pv_majority_pool k={kk}"] = timed(lambda: lib.majority_pool(sem, kk), a.repeats)
    for op in ("median", "max", "avg"):
        k[f"pv_window_filter {op}"] = timed(lambda: lib.window_filter(conf, op, sem), a.repeats)
    for view, kw in (("semantic", dict(sem=sem)), ("panoptic", dict(panoptic=pan, seg=seg, sem=sem)),
                     ("vox_conf", dict(sem=sem, conf=conf)), ("ins_conf", dict(panoptic=pan, seg=seg))):
        k[f"pv_compose {view}"] = timed(lambda: lib.compose(view, shape, out=colour, **kw), a.repeats)
    lib.compose("panoptic", shape, panoptic=pan, seg=seg, sem=sem, out=colour)
    k["pv_bricks"] = timed(lambda: lib.bricks(colour, out=bits), a.repeats)
    k[f"pv_render {n}x{n}"] = timed(lambda: lib.render(colour, bits, cam, n, n, pal, FACE_FACTORS, BACKGROUND), a.repeats)
    k[f"pv_downsample s={a.supersample}"] = timed(lambda: lib.downsample(rgb, a.supersample), a.repeats)

    def whole(ops, size=a.size, supersample=a.supersample):
        t0 = time.perf_counter()
        count = sum(1 for _ in viz.frame_images(rec, ops, "m", "000000", 1, size=size, supersample=supersample))
        return 1e3 * (time.perf_counter() - t0), count

    ops = viz.DeviceOps(viz.label_palette(CONFIG), viz.ramp_palette())
    whole(ops)
    torch.cuda.synchronize()
    runs = [whole(ops) for _ in range(a.repeats)]
    ms = [r[0] for r in runs]
    res["frame_device"] = {"images": runs[0][1], "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    if a.cpu_size:
        whole(ops, a.cpu_size, 1)
        res["frame_device_small"] = {"image": [a.cpu_size, a.cpu_size], "ms": whole(ops, a.cpu_size, 1)[0]}
        ms, count = whole(viz.HostOps(viz.label_palette(CONFIG), viz.ramp_palette()), a.cpu_size, 1)
        res["frame_host_small"] = {"image": [a.cpu_size, a.cpu_size], "images": count, "ms": ms}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
