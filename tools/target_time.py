"""The training targets of one batch - M = 3 subnets of a 256 x 256 x 32 frame, each under its own augmentation transform, with
and without the training crop - on the `pt_*` kernels (pasco_amd/data/targets.py `prepare_targets`) against the host
restatement (`semantic_kitti.build_train_item`'s target part: `transformed_labels`, the crop, `dense_labels`,
`multiscale_labels`, `mask_targets`), and against `transformed_labels` alone, which is what the host path of the parent commit
already paid per subnet for the bounds.

    python tools/target_time.py [--reps 100] [--windows 5] [--host-reps 3] [--out profiles/target_time.json]

The frame is synthetic and seeded: a ground sheet, 19 mixed classes over 12 % of the volume, 30 boxes with instance ids, an
unknown shell.  The transforms are `data.augment.random_transformation` draws (seeds 1..3).  Device side: wall clock around a call
that ends in its own host reads (it cannot be timed with events alone: the scene sizes come from the first read), median over
`windows` windows of `reps` calls after warm-up, min and max alongside; the five kernels' stages with device events.  Host side:
the median of `host-reps` calls.  Both sides' outputs are compared at this size and the number of differing voxels is reported
(a .5 rounding tie of the coordinate chain may differ between torch's CPU matmul and the device's fmaf chain: DESIGN.md 4d)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pasco_amd.data import semantic_kitti as SK  # noqa: E402
from pasco_amd.data.augment import random_transformation  # noqa: E402

GRID = (256, 256, 32)
M = 3


def frame(seed=0):
    rng = np.random.default_rng(seed)
    sem = np.full(GRID, 255, np.uint8)
    sem[2:250, 4:252, 0:30] = 0
    sem[2:250, 4:252, 0:3] = 9
    mix = (rng.random(GRID) < 0.12) & (sem == 0)
    sem[mix] = rng.integers(9, 20, GRID, dtype=np.uint8)[mix]
    ins = np.zeros(GRID, np.uint8)
    for k in range(1, 31):
        x, y = int(rng.integers(6, 236)), int(rng.integers(8, 236))
        sem[x:x + 10, y:y + 8, 3:9] = 1 + k % 8
        ins[x:x + 10, y:y + 8, 3:9] = k
    return sem, ins


def wall(fn, reps, windows, warm=2, sync=None):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(windows):
        if sync:
            sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        if sync:
            sync()
        ts.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def events(fn, reps, windows, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(windows):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return {"ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def host_targets(sem, ins, T, u):
    """The target part of `build_train_item` (no points)."""
    sem_f, sem_c, ins_f, ins_c, _, _ = SK.transformed_labels(sem, ins, T, 8)
    if u is not None:
        w = SK.crop_window(sem_c, u)
        ks, ki = SK.in_window(sem_c, w), SK.in_window(ins_c, w)
        sem_f, sem_c, ins_f, ins_c = sem_f[ks], sem_c[ks], ins_f[ki], ins_c[ki]
    lo, hi = sem_c.min(0)[0], sem_c.max(0)[0]
    if ins_c.shape[0] > 0:
        lo, hi = torch.min(lo, ins_c.min(0)[0]), torch.max(hi, ins_c.max(0)[0])
    min_c, max_c = SK.completion_bounds(lo, hi, 8)
    s, i = SK.dense_labels(sem_f, sem_c, ins_f, ins_c, min_c, SK.compute_scene_size(min_c, max_c, scale=8))
    geo, lab = SK.multiscale_labels(s, 20)
    return {"min_C": min_c, "semantic_label": s, "instance_label": i, "geo_labels": geo, "sem_labels": lab,
            "mask_label": SK.mask_targets(s, i)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("tools/target_time.py measures on the GPU; none found")
        return 1
    from pasco_amd.data.frame_lib import box_upper_bound
    from pasco_amd.data.target_lib import BOUNDS, CROP_BOUNDS, TABLE, target_lib
    from pasco_amd.data.targets import prepare_targets
    dev = torch.device("cuda", 0)
    sem, ins = frame()
    Ts = [random_transformation(np.random.RandomState(s)) for s in (1, 2, 3)]
    us = np.random.RandomState(7).rand(M, 3)
    d_sem, d_ins = torch.from_numpy(sem).to(dev), torch.from_numpy(ins).to(dev)
    sync = torch.cuda.synchronize
    results = {"grid": list(GRID), "M": M}

    t0 = time.perf_counter()
    for T in Ts:
        SK.transformed_labels(sem, ins, T, 8)
    results["host_transformed_labels_parent"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "calls": M,
                                                 "note": "bounds only: what the parent's host path computes per batch"}
    for tag, crop in (("no_crop", None), ("crop", us)):
        def device_call():
            return prepare_targets(d_sem, d_ins, Ts, thing_ids=SK.SEMANTIC_KITTI_THING_IDS, crop_u=crop)

        def device_with_masks():
            return [t["mask_label"]["masks"] for t in device_call()]

        got = device_call()
        rec = {"device": wall(device_call, a.reps, a.windows, sync=sync),
               "device_with_masks": wall(device_with_masks, a.reps, a.windows, sync=sync),
               "targets": [int(t["mask_label"]["labels"].numel()) for t in got],
               "scene": [list(t["semantic_label"].shape) for t in got]}
        hs = []
        for _ in range(a.host_reps):
            t0 = time.perf_counter()
            host = [host_targets(sem, ins, T, None if crop is None else crop[m]) for m, T in enumerate(Ts)]
            hs.append((time.perf_counter() - t0) * 1e3)
        rec["host"] = {"ms": round(float(np.median(hs)), 1), "min_ms": round(min(hs), 1), "max_ms": round(max(hs), 1)}
        rec["host_over_device"] = round(rec["host"]["ms"] / rec["device"]["ms"], 1)
        rec["host_over_device_with_masks"] = round(rec["host"]["ms"] / rec["device_with_masks"]["ms"], 1)
        diff = {}
        for m, (g, h) in enumerate(zip(got, host)):
            if not torch.equal(g["min_C"], h["min_C"]) or g["semantic_label"].shape != h["semantic_label"].shape:
                diff[m] = "bounds differ"
                continue
            diff[m] = {"semantic": int((g["semantic_label"].cpu() != h["semantic_label"]).sum()),
                       "instance": int((g["instance_label"].cpu() != h["instance_label"]).sum()),
                       "sem_1_2": int((g["sem_labels"]["1_2"].cpu() != h["sem_labels"]["1_2"]).sum()),
                       "sem_1_4": int((g["sem_labels"]["1_4"].cpu() != h["sem_labels"]["1_4"]).sum()),
                       "geo_1_4": int((g["geo_labels"]["1_4"].cpu() != h["geo_labels"]["1_4"]).sum()),
                       "labels_equal": bool(torch.equal(g["mask_label"]["labels"].cpu(), h["mask_label"]["labels"])),
                       "voxels": int(h["semantic_label"].numel())}
        rec["differing_voxels_host_vs_device"] = diff
        results[tag] = rec

    # the stages alone, device time (crop case)
    L = target_lib()
    Tf = [T.float() for T in Ts]
    Ti = [torch.inverse(T) for T in Tf]
    ub = box_upper_bound(GRID, Tf)
    stride = (int((ub[:, 3:] - ub[:, :3] + 1).long().prod(dim=1).max()) + 15) // 16 * 16
    sb, ib = torch.empty((M, stride), dtype=torch.uint8, device=dev), torch.empty((M, stride), dtype=torch.uint8, device=dev)
    bounds = torch.empty((M, BOUNDS), dtype=torch.int32, device=dev)
    L.resample(d_sem, d_ins, Tf, Ti, ub, sb, ib, bounds)
    hb = bounds.cpu()
    win = torch.stack([SK.crop_window_from_bounds(hb[m, 6:9], hb[m, 9:12], us[m]) for m in range(M)])
    cb = torch.empty((M, CROP_BOUNDS), dtype=torch.int32, device=dev)
    got = prepare_targets(d_sem, d_ins, Ts, thing_ids=SK.SEMANTIC_KITTI_THING_IDS, crop_u=us)
    outs = [{"semantic": t["semantic_label"], "instance": t["instance_label"], "geo_1": t["geo_labels"]["1_1"],
             "geo_2": t["geo_labels"]["1_2"], "geo_4": t["geo_labels"]["1_4"], "sem_2": t["sem_labels"]["1_2"],
             "sem_4": t["sem_labels"]["1_4"], "min_C": t["min_C"].tolist(), "scene": list(t["semantic_label"].shape)} for t in got]
    tables = torch.empty((M, TABLE), dtype=torch.int32, device=dev)
    ml = got[0]["mask_label"]
    semantic, instance, cls_slot, ins_slot = ml._grids
    xyz = torch.nonzero(semantic != 255)[::4]
    coords = torch.cat([torch.zeros((xyz.shape[0], 1), dtype=torch.long, device=dev), xyz + got[0]["min_C"].to(dev)], 1).to(torch.int32)
    masks = ml["masks"]
    from pasco_amd.grad.criterion import pack_targets
    origin = got[0]["min_C"].tolist()
    results["stages_device"] = {
        "pt_resample": events(lambda: L.resample(d_sem, d_ins, Tf, Ti, ub, sb, ib, bounds), a.reps, a.windows),
        "pt_crop_bounds": events(lambda: L.crop_bounds(sb, ib, ub, win, cb), a.reps, a.windows),
        "pt_labels": events(lambda: L.labels(sb, ib, ub, win, outs, 20, tables), a.reps, a.windows),
        "pt_masks_subnet0": events(lambda: L.masks(semantic, instance, cls_slot, ins_slot, ml.t), a.reps, a.windows),
        "pt_target_pack_subnet0": events(lambda: ml.pack(coords, None, origin), a.reps, a.windows),
        "pm_target_pack_subnet0": events(lambda: pack_targets(masks, None, coords, origin), a.reps, a.windows),
        "rows": int(coords.shape[0]), "targets_subnet0": ml.t, "box_cells": [int(v) for v in (ub[:, 3:] - ub[:, :3] + 1).long().prod(dim=1)],
        "mask_bytes_subnet0": int(masks.numel())}
    print("TARGET_TIME " + json.dumps(results), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/target_time.py", "device": "MI355X", "reps": a.reps, "windows": a.windows,
                       "host_reps": a.host_reps, "results": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
