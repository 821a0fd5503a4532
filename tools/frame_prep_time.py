"""Frame preparation: host restatement vs the pf_* kernels, on a synthetic full-size frame (256 x 256 x 32 label grids,
120 k points), for both datasets at M = 1, 2, 3 subnets.

    python tools/frame_prep_time.py [--points 120000] [--reps 5]

Per dataset and M it prints one JSON line: `kernels_ms` (the pf_* launches alone, device events, inputs already on the device),
`device_batch_ms` / `host_batch_ms` (the whole preparation from host arrays to the collated batch, wall clock; file reading
excluded on both sides) and their ratio."""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synthetic_frame(n, rng):
    grid = (256, 256, 32)
    sem = rng.integers(0, 19, grid).astype(np.uint8)
    sem[:, :, 18:] = 0
    sem[rng.random(grid) < 0.3] = 255
    ins = np.zeros(grid, np.uint8)
    ins[100:120, 40:60, 2:8] = 3
    ins[180:190, 200:230, 2:6] = 7
    xyz = np.stack([rng.uniform(-10, 60, n), rng.uniform(-30, 30, n), rng.uniform(-3, 5, n)], 1)
    pc = np.concatenate([xyz, rng.random((n, 1))], 1).astype(np.float32)
    return pc, sem, ins


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts))


def kernels_only(lib, pts, args, segs_keep, sem, ins, Ts, reps):
    from pasco_amd.data.frame_lib import box_upper_bound
    n, M, dev = int(pts.shape[0]), len(Ts), pts.device
    feat = torch.empty((n, lib.channels(args)), dtype=torch.float32, device=dev)
    vox = torch.empty((n, 3), dtype=torch.float64, device=dev)
    kept = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(max(int(lib.lib.pf_points_workspace_bytes(n)), 4), dtype=torch.uint8, device=dev)
    out = torch.empty((M, n, 3), dtype=torch.int64, device=dev)
    bounds = torch.empty((M, 12), dtype=torch.int32, device=dev)
    Tinv = [torch.inverse(T) for T in Ts]
    bb = box_upper_bound(tuple(sem.shape), Ts)

    def run():
        lib.points_into(pts, args, feat, vox, None, kept, ws)
        lib.transform_coords(vox, Ts, n_dev=kept, out=out)
        lib.label_bounds(sem, ins, Ts, Tinv, bb, out=bounds)

    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from pasco_amd.data import build_item, build_item_kitti360, collate
    from pasco_amd.data.frame_lib import _seg, frame_lib, segment
    from pasco_amd.data.kitti360 import MAX_EXTENT as K_HI, MIN_EXTENT as K_LO, prepare_kitti360_on_device
    from pasco_amd.data.semantic_kitti import (MAX_EXTENT, MIN_EXTENT, VOX_ORIGIN, prepare_semantic_kitti_on_device)
    from pasco_amd.eval.kitti import subnet_transforms
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    pc, sem, ins = synthetic_frame(a.points, rng)
    lib = frame_lib()
    sem_d, ins_d, pts_d = torch.from_numpy(sem).to(dev), torch.from_numpy(ins).to(dev), torch.from_numpy(pc).to(dev)
    P = pc.shape[0]
    vote, emb = rng.random((P, 19)).astype(np.float32), rng.standard_normal((2, 256, P)).astype(np.float32)
    tmp = tempfile.mkdtemp()
    wpath = os.path.join(tmp, "w.pkl")
    with open(wpath, "wb") as f:
        pickle.dump({"embedding": emb, "coords": pc, "vote": vote}, f)
    vote_d, emb_d = torch.from_numpy(vote).to(dev), torch.from_numpy(np.ascontiguousarray(emb[0])).to(dev)
    for M in (1, 2, 3):
        Ts = subnet_transforms(M)
        # KITTI-360
        args = lib.points_args(K_LO, K_HI, (1, 1, 1), (0, 0, 0), VOX_ORIGIN, 0.2, True, [_seg(pts_d[:, 3:], 1, 4, 1)])
        k_ms = kernels_only(lib, pts_d, args, None, sem_d, ins_d, Ts, a.reps)
        d_ms = wall(lambda: prepare_kitti360_on_device(pc, sem, ins, Ts, dev), a.reps)
        h_ms = wall(lambda: collate([build_item_kitti360(pc, sem, ins, T) for T in Ts]), max(1, a.reps // 2))
        print(json.dumps({"dataset": "kitti360", "M": M, "points": P, "kernels_ms": round(k_ms, 4),
                          "device_batch_ms": round(d_ms, 3), "host_batch_ms": round(h_ms, 1),
                          "speedup": round(h_ms / d_ms, 1)}), flush=True)
        # SemanticKITTI (283 channels)
        args = lib.points_args(MIN_EXTENT, MAX_EXTENT, (0, 0, 0), (0, 0, 0), VOX_ORIGIN, 0.2, False,
                               [segment(vote_d), _seg(pts_d[:, 3:], 1, 4, 1)], [_seg(emb_d, 256, 1, P)])
        k_ms = kernels_only(lib, pts_d, args, None, sem_d, ins_d, Ts, a.reps)
        d_ms = wall(lambda: prepare_semantic_kitti_on_device(wpath, sem, ins, Ts, dev), a.reps)
        xyz, inten, e = pc[:, :3], pc[:, 3:], emb[0].T
        h_ms = wall(lambda: collate([build_item(xyz, vote, inten, e, sem, ins, T) for T in Ts]), max(1, a.reps // 2))
        print(json.dumps({"dataset": "semantic_kitti", "M": M, "points": P, "kernels_ms": round(k_ms, 4),
                          "device_batch_ms": round(d_ms, 3), "host_batch_ms": round(h_ms, 1),
                          "speedup": round(h_ms / d_ms, 1), "note": "device_batch_ms includes unpickling the features"}),
              flush=True)


if __name__ == "__main__":
    main()
