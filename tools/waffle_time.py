"""Time the point-feature stage on one synthetic full-size scan: every stage of the kernel route, the total, and the same
network as `pasco_amd.waffle.host.forward`'s plain torch formulation on the same GPU.

    python tools/waffle_time.py [--points 120000] [--channels 256] [--depth 48] [--repeats 5] [--out profiles/waffle_time.json]

The scan has SemanticKITTI's extent (a ground sheet, walls and clutter out to 60 m, so part of it lies outside the field of
view), the net seeded random weights with the published geometry (grids 250 x 250, 250 x 12, 250 x 12, 16 neighbours), one
vote.  Device events around each stage, 1 warm-up call + `--repeats` timed ones, median (min - max).  The 48 layers are timed
as one run of all spatial mixes and one of all channel mixes on the same tokens (the stages do not depend on the values).
Needs the MI355X; there is no fallback."""
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


def synthetic_scan(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    r = 60.0 * np.sqrt(rng.random(n)) ** 1.5                      # denser near the sensor, as a rotating scanner sees it
    phi = rng.uniform(-np.pi, np.pi, n)
    kind = rng.random(n)
    z = np.where(kind < 0.6, rng.normal(-1.7, 0.05, n), rng.uniform(-1.7, 1.9, n))
    xyz = np.stack([r * np.cos(phi), r * np.sin(phi), z], 1)
    return np.concatenate([xyz, rng.random((n, 1))], 1).astype(np.float32)


def random_state(C: int, depth: int, cin: int = 5, classes: int = 19, seed: int = 0):
    from pasco_amd.waffle.net import _Segmenter
    torch.manual_seed(seed)
    tree = _Segmenter(cin, C, classes, depth)
    st = tree.state_dict()
    for k, v in st.items():
        if k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape))
        elif k.endswith("running_mean"):
            v.copy_(0.3 * torch.randn(v.shape))
        elif ".scale." in k:
            v.copy_(0.1 + 0.05 * torch.randn(v.shape))
    return st


def timed(fn, repeats: int):
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


def wall(fn, repeats: int):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("waffle_time.py needs the MI355X")
    from pasco_amd.waffle import WaffleNet, host, prep
    from pasco_amd.waffle.lib import waffle_lib
    dev = torch.device("cuda", 0)
    L = waffle_lib()
    cfg = prep.settings({"waffleiron": {"nb_channels": a.channels, "depth": a.depth, "fov_xyz": [[-50, -50, -3], [50, 50, 2]],
                                        "dim_proj": [2, 1, 0], "grids_size": [[250, 250], [250, 12], [250, 12]]},
                         "classif": {"nb_class": 19},
                         "embedding": {"input_feat": ["intensity", "xyz", "radius"], "neighbors": 16, "voxel_size": 0.1}})
    pc = prep.input_features(synthetic_scan(a.points), cfg["input_feat"])
    net = WaffleNet(random_state(a.channels, a.depth), cfg["grids"], dev)
    it = prep.prepare_device(pc, cfg, dev)
    feat, cells, knn = it["feat"], it["cells"], it["knn"]
    N = int(feat.shape[0])
    res = {"points": a.points, "kept": N, "channels": a.channels, "depth": a.depth, "repeats": a.repeats,
           "search_grid": {"h": it["grid"].h, "cells": list(it["grid"].G)}, "stages": {}}
    s = res["stages"]
    s["preparation (upload, voxel, crop, cells, CSR, kNN, nearest)"] = wall(lambda: prep.prepare_device(pc, cfg, dev), a.repeats)
    cur = torch.from_numpy(pc).to(dev)[it["kept"]].contiguous()
    d_pc = torch.from_numpy(pc).to(dev)
    status = L.new_status(dev)
    g = it["grid"]
    sstart, sorder = L.cells_build(L.grid_cells(cur, g, status), g.ncell, status)
    s["pw_knn k=16"] = timed(lambda: L.knn(cur, sstart, sorder, g, 16), a.repeats)
    s["pw_nearest"] = timed(lambda: L.nearest(cur, sstart, sorder, g, d_pc), a.repeats)
    with torch.no_grad():
        s["embedding"] = timed(lambda: net.embedding(feat, knn, status), a.repeats)
        tokens = net.embedding(feat, knn, status).clone()
        most = max(H * W for _, _, _, (H, W) in cells)
        bufs = [torch.empty((most, net.C), dtype=torch.float32, device=dev) for _ in range(2)]

        def spatial():
            t = tokens.clone()
            for d, layer in enumerate(net.layers):
                net.spatial_mix(t, layer, cells[d % len(cells)], status, bufs)

        def channel():
            for layer in net.layers:
                net.channel_mix(tokens, layer)

        s[f"{a.depth} spatial mixes"] = timed(spatial, a.repeats)
        s[f"{a.depth} channel mixes"] = timed(channel, a.repeats)
        from pasco_amd.waffle.net import linear
        s["classifier"] = timed(lambda: linear(tokens, net.classif), a.repeats)
        res["network_kernels"] = wall(lambda: net.forward(feat, cells, knn), a.repeats)
        res["network_torch"] = wall(lambda: net.forward_host(feat, cells, knn), a.repeats)
        k_out = net.forward(feat, cells, knn)
        t_out = net.forward_host(feat, cells, knn)
    res["kernels_against_torch"] = {n: float((x - y).abs().max() / max(1.0, float(y.abs().max())))
                                    for n, x, y in zip(("embedding", "tokens", "logits"), k_out, t_out)}
    res["status"] = int(status.item())
    res["total_ms"] = s["preparation (upload, voxel, crop, cells, CSR, kNN, nearest)"]["median_ms"] + res["network_kernels"]["median_ms"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
