"""The k-nearest-neighbour up-sampling of include/pasco_knn.h at a point-cloud segmenter's shape: the search, the weights and the
forward gather, and the backward, against a chunked torch brute force (`cdist` + `topk`) on the same GPU tensors.

    python tools/knn_time.py [--points 120000] [--k 3] [--reps 20] [--windows 5] [--out profiles/knn_time.json]

Workload: `points` points uniform in a 100 x 100 x 8 box (the aspect of a LiDAR sweep) against 80 000 / 20 000 / 5 000 voxels - that
many distinct cells, drawn at random, of a lattice over the same box with 60 % of its cells occupied - the three decoder levels a
MinkUNet carries back to the points.  k = 3.  Method of tools/field_time.py: the median over `windows` device-event windows of
`reps` calls each, after warm-up calls (min and max alongside).  `search` is pk_knn alone over a CSR built before; `csr` is that
build (pw_grid_cells + pq_group); `knn_up` is the whole module call, its one host read included.  The brute force is the one a
maintainer would write without these kernels: squared distances of a chunk of queries to every voxel (`torch.cdist`), `topk` of the
negated distances; it is not exact under the header's ordering rule and is timed, not compared.  Recorded beside them: pw_knn's
time for k = 16 on 105 k points, the repository's other exact grid search.  There is no pass mark: an entry at
which the device route is slower than the brute force is reported as such ("slower")."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_time import device_timer  # noqa: E402

VOXELS = (80000, 20000, 5000)
CHANNELS = (96, 256)
BOX = (100.0, 100.0, 8.0)
PW_KNN_MS_K16_105K = 1.11
CHUNK = 4096                     # queries of one brute-force chunk: 4096 x 80 000 distances = 1.3 GB


def clouds(points: int, voxels: int, seed: int = 0):
    g = torch.Generator().manual_seed(seed + voxels)
    box = torch.tensor(BOX)
    p = torch.rand(points, 3, generator=g) * box
    s = (float(box.prod()) * 0.6 / voxels) ** (1.0 / 3.0)
    dims = torch.ceil(box / s).long()
    cells = torch.randperm(int(dims.prod()), generator=g)[:voxels]
    assert cells.numel() == voxels
    v = torch.stack([cells % dims[0], (cells // dims[0]) % dims[1], cells // (dims[0] * dims[1])], dim=1).float() * s
    return v, p, s


def brute(v, p, k):
    out_d, out_i = [], []
    for a in range(0, p.shape[0], CHUNK):
        d = torch.cdist(p[a:a + CHUNK], v).square_()
        val, ind = torch.topk(d, k, dim=1, largest=False)
        out_d.append(val)
        out_i.append(ind)
    return torch.cat(out_d), torch.cat(out_i)


def run(points, voxels, k, reps, windows, dev):
    from pasco_amd.grad import knn as K
    from pasco_amd.grad.knnlib import knn_lib
    L = knn_lib()
    v, p, s = clouds(points, voxels)
    v, p = v.to(dev), p.to(dev)
    box = torch.stack(torch.aminmax(v, dim=0)).cpu()
    grid = K.search_grid(box[0].tolist(), box[1].tolist(), voxels)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    start, order = L.csr(v, grid, status)
    idx, d2 = L.knn(v, start, order, grid, p, k)
    assert int(status.item()) == 0 and bool((idx >= 0).all())
    bd, bi = brute(v, p, k)
    agree = float((bi.t() == idx.long()).float().mean())
    w = L.weights(d2, idx)
    timer = lambda fn, r=reps: device_timer(fn, r, windows)
    rec = {"voxels": voxels, "points": points, "k": k, "lattice_edge": round(s, 4), "grid": {"h": round(grid.h, 4), "cells": list(grid.G)},
           "voxels_per_cell": round(voxels / grid.ncell, 3), "selection_agrees_with_brute_force": round(agree, 6), "ops": {}}
    t_brute = timer(lambda: brute(v, p, k), max(2, reps // 10))
    rec["ops"]["brute_force_cdist_topk"] = t_brute
    for name, fn in (("search", lambda: L.knn(v, start, order, grid, p, k)), ("csr", lambda: L.csr(v, grid, status)),
                     ("search_with_csr", lambda: K.knn_search(v, p, k))):
        t = timer(fn)
        rec["ops"][name] = {**t, "brute_over_kernel": round(t_brute["ms"] / t["ms"], 2), "slower": t["ms"] > t_brute["ms"]}
    rec["ops"]["search"]["over_pw_knn_k16_105k"] = round(rec["ops"]["search"]["ms"] / PW_KNN_MS_K16_105K, 2)
    il, up = idx.long().t().contiguous(), K.knn_up(k)
    for c in CHANNELS:
        g = torch.Generator().manual_seed(c)
        x, dy = torch.randn(voxels, c, generator=g).to(dev), torch.randn(points, c, generator=g).to(dev)
        wt = w.t().contiguous()

        def torch_fwd():
            r = 1.0 / (bd + 1e-8)
            return (x[il] * (r / r.sum(dim=1, keepdim=True))[:, :, None]).sum(dim=1)

        def torch_bwd():
            return torch.zeros((voxels, c), device=dev).index_add_(0, il.reshape(-1), (wt[:, :, None] * dy[:, None, :]).reshape(-1, c))

        for name, fn, ref in ((f"weights_forward_C{c}", lambda: L.interp_fwd(x, idx, L.weights(d2, idx)), torch_fwd),
                              (f"backward_C{c}", lambda: L.interp_bwd(dy, idx, w, voxels), torch_bwd)):
            t, tt = timer(fn), timer(ref)
            rec["ops"][name] = {"kernel": t, "torch": tt, "torch_over_kernel": round(tt["ms"] / t["ms"], 2), "slower": t["ms"] > tt["ms"]}
        with torch.no_grad():
            rec["ops"][f"knn_up_C{c}"] = timer(lambda: up(v, x, p))
        del x, dy
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "knn_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "knn_time.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": a.points, "k": a.k,
           "pw_knn_ms_k16_105k_points": PW_KNN_MS_K16_105K, "shapes": []}
    for voxels in VOXELS:
        rec = run(a.points, voxels, a.k, a.reps, a.windows, dev)
        print(json.dumps(rec), flush=True)
        out["shapes"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
