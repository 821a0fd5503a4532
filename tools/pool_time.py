"""The pooling / broadcast / channel-wise kernels of include/pasco_pool.h, forward and backward, against their torch restatement
(pasco_amd/grad/host.py pool_*, run on the same GPU tensors), at the four levels of the synthetic scene of tools/grad_time.py.

    python tools/pool_time.py [--reps 20] [--windows 5] [--out profiles/pool_time.json]

Level l = tensor stride 2^l of `make_occupancy(0)` with C = 32 << l channels; the per-batch operators see B = 3 batch indices dealt
out row by row (i % 3: the rows of one batch index are not contiguous).  Method of tools/grad_time.py: the median over `windows`
device-event windows of `reps` calls each, after warm-up calls (min and max alongside).  Bytes are the formula's own: every operand
row read once, every result row written once, the table or the coordinates read once; the share is of 8 TB/s.  There is no pass
mark: a shape at which the kernel is slower than the restatement is reported as such ("slower")."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_time import PEAK_HBM, device_timer, level_keys  # noqa: E402

B = 3


def rate(nbytes, ms):
    return {"bytes": int(nbytes), "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "share_of_8tbs": round(nbytes / PEAK_HBM / (ms * 1e-3), 4)}


def run_level(level, mgr, keys, L, H, G, timer):
    from pasco_amd.me.backend import hip_backend
    be = hip_backend()
    key = keys[level]
    n, c = mgr.size(key), 32 << level
    dev = mgr.get_coordinates(key).device
    g = torch.Generator().manual_seed(level)
    x, dy = torch.randn(n, c, generator=g).to(dev), torch.randn(n, c, generator=g).to(dev)
    coords = mgr.get_coordinates(key).clone()
    coords[:, 0] = torch.arange(n, device=dev, dtype=torch.int32) % B
    glob, dglob = torch.randn(B, c, generator=g).to(dev), torch.randn(B, c, generator=g).to(dev)
    rec = {"level": level, "rows": n, "C": c, "ops": {}}
    rows, crd = 4.0 * n * c, 16.0 * n

    def op(name, kernel, restated, nbytes):
        k, t = timer(kernel), timer(restated)
        rec["ops"][name] = {"kernel": k, "torch": t, "torch_over_kernel": round(t["ms"] / k["ms"], 2), **rate(nbytes, k["ms"]),
                            "slower": k["ms"] > t["ms"]}

    _, cnt, arg = L.seg_reduce(x, coords, B, H.POOL_MAX)
    op("global_avg", lambda: L.seg_reduce(x, coords, B, H.POOL_AVG), lambda: H.pool_seg_reduce(x, coords, B, H.POOL_AVG), rows + crd)
    op("global_avg_bwd", lambda: L.broadcast(None, dglob, coords, H.POOL_BC_COPY, cnt),
       lambda: H.pool_broadcast(None, dglob, coords, H.POOL_BC_COPY, cnt), rows + crd)
    idx = coords[:, :1].long().expand(n, c)
    op("global_max", lambda: L.seg_reduce(x, coords, B, H.POOL_MAX),
       lambda: torch.zeros((B, c), device=dev).scatter_reduce_(0, idx, x, "amax", include_self=False), rows + crd)
    op("global_max_bwd", lambda: L.seg_max_bwd(dglob, arg, n), lambda: H.pool_seg_max_bwd(dglob, arg, n), rows)
    op("broadcast_mul", lambda: L.broadcast(x, glob, coords, H.POOL_BC_MUL), lambda: H.pool_broadcast(x, glob, coords, H.POOL_BC_MUL),
       2 * rows + crd)
    op("broadcast_mul_bwd", lambda: L.broadcast_mul_bwd(dy, x, glob, coords), lambda: H.pool_broadcast_mul_bwd(dy, x, glob, coords),
       3 * rows + crd)
    op("broadcast_cat", lambda: L.broadcast(x, glob, coords, H.POOL_BC_CAT), lambda: H.pool_broadcast(x, glob, coords, H.POOL_BC_CAT),
       3 * rows + crd)
    dcat = torch.randn(n, 2 * c, generator=g).to(dev)
    op("broadcast_cat_bwd", lambda: L.seg_reduce(dcat[:, c:], coords, B, H.POOL_SUM),
       lambda: H.pool_seg_reduce(dcat[:, c:], coords, B, H.POOL_SUM), rows + crd)

    for label, ks, stride in (("k2s2", 2, 2), ("3^3", 3, 1)):
        if stride == 2 and level + 1 >= len(keys):
            continue
        out_key = keys[level + 1] if stride == 2 else key
        nbr = mgr.kernel_map(key, out_key, ks)
        K, n_out = nbr.shape
        inv = G.nbr_invert(nbr, n)
        dyo = torch.randn(n_out, c, generator=g).to(dev)
        table = 4.0 * K * n_out
        _, pc = L.pool(x, nbr, H.POOL_AVG)
        both = rows + 4.0 * n_out * c
        op(f"avg_pool_{label}", lambda: L.pool(x, nbr, H.POOL_AVG), lambda: H.pool_pool(x, nbr, H.POOL_AVG), both + table)
        op(f"avg_pool_{label}_bwd", lambda: L.pool_bwd(dyo, pc, inv, n, H.POOL_AVG), lambda: H.pool_pool_bwd(dyo, pc, inv, n, H.POOL_AVG),
           both + 4.0 * K * n)
        w, bias = torch.randn(K, c, generator=g).to(dev), torch.randn(c, generator=g).to(dev)
        op(f"chconv_{label}", lambda: L.chconv_fwd(x, nbr, w, bias), lambda: H.pool_chconv_fwd(x, nbr, w, bias), both + table)
        op(f"chconv_{label}_dgrad", lambda: L.chconv_fwd(dyo, inv, w, None), lambda: H.pool_chconv_fwd(dyo, inv, w, None),
           both + 4.0 * K * n)
        op(f"chconv_{label}_wgrad", lambda: L.chconv_wgrad(x, dyo, nbr), lambda: H.pool_chconv_wgrad(x, dyo, nbr), both + table)
        if stride == 2:                          # pooling transpose up from the coarser level: a gather; its backward a sum pooling
            parent = inv.max(dim=0).values.contiguous()          # the coarse row of every fine row
            up = torch.randn(n_out, c, generator=g).to(dev)
            op("pool_transpose_k2s2", lambda: be.gather_rows(up, parent), lambda: up[parent.long()], both + 4.0 * n)
            op("pool_transpose_k2s2_bwd", lambda: L.pool(dy, nbr, H.POOL_SUM), lambda: H.pool_pool(dy, nbr, H.POOL_SUM), both + table)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "pool_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pool_time.py measures on the GPU; there is nothing to report without one"
    import pasco_amd.grad as G
    from pasco_amd.grad import host as H
    from pasco_amd.grad.poollib import pool_lib
    from pasco_amd.graph.synth import make_occupancy
    from pasco_amd.me.core import CoordinateManager
    dev = torch.device("cuda", 0)
    c = np.argwhere(make_occupancy(0)).astype(np.int32)
    coords = torch.from_numpy(np.concatenate([np.zeros((len(c), 1), np.int32), c], 1)).to(dev)
    mgr = CoordinateManager(D=3, device=dev)
    key, _ = mgr.insert_and_map(coords, 1)
    keys = level_keys(mgr, key, 3)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "batch_indices": B,
           "rows_per_level": [mgr.size(k) for k in keys], "levels": []}
    for level in range(4):
        rec = run_level(level, mgr, keys, pool_lib(), H, G, lambda fn: device_timer(fn, a.reps, a.windows))
        print(json.dumps(rec), flush=True)
        out["levels"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
