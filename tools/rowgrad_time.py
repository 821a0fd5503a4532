"""Backward of `SparseTensor.dense()` and `ME.to_sparse()`: the two tile-transpose kernels of include/pasco_rowgrad.h against
(a) torch autograd of the index formulation and (b) the forward kernel of include/pasco_hip.h that moves the same bytes in the
thread-per-(row, channel) layout (`ph_dense_gather` for `pr_dense_rows`, `ph_to_dense` for `pr_rows_dense`), on the same GPU.

    python tools/rowgrad_time.py [--reps 20] [--windows 5] [--out profiles/rowgrad_time.json]

Shapes: "merge" = Augmenter.merge at the benchmark's scene, B = 3, C = 32, 256 x 256 x 32 with the synthetic scene's
full-resolution rows (pasco_amd/graph/synth.py) in to_sparse order; "bottleneck" = B = 1, C = 256, 32 x 32 x 4, every site.
Method of tools/grad_time.py: the median over `windows` device-event windows of `reps` calls each, after warm-up calls (min and
max alongside).  Bytes are the algorithm's own: the rows read and written (n * C * 4 each way) plus the coordinates (16 n), and for
the dense-writing direction the zero fill of the grid; the share is of 8 TB/s."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_time import PEAK_HBM, device_timer  # noqa: E402


def merge_shape(dev):
    from pasco_amd.graph.synth import make_occupancy
    parts = []
    for b in range(3):
        c = np.argwhere(make_occupancy(b)).astype(np.int32)            # lexicographic (x, y, z): to_sparse order
        parts.append(np.concatenate([np.full((len(c), 1), b, np.int32), c], 1))
    return "merge", (3, 32, 256, 256, 32), torch.from_numpy(np.ascontiguousarray(np.concatenate(parts))).to(dev)


def bottleneck_shape(dev):
    c = np.argwhere(np.ones((1, 32, 32, 4), dtype=bool)).astype(np.int32)
    return "bottleneck", (1, 256, 32, 32, 4), torch.from_numpy(np.ascontiguousarray(c)).to(dev)


def rate(nbytes, ms):
    return {"bytes": int(nbytes), "gbs": round(nbytes / (ms * 1e-3) / 1e9, 1), "share_of_8tbs": round(nbytes / PEAK_HBM / (ms * 1e-3), 4)}


def run_shape(name, shape5, sites, be, lib, timer):
    B, C, X, Y, Z = shape5
    n = int(sites.shape[0])
    dev = sites.device
    g = torch.Generator().manual_seed(n)
    dense = torch.randn(shape5, generator=g).to(dev)
    rows = torch.randn((n, C), generator=g).to(dev)
    b, x, y, z = (sites[:, a].long() for a in range(4))
    rec = {"shape": name, "B": B, "C": C, "grid": [X, Y, Z], "rows": n}
    row_bytes = 2.0 * n * C * 4 + 16.0 * n
    fill_bytes = 4.0 * B * C * X * Y * Z

    # pr_dense_rows: the backward of dense(); g = `dense`
    out = torch.empty((n, C), device=dev)
    rec["dense_rows"] = timer(lambda: lib.dense_rows(dense, sites, (0, 0, 0), 1, out=out))
    feats = rows.clone().requires_grad_(True)
    fwd = torch.zeros((B, X, Y, Z, C), device=dev).index_put((b, x, y, z), feats).permute(0, 4, 1, 2, 3)
    rec["dense_rows_torch_autograd"] = timer(lambda: torch.autograd.grad(fwd, feats, dense, retain_graph=True))
    rec["dense_rows_thread_per_element"] = timer(lambda: be.dense_gather(dense, sites))
    assert torch.equal(out, torch.autograd.grad(fwd, feats, dense, retain_graph=True)[0])
    assert torch.equal(out, be.dense_gather(dense, sites))
    del fwd, feats
    rec["dense_rows_rate"] = rate(row_bytes, rec["dense_rows"]["ms"])

    # pr_rows_dense: the backward of to_sparse(); g = `rows`
    grid = torch.empty(shape5, device=dev)
    rec["rows_dense"] = timer(lambda: lib.rows_dense(rows, sites, shape5, out=grid))
    src = dense.clone().requires_grad_(True)
    gathered = src[b, :, x, y, z]
    rec["rows_dense_torch_autograd"] = timer(lambda: torch.autograd.grad(gathered, src, rows, retain_graph=True))
    rec["rows_dense_thread_per_element"] = timer(lambda: be.to_dense(rows, sites, (0, 0, 0), 1, (B, X, Y, Z)))
    assert torch.equal(grid, torch.autograd.grad(gathered, src, rows, retain_graph=True)[0])
    assert torch.equal(grid, be.to_dense(rows, sites, (0, 0, 0), 1, (B, X, Y, Z)))
    rec["rows_dense_fill_only"] = timer(lambda: grid.zero_())
    rec["rows_dense_rate"] = rate(row_bytes + fill_bytes, rec["rows_dense"]["ms"])
    for k in ("dense_rows", "rows_dense"):
        for other in ("torch_autograd", "thread_per_element"):
            rec[f"{k}_ratio_{other}_over_kernel"] = round(rec[f"{k}_{other}"]["ms"] / rec[k]["ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "rowgrad_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "rowgrad_time.py measures on the GPU; there is nothing to report without one"
    from pasco_amd.grad.rowlib import rowgrad_lib
    from pasco_amd.me.backend import hip_backend
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "shapes": []}
    for make in (merge_shape, bottleneck_shape):
        name, shape5, sites = make(dev)
        rec = run_shape(name, shape5, sites, hip_backend(), rowgrad_lib(), lambda fn: device_timer(fn, a.reps, a.windows))
        print(json.dumps(rec), flush=True)
        out["shapes"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
