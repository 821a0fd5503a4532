"""One (scale, subnet) call of the semantic completion losses, forward plus backward, on the `ps_*` kernels
(pasco_amd/grad/semloss.py) against the same call written in torch the way the training code it replaces writes it - a boolean
prune of the rows, the label gather, F.cross_entropy, and per class a mask, an error vector, a sort, two float cumsums, a
difference and a dot - on the same GPU, at C = 20 classes and N = 20 000, 80 000 and 300 000 rows (the orders of magnitude of
scales 4, 2 and 1 at the benchmark's occupancy) of a 256 x 256 x 32 grid, 10 % of the voxels labelled 255, 2 % of the rows outside
the box.

    python tools/sem_time.py [--reps 10] [--windows 5] [--out profiles/sem_time.json]

Every size runs in a child process of its own under a time limit (`--limit` seconds); the parent never opens the GPU and stops at
the first child that fails.  Wall-clock times are taken around a synchronised forward + backward (median over `windows` windows of
`reps` calls each, after warm-up; min and max alongside); the four stages of the kernel side are timed alone with device events.
Per size one JSON line: both sides, the ratio torch / kernel, the stages, the declared workspace, the peak device memory of one
call of each kind over the level before it, and the difference between the two sides' losses."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C = 20
DIMS = (256, 256, 32)
SIZES = (20000, 80000, 300000)


def wall_timer(fn, reps, windows, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def event_timer(fn, reps, windows, warm=3):
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


def torch_call(Fx, coords, target, min_C, max_C, scale, w):
    """The formulation of the training code, on the device of its inputs -> (ce, lovasz)."""
    xyz = coords[:, 1:4]
    keep = ((xyz <= max_C) & (xyz >= min_C)).all(dim=1)
    x = Fx[keep]
    idx = ((xyz[keep] - min_C) // scale).long()
    y = target[idx[:, 0], idx[:, 1], idx[:, 2]]
    ce = F.cross_entropy(x, y.long(), weight=w, ignore_index=255, reduction="mean")
    p = F.softmax(x, dim=1)
    losses = []
    for c in range(x.shape[1]):
        fg = (y == c).float()
        if fg.sum() == 0:
            continue
        err = (fg - p[:, c]).abs()
        err_sorted, perm = torch.sort(err, 0, descending=True)
        fgs = fg[perm]
        gts = fgs.sum()
        jac = 1.0 - (gts - fgs.cumsum(0)) / (gts + (1 - fgs).cumsum(0))
        jac[1:] = jac[1:] - jac[:-1]
        losses.append(torch.dot(err_sorted, jac))
    return ce, sum(losses) / len(losses)


def child(n, reps, windows):
    from pasco_amd.grad.semlib import sem_lib
    from pasco_amd.grad.semloss import sem_compl_loss
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n)
    Fx = (torch.randn(n, C, device=dev, generator=g) * 2).requires_grad_(True)
    target = torch.randint(0, C, DIMS, device=dev, generator=g).to(torch.uint8)
    target[torch.rand(DIMS, device=dev, generator=g) < 0.1] = 255
    pick = torch.randperm(DIMS[0] * DIMS[1] * DIMS[2], device=dev, generator=g)[:n]
    coords = torch.stack([torch.zeros_like(pick), pick // (DIMS[1] * DIMS[2]), (pick // DIMS[2]) % DIMS[1], pick % DIMS[2]], dim=1).to(torch.int32)
    coords[: n // 50, 1] += DIMS[0]
    min_C = torch.zeros(3, dtype=torch.int32, device=dev)
    max_C = torch.tensor([d - 1 for d in DIMS], dtype=torch.int32, device=dev)
    w = torch.rand(C, device=dev, generator=g) + 0.5
    L = sem_lib()

    def kernel_step():
        Fx.grad = None
        ce, lov = sem_compl_loss(Fx, coords, target, min_C, max_C, 1, w)
        (ce + lov).backward()
        return ce, lov

    def torch_step():
        Fx.grad = None
        ce, lov = torch_call(Fx, coords, target, min_C, max_C, 1, w)
        (ce + lov).backward()
        return ce, lov

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated(dev) - before)

    k_ce, k_lov = kernel_step()
    t_ce, t_lov = torch_step()
    res = {"n": n, "c": C, "rows_inside": int(n - n // 50), "workspace_bytes": L.workspace_bytes(n, C),
           "kernel": wall_timer(kernel_step, reps, windows), "torch": wall_timer(torch_step, reps, windows)}
    res["torch_over_kernel"] = round(res["torch"]["ms"] / res["kernel"]["ms"], 3)
    # the stages alone, device time
    geo = L.geometry(n, C)
    ws = L._workspace(geo["workspace_bytes"], dev)
    keys, perm, ws_sort, ws_rows, ws_lov = L.parts(ws, n, C, geo)
    box = torch.cat([min_C, max_C])
    Fd = Fx.detach()
    label, ce3, cc, info = L.rows_fwd(Fd, coords, target, box, 1, w, keys, ws_rows)
    L.sort_desc(keys, perm, ws_sort)
    loss_c, coef, lov1, present = L.lovasz_fwd(perm, label, keys, cc, ws_lov)
    gg = torch.ones(2, device=dev)
    res["stages_device"] = {
        "rows_fwd": event_timer(lambda: L.rows_fwd(Fd, coords, target, box, 1, w, keys, ws_rows), reps, windows),
        "sort_desc": event_timer(lambda: L.sort_desc(keys, perm, ws_sort), reps, windows),
        "lovasz_fwd": event_timer(lambda: L.lovasz_fwd(perm, label, keys, cc, ws_lov), reps, windows),
        "loss_bwd": event_timer(lambda: L.loss_bwd(Fd, label, coef, w, ce3, present, gg), reps, windows)}
    res["kernel_device"] = event_timer(kernel_step, reps, windows)
    res["torch_device"] = event_timer(torch_step, reps, windows)
    res["peak_bytes"] = {"kernel": peak(kernel_step), "torch": peak(torch_step)}
    res["loss_difference"] = {"ce": abs(float(k_ce) - float(t_ce)), "lovasz": abs(float(k_lov) - float(t_lov))}
    print("SEM_TIME " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=150)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", type=int, default=None)
    a = ap.parse_args()
    if a.child is not None:
        child(a.child, a.reps, a.windows)
        return 0
    results = []
    for n in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(n), "--reps", str(a.reps), "--windows", str(a.windows)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f"N = {n}: no result within {a.limit} s; stopping", flush=True)
            return 1
        lines = [l for l in r.stdout.splitlines() if l.startswith("SEM_TIME ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            print(f"N = {n}: the child ended with {r.returncode}; stopping", flush=True)
            return 1
        print(lines[-1], flush=True)
        results.append(json.loads(lines[-1][len("SEM_TIME "):]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/sem_time.py", "device": "MI355X", "reps": a.reps, "windows": a.windows, "results": results}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
