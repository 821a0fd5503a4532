"""Training-mode batch normalisation + ReLU over rows, forward plus backward: `pasco_amd.grad.norm.batch_norm_rows(act="relu")`
(the pn_* kernels of include/pasco_norm.h) against torch's `F.batch_norm` + `F.relu` with torch's autograd, on the same GPU.

    python tools/norm_time.py [--reps 20] [--windows 7] [--out profiles/norm_time.json]

Sizes: N in {20 000, 300 000} rows, C in {32, 64, 256} channels (a coarse and a full-resolution level of the benchmark's scene).
Method of tools/grad_time.py: device events around `reps` forward + backward calls, the median over `windows` windows after
warm-up calls of the same shape (min and max alongside); the two routes alternate window by window, so a neighbour's load on the
machine falls on both.  The results are compared before anything is timed.

Bytes are the algorithm's own, as include/pasco_norm.h counts them: the forward reads x twice and writes y (3 N C 4), the
backward reads x and dy twice and writes dx (5 N C 4): 32 N C bytes per forward + backward; the share is of 8 TB/s and is the
whole call's (four row kernels, three per-channel ones and the host between them), not a kernel's.  The entry points are also
timed one by one (moments: one pass over [N, C] from HBM, the second read of a tile is the L2's; apply and bwd_sums: two passes;
bwd_dx: three), each share being that entry point's launches with their allocations."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_time import PEAK_HBM  # noqa: E402

SIZES = [(n, c) for n in (20_000, 300_000) for c in (32, 64, 256)]


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def stats(ts):
    return {"ms": round(float(np.median(ts)), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def run_size(n, c, dev, reps, windows):
    from pasco_amd.grad.norm import batch_norm_rows
    g = torch.Generator().manual_seed(n + c)
    x = (torch.randn(n, c, generator=g) * 1.3 + 0.37).to(dev).requires_grad_(True)
    dy = (torch.randn(n, c, generator=g) * 0.71).to(dev)
    w = (torch.randn(c, generator=g) * 0.37 + 1.13).to(dev).requires_grad_(True)
    b = (torch.randn(c, generator=g) * 0.29).to(dev).requires_grad_(True)
    rm, rv = torch.zeros(c, device=dev), torch.ones(c, device=dev)
    nbt = torch.zeros((), dtype=torch.long, device=dev)

    def ours():
        y = batch_norm_rows(x, w, b, rm, rv, nbt, 0.1, 1e-5, act="relu")
        return (y,) + torch.autograd.grad(y, (x, w, b), dy)

    def theirs():
        y = F.relu(F.batch_norm(x, rm, rv, w, b, True, 0.1, 1e-5))
        return (y,) + torch.autograd.grad(y, (x, w, b), dy)

    # Compared before anything is timed.  Without an activation every output has to agree with torch's to 1e-4 of the tensor's
    # largest magnitude.  ReLU's gradient is a step: an element whose pre-activation is within an fp32 rounding of 0 can take
    # the other side in the two routes, its dx then differs by a whole g and the channel's sums with it - so with ReLU y is held
    # to the same 1e-4 and the dx elements on the other side are COUNTED (a few in 10^7 are expected) and reported.
    def plain(fn_norm):
        y = fn_norm()
        return (y,) + torch.autograd.grad(y, (x, w, b), dy)

    a_none = plain(lambda: batch_norm_rows(x, w, b, rm.clone(), rv.clone(), None, 0.1, 1e-5))
    t_none = plain(lambda: F.batch_norm(x, rm.clone(), rv.clone(), w, b, True, 0.1, 1e-5))
    for a, t, name in zip(a_none, t_none, ("y", "dx", "dw", "db")):
        worst, scale = float((a - t).abs().max()), float(t.abs().max())
        assert worst <= 1e-4 * scale, f"{name} differs from torch's by {worst:.3e} of {scale:.3e} at n = {n}, c = {c}"
    rec = {"rows": n, "C": c}
    (ya, dxa, _, _), (yt, dxt, _, _) = ours(), theirs()
    assert float((ya - yt).abs().max()) <= 1e-4 * float(yt.abs().max()), f"y (ReLU) differs from torch's at n = {n}, c = {c}"
    count = int(((dxa - dxt).abs() > 1e-4 * float(dxt.abs().max())).sum())
    rec["dx_elements_on_the_other_side_of_relu"] = count
    assert count <= 1e-5 * dxa.numel(), f"dx (ReLU) differs from torch's in {count} elements at n = {n}, c = {c}"
    del a_none, t_none, ya, dxa, yt, dxt
    for _ in range(3):
        ours(), theirs()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(windows):
        t_ours.append(window(ours, reps))
        t_theirs.append(window(theirs, reps))
    rec.update({"batch_norm_rows": stats(t_ours), "torch": stats(t_theirs)})
    nbytes = 32.0 * n * c
    ms = rec["batch_norm_rows"]["ms"]
    rec["bytes"] = int(nbytes)
    rec["gbs"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    rec["share_of_8tbs"] = round(nbytes / PEAK_HBM / (ms * 1e-3), 4)
    rec["ratio_torch_over_kernels"] = round(rec["torch"]["ms"] / ms, 2)
    # the entry points one by one (each with its allocations, as the operator calls them): (name, call, passes over [n, c] fp32)
    from pasco_amd.grad.normlib import norm_lib
    lib, xd, wd, bd = norm_lib(), x.detach(), w.detach(), b.detach()
    total = lib.moments(xd)
    mr = lib.finish(total, 1e-5, 0.0, None, None)
    sums = lib.bwd_sums(dy, xd, mr, wd, bd, 1, 0.0)
    parts = [("moments", lambda: lib.moments(xd), 1), ("finish", lambda: lib.finish(total, 1e-5, 0.0, None, None), 0),
             ("apply", lambda: lib.apply(xd, mr, wd, bd, 1, 0.0), 2), ("bwd_sums", lambda: lib.bwd_sums(dy, xd, mr, wd, bd, 1, 0.0), 2),
             ("bwd_dx", lambda: lib.bwd_dx(dy, xd, mr, wd, bd, 1, 0.0, sums, total), 3)]
    rec["entry_points"] = {}
    for name, fn, passes in parts:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = stats([window(fn, reps) for _ in range(windows)])
        if passes:
            t["share_of_8tbs"] = round(passes * 4.0 * n * c / PEAK_HBM / (t["ms"] * 1e-3), 4)
        rec["entry_points"][name] = t
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "norm_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "norm_time.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "sizes": []}
    for n, c in SIZES:
        rec = run_size(n, c, dev, a.reps, a.windows)
        print(json.dumps(rec), flush=True)
        out["sizes"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
