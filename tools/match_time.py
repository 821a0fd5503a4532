"""One matcher + mask losses + backward on the `pm_*` kernels (pasco_amd/grad/criterion.py) against the same step written in torch
the way the training code it replaces writes it - transposed logits, the dense targets gathered to [N, T] floats, boolean
compactions, two pairs of einsum, the per-pair losses through autograd - on the same GPU, at Q = 100 queries, T = 30 targets,
N = 20 000 and N = 60 000 voxels of a 256 x 256 x 32 grid.  Both sides solve the assignment with pm_assign, so the difference
is the device work and its synchronisations.

    python tools/match_time.py [--reps 10] [--windows 5] [--out profiles/match_time.json]

Every size runs in a child process of its own under a time limit (`--limit` seconds); the parent never opens the GPU and stops at
the first child that fails.  A step contains a device-to-host copy on both sides, so the times are wall-clock times around a
synchronised step (median over `windows` windows of `reps` steps each, after warm-up; min and max alongside).  Per size one JSON
line: the step with and without packing the targets, the parts of the kernel side alone (device events), the ratio torch /
kernel, the peak device memory of one step of each kind over the level before it, and the largest difference between the two
sides' losses and gradients."""
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

Q, T, C = 100, 30, 20
DIMS = (256, 256, 32)
SIZES = (20000, 60000)


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


def peak_over(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    del r
    return int(peak)


def torch_step(logits, query_logits, masks, unknown, coords, labels, class_weights, assign):
    """The step in torch -> (loss_mask [K], loss_dice [K], dlogits)."""
    x_all = logits.detach().requires_grad_(True)
    c = coords.long()
    tgt_rows = masks[:, c[:, 1], c[:, 2], c[:, 3]].t().float()                    # [N, T]
    unk = unknown[c[:, 1], c[:, 2], c[:, 3]]
    with torch.no_grad():
        valid = (tgt_rows.sum(1) > 0) & ~unk
        x = x_all.t()[:, valid]
        y = tgt_rows.t()[:, valid]
        p = x.sigmoid()
        dice = 1 - (2 * torch.einsum("nc,mc->nm", p, y) + 1) / (p.sum(-1)[:, None] + y.sum(-1)[None, :] + 1)
        pos = 0.25 * (1 - p) ** 2 * F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
        neg = 0.75 * p ** 2 * F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
        focal = (torch.einsum("nc,mc->nm", pos, y) + torch.einsum("nc,mc->nm", neg, 1 - y)) / x.shape[1]
        cost = (focal - query_logits.softmax(-1)[:, labels] + dice) * class_weights[labels][None, :]
        src, tgt = assign(cost.cpu())
    w = class_weights[labels[tgt.to(labels.device)]]
    known = ~unk
    xs = x_all[:, src.to(x_all.device)][known]
    ys = tgt_rows[:, tgt.to(x_all.device)][known]
    p = xs.sigmoid()
    ce = F.binary_cross_entropy_with_logits(xs, ys, reduction="none")
    p_t = p * ys + (1 - p) * (1 - ys)
    loss_mask = ((0.25 * ys + 0.75 * (1 - ys)) * ce * (1 - p_t) ** 2 * w[None, :]).mean(0)
    loss_dice = (1 - (2 * (p * ys).sum(0) + 1) / (p.sum(0) + ys.sum(0) + 1)) * w
    (loss_mask.mean() + loss_dice.mean()).backward()
    return loss_mask.detach(), loss_dice.detach(), x_all.grad


def run_size(n, reps, windows):
    from pasco_amd.grad import criterion as crit
    from pasco_amd.grad.matchlib import BIT_KNOWN, geometry, match_lib
    dev = torch.device("cuda", 0)
    lib = match_lib()
    g = torch.Generator(device=dev).manual_seed(n)
    owner = torch.randint(0, T + 3, DIMS, device=dev, generator=g)
    masks = (owner[None] == torch.arange(T, device=dev)[:, None, None, None]).to(torch.uint8)
    unknown = torch.rand(DIMS, device=dev, generator=g) < 0.1
    pick = torch.randperm(DIMS[0] * DIMS[1] * DIMS[2], device=dev, generator=g)[:n]
    coords = torch.stack([torch.zeros_like(pick), pick // (DIMS[1] * DIMS[2]), (pick // DIMS[2]) % DIMS[1], pick % DIMS[2]],
                         dim=1).to(torch.int32)
    logits = torch.randn(n, Q, device=dev, generator=g) * 2
    query_logits = torch.randn(Q, C + 1, device=dev, generator=g)
    labels = torch.randint(0, C, (T,), device=dev, generator=g)
    class_weights = torch.rand(C + 1, device=dev, generator=g) + 0.5
    matcher = crit.HungarianMatcher()
    unknown_u8 = unknown.to(torch.uint8)

    def kernel_step(packed=None):
        x = logits.detach().requires_grad_(True)
        pk = crit.pack_targets(masks, unknown_u8, coords) if packed is None else packed
        src, tgt = matcher.match_packed(x, query_logits, labels, class_weights, pk)
        lm, ld = crit.mask_losses(x, pk, src, tgt, class_weights[labels[tgt.to(dev)]])
        (lm.mean() + ld.mean()).backward()
        return lm.detach(), ld.detach(), x.grad

    def t_step():
        return torch_step(logits, query_logits, masks, unknown, coords, labels, class_weights, lib.assign)

    packed = crit.pack_targets(masks, unknown_u8, coords)
    tq = torch.zeros(Q, dtype=torch.int32, device=dev)
    coef = torch.ones(Q, 3, device=dev)
    rec = {"n": n, "Q": Q, "T": T, "geometry": geometry(n, Q, T)}
    rec["kernel_step"] = wall_timer(kernel_step, reps, windows)
    rec["kernel_step_targets_packed"] = wall_timer(lambda: kernel_step(packed), reps, windows)
    rec["torch_step"] = wall_timer(t_step, reps, windows)
    rec["pm_target_pack"] = event_timer(lambda: crit.pack_targets(masks, unknown_u8, coords), reps, windows)
    rec["pm_pair_sums"] = event_timer(lambda: lib.pair_sums(logits, packed.tbits, packed.flags, BIT_KNOWN, T), reps, windows)
    rec["pm_mask_loss_bwd"] = event_timer(lambda: lib.mask_loss_bwd(logits, packed.tbits, packed.flags, tq, coef, T), reps, windows)
    cost = torch.randn(Q, T, dtype=torch.float64)
    t0 = time.perf_counter()
    for _ in range(100):
        lib.assign(cost)
    rec["pm_assign_ms"] = round((time.perf_counter() - t0) * 10, 4)
    rec["kernel_peak_bytes"] = peak_over(kernel_step, dev)
    rec["torch_peak_bytes"] = peak_over(t_step, dev)
    rec["logits_bytes"] = 4 * n * Q
    a, b = kernel_step(), t_step()
    rec["max_diff_over_max"] = {name: float((u - v).abs().max() / v.abs().max())
                                for name, u, v in zip(("loss_mask", "loss_dice", "dlogits"), a, b)}
    rec["ratio_torch_over_kernel"] = round(rec["torch_step"]["ms"] / rec["kernel_step"]["ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds a size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_time.json"))
    ap.add_argument("--one", type=int, default=None, help="(internal) run this size in this process and print its JSON line")
    a = ap.parse_args()
    if a.one is not None:
        assert torch.cuda.is_available(), "match_time.py measures on the GPU; there is nothing to report without one"
        print(json.dumps(run_size(a.one, a.reps, a.windows)), flush=True)
        return 0
    out = {"reps": a.reps, "windows": a.windows, "sizes": []}
    for n in SIZES:
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--one", str(n), "--reps", str(a.reps),
               "--windows", str(a.windows)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            print(f"match_time.py: N = {n} ended with status {r.returncode}; nothing more is started", file=sys.stderr)
            return r.returncode
        line = r.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        out["sizes"].append(json.loads(line))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
