"""Backward of the masked cross-attention: `pa_attn_cross_bwd` (and its statistics pass alone) against torch autograd's backward of
the materialised formulation - `graph.transformer._attention_math` with a -inf bias, which keeps the [B, H, Q, N] score tensor -
on the same GPU, at the decoder's shape (B = 3 subnets, H = 8, Q = 100, Dh = 48) over the synthetic scene's level row counts.

    python tools/attn_grad_time.py [--reps 20] [--windows 5] [--out profiles/attn_grad_time.json]

Per level it prints one JSON line and collects them in `--out`: the times (median over `windows` device-event windows of `reps`
calls each, after warm-up calls of every shape; min and max alongside), the ratio torch / kernel, the achieved rate from the
algorithm's own count (5 products of 2 B H Q N Dh flops: S, dP, dV, dK, dQ) with its share of the fp32 matrix peak, and the peak
device memory of one backward of each kind over the level before it (torch.cuda.max_memory_allocated)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MATRIX = 157.3e12      # MI355X, v_mfma_f32_16x16x4_f32
B, H, Q, DH = 3, 8, 100, 48
LEVEL_ROWS = (210542, 44415, 8963, 1912)      # the synthetic scene's map levels (tools/grad_time.py rows_per_level)
ALLOWED = 0.3


def device_timer(fn, reps, windows, warm=3):
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
    """Peak device memory during fn() over the level before it; the result of fn is dropped before returning."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    r = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - before
    del r
    return int(peak)


def run_level(n, be, lib, timer, dev):
    from pasco_amd.graph.transformer import _attention_math
    g = torch.Generator(device=dev).manual_seed(n)
    q_raw = torch.randn(B, H, Q, DH, device=dev, generator=g)
    k = torch.randn(B, n, H * DH, device=dev, generator=g) * 1.7
    v = torch.randn(B, n, H * DH, device=dev, generator=g)
    dout = torch.randn(B, Q, H * DH, device=dev, generator=g)
    allow = torch.rand(B, n, Q, device=dev, generator=g) < ALLOWED
    bits, any_ = be.attn_mask_pack(allow.reshape(B * n, Q).float(), B, n)
    q4 = (q_raw * DH ** -0.5).contiguous()
    out = be.attn_cross_fwd(q4, k, v, bits, any_)
    rec = {"n": n, "B": B, "H": H, "Q": Q, "Dh": DH, "allowed": ALLOWED, "workspace_bytes": lib.workspace_bytes(n, B, H, Q)}
    rec["kernel"] = timer(lambda: lib.attn_cross_bwd(q4, k, v, bits, any_, out, dout))
    rec["kernel_stats_pass"] = timer(lambda: lib.attn_bwd_stats(q4, k, bits, any_, out, dout))
    rec["forward"] = timer(lambda: be.attn_cross_fwd(q4, k, v, bits, any_))
    rec["kernel_peak_bytes"] = peak_over(lambda: lib.attn_cross_bwd(q4, k, v, bits, any_, out, dout), dev)
    dq, dk, dv = lib.attn_cross_bwd(q4, k, v, bits, any_, out, dout)
    # torch: the materialised formulation, its graph kept so that only the backward is timed
    empty = ~allow.any(dim=1)                                                     # [B, Q]: attends everywhere
    bias = torch.zeros(B, 1, Q, n, device=dev).masked_fill_(~(allow.transpose(1, 2) | empty[:, :, None])[:, None], float("-inf"))
    del allow
    qt, kt, vt = (t.detach().clone().requires_grad_(True) for t in (q_raw, k, v))
    o = _attention_math(qt, kt.view(B, n, H, DH).transpose(1, 2), vt.view(B, n, H, DH).transpose(1, 2), bias)
    o = o.transpose(1, 2).reshape(B, Q, H * DH)
    rec["torch_saved_bytes"] = int(torch.cuda.memory_allocated(dev))
    rec["torch_backward"] = timer(lambda: torch.autograd.grad(o, (qt, kt, vt), dout, retain_graph=True))
    rec["torch_peak_bytes"] = peak_over(lambda: torch.autograd.grad(o, (qt, kt, vt), dout, retain_graph=True), dev)
    rec["score_tensor_bytes"] = 4 * B * H * Q * n
    tq, tk, tv = torch.autograd.grad(o, (qt, kt, vt), dout, retain_graph=True)
    tq = tq * DH ** 0.5                                                           # d / d(pre-scaled q)
    rec["max_diff_over_max"] = {name: float((a - b).abs().max() / b.abs().max())
                                for name, a, b in (("dq", dq, tq), ("dk", dk, tk), ("dv", dv, tv))}
    ms = rec["kernel"]["ms"]
    flops = 5 * 2.0 * B * H * Q * n * DH
    rec["ratio_torch_over_kernel"] = round(rec["torch_backward"]["ms"] / ms, 2)
    rec["tflops"] = round(flops / (ms * 1e-3) / 1e12, 2)
    rec["share_of_fp32_matrix_peak"] = round(flops / PEAK_FP32_MATRIX / (ms * 1e-3), 3)
    fwd_flops = 2 * 2.0 * B * H * Q * n * DH
    rec["forward_share_of_fp32_matrix_peak"] = round(fwd_flops / PEAK_FP32_MATRIX / (rec["forward"]["ms"] * 1e-3), 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "attn_grad_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attn_grad_time.py measures on the GPU; there is nothing to report without one"
    from pasco_amd.grad.attnlib import attn_grad_lib
    from pasco_amd.me.backend import hip_backend
    dev = torch.device("cuda", 0)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "levels": []}
    for n in LEVEL_ROWS:
        rec = run_level(n, hip_backend(), attn_grad_lib(), lambda fn: device_timer(fn, a.reps, a.windows), dev)
        print(json.dumps(rec), flush=True)
        out["levels"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
