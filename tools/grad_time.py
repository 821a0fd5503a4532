"""Backward of the sparse convolutions: the pg_* weight gradient and the input-gradient launch against what a caller would write
without them - the per-offset loop over `kernel_map_coo` with `index_select` and `matmul` in torch - on the same GPU, at the layer
shapes of the U-Net on the synthetic scene's map levels (pasco_amd/graph/synth.py).

    python tools/grad_time.py [--reps 20] [--windows 5] [--out profiles/grad_time.json]

Per layer it prints one JSON line and collects them in `--out`: pairs P, the times (median over `windows` device-event windows of
`reps` calls each, after warm-up calls of every shape; min and max alongside), the ratio torch / kernel, the achieved rate from
the algorithm's own counts (weight gradient: 2 P cin cout flops, 4 P (cin + cout) gathered bytes) and the share of the bound,
bound = max(flops / fp32 matrix peak, bytes / HBM peak), with which of the two it is.  The inverse table is built once per map
(cached by the manager); its build time is reported on its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP32_MATRIX = 157.3e12      # MI355X, v_mfma_f32_32x32x2_f32
PEAK_HBM = 8.0e12

# (name, level of the input map, kind, cin, cout): level l = tensor stride 2^l
LAYERS = [
    ("3^3 32->32 @1", 0, "same", 32, 32),
    ("3^3 64->64 @2", 1, "same", 64, 64),
    ("3^3 128->128 @4", 2, "same", 128, 128),
    ("3^3 256->256 @8", 3, "same", 256, 256),
    ("k2s2 down 32->64 @1", 0, "down", 32, 64),
    ("k2s2 down 64->128 @2", 1, "down", 64, 128),
    ("k2s2 down 128->256 @4", 2, "down", 128, 256),
    ("k2s2 up 256->128 @8", 3, "gen", 256, 128),
    ("k2s2 up 128->64 @4", 2, "gen", 128, 64),
    ("k2s2 up 64->32 @2", 1, "gen", 64, 32),
]


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


def level_keys(mgr, key, levels):
    keys = [key]
    for _ in range(levels):
        keys.append(mgr.stride(keys[-1], 2))
    return keys


def layer_maps(mgr, keys, level, kind):
    """-> (in_key, out_key, kernel_size, transposed) of one layer."""
    if kind == "same":
        return keys[level], keys[level], 3, False
    if kind == "down":
        return keys[level], keys[level + 1], 2, False
    return keys[level], mgr.expand(keys[level], 2), 2, True


def torch_wgrad(x, dy, coo, out):
    for k, (pin, pout) in enumerate(coo):
        out[k] = x.index_select(0, pin).t() @ dy.index_select(0, pout)
    return out


def torch_dgrad(dy, w, coo, out):
    out.zero_()
    for k, (pin, pout) in enumerate(coo):
        out.index_add_(0, pin, dy.index_select(0, pout) @ w[k].t())
    return out


def share(flops, nbytes, ms):
    t_f, t_b = flops / PEAK_FP32_MATRIX, nbytes / PEAK_HBM
    return {"tflops": round(flops / (ms * 1e-3) / 1e12, 2), "gathered_gbs": round(nbytes / (ms * 1e-3) / 1e9, 1),
            "share_of_bound": round(max(t_f, t_b) / (ms * 1e-3), 3), "bound": "fp32 matrix" if t_f >= t_b else "HBM"}


def run_layer(mgr, keys, layer, be, G, timer):
    name, level, kind, cin, cout = layer
    in_key, out_key, ks, transposed = layer_maps(mgr, keys, level, kind)
    nbr = mgr.kernel_map(in_key, out_key, ks, transposed=transposed)
    n_in, n_out, K = mgr.size(in_key), mgr.size(out_key), nbr.shape[0]
    dev = nbr.device
    g = torch.Generator().manual_seed(level * 7 + cin)
    x = torch.randn(n_in, cin, generator=g).to(dev)
    dy = torch.randn(n_out, cout, generator=g).to(dev)
    w = (torch.randn(K, cin, cout, generator=g) / (K * cin) ** 0.5).to(dev)
    coo = [(a.long(), b.long()) for a, b in mgr.kernel_map_coo(in_key, out_key, ks, transposed=transposed)]
    P = int(sum(a.numel() for a, _ in coo))
    rec = {"layer": name, "K": K, "cin": cin, "cout": cout, "n_in": n_in, "n_out": n_out, "pairs": P}
    # weight gradient
    dw_t = torch.empty(K, cin, cout, device=dev)
    dw = torch.empty_like(dw_t)
    rec["wgrad"] = timer(lambda: G.conv_wgrad(x, dy, nbr))
    rec["wgrad_torch_loop"] = timer(lambda: torch_wgrad(x, dy, coo, dw_t))
    dw = G.conv_wgrad(x, dy, nbr)
    rec["wgrad_max_diff_over_max"] = float((dw - dw_t).abs().max() / dw_t.abs().max())
    rec["wgrad_ratio_torch_over_kernel"] = round(rec["wgrad_torch_loop"]["ms"] / rec["wgrad"]["ms"], 2)
    rec["wgrad_rate"] = share(2.0 * P * cin * cout, 4.0 * P * (cin + cout), rec["wgrad"]["ms"])
    # input gradient: the forward kernels over the inverse table (built once per map)
    rec["inverse_table_build"] = timer(lambda: G.nbr_invert(nbr, n_in))
    inv = mgr.kernel_map_inverse(nbr, n_in)
    w_t = w.transpose(1, 2).contiguous()
    dx_t = torch.empty(n_in, cin, device=dev)
    rec["dgrad"] = timer(lambda: be.conv_fwd(dy, w_t, inv, n_in))
    rec["dgrad_torch_loop"] = timer(lambda: torch_dgrad(dy, w, coo, dx_t))
    dx = be.conv_fwd(dy, w_t, inv, n_in)
    rec["dgrad_max_diff_over_max"] = float((dx - dx_t).abs().max() / dx_t.abs().max())
    rec["dgrad_ratio_torch_over_kernel"] = round(rec["dgrad_torch_loop"]["ms"] / rec["dgrad"]["ms"], 2)
    rec["dgrad_rate"] = share(2.0 * P * cin * cout, 4.0 * (P * cout + n_in * cin), rec["dgrad"]["ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "grad_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "grad_time.py measures on the GPU; there is nothing to report without one"
    import pasco_amd.grad as G
    from pasco_amd.graph.synth import make_occupancy
    from pasco_amd.me.backend import hip_backend
    from pasco_amd.me.core import CoordinateManager
    dev = torch.device("cuda", 0)
    c = np.argwhere(make_occupancy(0)).astype(np.int32)
    coords = torch.from_numpy(np.concatenate([np.zeros((len(c), 1), np.int32), c], 1)).to(dev)
    mgr = CoordinateManager(D=3, device=dev)
    key, _ = mgr.insert_and_map(coords, 1)
    keys = level_keys(mgr, key, 4)
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows,
           "rows_per_level": [mgr.size(k) for k in keys], "layers": []}
    for layer in LAYERS:
        rec = run_layer(mgr, keys, layer, hip_backend(), G, lambda fn: device_timer(fn, a.reps, a.windows))
        print(json.dumps(rec), flush=True)
        out["layers"].append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
