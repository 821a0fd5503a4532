"""One optimiser step over the parameters of a constructed `PascoNet` with random gradients: `pasco_amd.grad.optim.AdamW(max_norm=0.5)`
(the po_* kernels of include/pasco_optim.h: three launches) against torch on the same GPU, both of its multi-tensor paths:
`clip_grad_norm_(foreach=True)` + `AdamW(foreach=True)` and `clip_grad_norm_(foreach=True)` + `AdamW(fused=True)`.

    python tools/optim_time.py [--reps 20] [--windows 7] [--out profiles/optim_time.json]

The net is the benchmark's (bench.py `build_net`: MIMO-3, 283 input channels, f = 64, 100 queries, light decoder); only its
parameter shapes matter.  Method of tools/norm_time.py: device events around `reps` steps, the median over `windows` windows
after warm-up steps (min and max alongside); the three routes alternate window by window, so a neighbour's load on the machine
falls on all of them.  One step of each route from the same weights is compared before anything is timed.

Bytes are the algorithm's own, 32 per element: the norm reads g (4), the update reads p, g, m, v and writes p, m, v (28).  The
share is of 8 TB/s and is the whole step's - three launches and the Python in front of them - not a kernel's; the three entry
points are also timed one by one.  Launches per step are counted by torch's profiler in a step of its own, outside the timed
windows.  The clocks are read (not set) before and after, as `rocm-smi --showclocks` prints them."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_time import PEAK_HBM  # noqa: E402
from tools.norm_time import stats, window  # noqa: E402


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "-d", "0"], capture_output=True, text=True, timeout=60).stdout
        return [line.strip() for line in out.splitlines() if "clk" in line and "GPU[0]" in line]
    except Exception as e:      # noqa: BLE001 - the clocks are a note next to the numbers, not a measurement
        return [f"not read: {e}"]


def launches_of(fn):
    """Kernel launches of one call of `fn`, from torch's profiler; None where the profiler gives no device events."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        # device events that are kernels: no copies, no fills, and not the `Optimizer.step#...` range torch's optimiser base class
        # records around every step (the profiler mirrors it on the device timeline)
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name
                 and "emset" not in e.name and not e.name.startswith("Optimizer.step")]
        return {"count": len(names), "distinct": sorted(set(n[:60] for n in names))[:12]} if names else None
    except Exception:      # noqa: BLE001
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--f", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "optim_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "optim_time.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    from pasco_amd.grad.optim import AdamW
    from pasco_amd.grad.optimlib import PO_CHUNK, optim_lib
    from pasco_amd.graph import PascoNet

    torch.manual_seed(1234)
    net = PascoNet(n_classes=20, n_infers=3, in_channels=283, f=a.f, num_queries=100, heavy_decoder=False)
    shapes = [tuple(p.shape) for p in net.parameters()]
    values = [p.detach().clone() for p in net.parameters()]
    del net
    sizes = np.array([int(np.prod(s)) for s in shapes])
    g = torch.Generator().manual_seed(7)
    grads = [torch.randn(s, generator=g) * 0.01 for s in shapes]

    def params():
        ps = [torch.nn.Parameter(v.to(dev).clone()) for v in values]
        for p, gr in zip(ps, grads):
            p.grad = gr.to(dev).clone()
        return ps

    kw = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    p_ours, p_each, p_fused = params(), params(), params()
    ours = AdamW(p_ours, max_norm=0.5, **kw)
    each = torch.optim.AdamW(p_each, foreach=True, **kw)
    fused = torch.optim.AdamW(p_fused, fused=True, **kw)

    def step_ours():
        ours.step()

    def step_each():
        torch.nn.utils.clip_grad_norm_(p_each, 0.5, foreach=True)
        each.step()

    def step_fused():
        torch.nn.utils.clip_grad_norm_(p_fused, 0.5, foreach=True)
        fused.step()

    routes = {"kernels": step_ours, "torch_foreach": step_each, "torch_fused": step_fused}
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "tensors": len(shapes),
           "elements": int(sizes.sum()), "tensors_under_4096": int((sizes < 4096).sum()), "largest_tensor": int(sizes.max()),
           "chunks": int(((sizes + PO_CHUNK - 1) // PO_CHUNK).sum()), "clocks_before": clocks()}

    # one step of each route from the same weights, compared before anything is timed
    for fn in routes.values():
        fn()
    torch.cuda.synchronize()
    norm = float(ours.grad_norm)
    out["grad_norm"] = norm
    for name, ps in (("torch_foreach", p_each), ("torch_fused", p_fused)):
        worst = max(float((x.detach() - y.detach()).abs().max()) for x, y in zip(p_ours, ps))
        out[f"max_abs_difference_from_{name}"] = worst
        assert worst <= 1e-6, f"one step differs from {name} by {worst:.3e}"      # a step moves a weight by lr = 1e-4 at most
    out["launches"] = {name: launches_of(fn) for name, fn in routes.items()}

    for _ in range(3):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in routes}
    for _ in range(a.windows):
        for name, fn in routes.items():
            times[name].append(window(fn, a.reps))
    nbytes = 32.0 * float(sizes.sum())
    for name in routes:
        out[name] = stats(times[name])
    ms = out["kernels"]["ms"]
    out["bytes"] = int(nbytes)
    out["gbs"] = round(nbytes / (ms * 1e-3) / 1e9, 1)
    out["share_of_8tbs"] = round(nbytes / PEAK_HBM / (ms * 1e-3), 4)
    for name in ("torch_foreach", "torch_fused"):
        out[f"ratio_{name}_over_kernels"] = round(out[name]["ms"] / ms, 2)

    # the entry points one by one, on the optimiser's own tables: (name, call, bytes per element)
    lib, buf = optim_lib(), ours._buffers()
    T, C = len(buf.key), buf.n_chunks
    hyper = [(kw["lr"], 0.9, 0.999, kw["eps"], kw["weight_decay"])]
    parts = [("sqnorm", lambda: lib.sqnorm(buf.tensors, T, buf.chunks, C, buf.partials), 4),
             ("prepare", lambda: lib.prepare(buf.tensors, T, buf.partials, C, hyper, 0.5, 1.0, 0, buf.states, buf.scalars, buf.result,
                                             buf.step), 0),
             ("adamw", lambda: lib.adamw(buf.tensors, T, buf.chunks, C, buf.scalars, buf.step), 28)]
    out["entry_points"] = {}
    for name, fn, per_element in parts:
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t = stats([window(fn, a.reps) for _ in range(a.windows)])
        if per_element:
            t["share_of_8tbs"] = round(per_element * float(sizes.sum()) / PEAK_HBM / (t["ms"] * 1e-3), 4)
        out["entry_points"][name] = t
    out["clocks_after"] = clocks()
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
