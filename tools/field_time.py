"""The point <-> voxel kernels of include/pasco_field.h, forward and backward, against their torch restatement (`index_add_`,
`scatter_reduce`, indexed gathers on the same GPU tensors) at a point-cloud network's shape.

    python tools/field_time.py [--points 120000] [--reps 200] [--windows 5] [--out profiles/field_time.json]

Workload: `points` points in 2 batch elements, uniform in a cube whose side is chosen so that about 1.5 points share a voxel at
tensor stride 1 (see `cloud`), C = 4, 96 and 256 channels; the interpolation reads the voxel
tensor at the same points.  Method of tools/grad_time.py: the median over `windows` device-event windows of `reps` calls each,
after warm-up calls (min and max alongside); 200 calls make a window of 2 - 100 ms.  Bytes are the formula's own: every operand
row read once, every result row written once, every table entry read once; `effective_gbs` is those bytes over the CALL's time
(the grouping is ten launches, its rate is not a kernel's).  It is NOT an HBM rate: the operands of one shape (4 - 200 MB) are
reread by every call of a window and largely stay in the 256 MB last-level cache.  There is no pass mark: a shape at which the device route is slower than the
restatement is reported as such ("slower")."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.grad_time import device_timer  # noqa: E402

CHANNELS = (4, 96, 256)


def rate(nbytes, ms):
    return {"bytes": int(nbytes), "effective_gbs": round(nbytes / (ms * 1e-3) / 1e9, 1)}


def cloud(points: int, seed: int = 0):
    """-> coordinates fp32 [points, 4].  Uniform points in 2 batch elements of a cube of side s: a voxel holds Poisson(lam) points
    with lam = points / (2 s^3), and an OCCUPIED voxel holds lam / (1 - exp(-lam)) of them on average; lam = 0.874 makes that 1.5."""
    lam = 0.874
    side = (points / 2 / lam) ** (1.0 / 3.0)
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(points, 3, generator=g) * side
    b = (torch.arange(points) % 2).float()[:, None]
    return torch.cat([b, xyz], dim=1)


def torch_group(keys, n_seg):
    perm = torch.sort(keys, stable=True).indices.to(torch.int32)
    offsets = torch.zeros(n_seg + 1, dtype=torch.int32, device=keys.device)
    offsets[1:] = torch.cumsum(torch.bincount(keys, minlength=n_seg), 0)
    return offsets, perm


def run_channels(c, field, st, L, H, be, timer, points):
    mgr = field.coordinate_manager
    fkey, key = field.coordinate_field_map_key, st.coordinate_map_key
    dev = field.F.device
    n, nv = len(field), len(st)
    inv = mgr.field_map(fkey, key)
    invl = inv.long()
    offsets, perm = mgr.field_grouping(fkey, key, L)
    g = torch.Generator().manual_seed(c)
    x, dyv = torch.randn(n, c, generator=g).to(dev), torch.randn(nv, c, generator=g).to(dev)
    xv, dyp = torch.randn(nv, c, generator=g).to(dev), torch.randn(n, c, generator=g).to(dev)
    rec = {"C": c, "points": n, "voxels": nv, "ops": {}}
    prow, vrow, idx = 4.0 * n * c, 4.0 * nv * c, 4.0 * n

    def op(name, kernel, restated, nbytes):
        k, t = timer(kernel), timer(restated)
        rec["ops"][name] = {"kernel": k, "torch": t, "torch_over_kernel": round(t["ms"] / k["ms"], 2), **rate(nbytes, k["ms"]),
                            "slower": k["ms"] > t["ms"]}

    _, cnt, arg = L.seg_rows(x, offsets, perm, H.FIELD_MAX)
    if c == CHANNELS[0]:                 # the tables do not depend on the channels
        op("group", lambda: L.group(inv, nv), lambda: torch_group(invl, nv), 2 * idx + 4.0 * (nv + 1))
    op("sparse_avg", lambda: L.seg_rows(x, offsets, perm, H.FIELD_AVG),
       lambda: torch.zeros((nv, c), device=dev).index_add_(0, invl, x) / torch.bincount(invl, minlength=nv).clamp(min=1)[:, None],
       prow + vrow + idx + 4.0 * (nv + 1))
    op("sparse_avg_bwd", lambda: L.gather_w(dyv, inv, cnt), lambda: dyv[invl] * (1.0 / cnt[invl])[:, None], prow + vrow + 2 * idx)
    op("sparse_sum", lambda: L.seg_rows(x, offsets, perm, H.FIELD_SUM), lambda: torch.zeros((nv, c), device=dev).index_add_(0, invl, x),
       prow + vrow + idx + 4.0 * (nv + 1))
    ie = invl[:, None].expand(n, c)
    op("sparse_max", lambda: L.seg_rows(x, offsets, perm, H.FIELD_MAX),
       lambda: torch.zeros((nv, c), device=dev).scatter_reduce_(0, ie, x, "amax", include_self=False), prow + 2 * vrow + idx + 4.0 * (nv + 1))
    op("sparse_max_bwd", lambda: L.seg_max_bwd(dyv, arg, n), lambda: H.field_seg_max_bwd(dyv, arg, n), prow + 2 * vrow)
    op("slice", lambda: be.gather_rows(xv, inv), lambda: xv[invl], prow + vrow + idx)
    op("slice_bwd", lambda: L.seg_rows(dyp, offsets, perm, H.FIELD_SUM), lambda: torch.zeros((nv, c), device=dev).index_add_(0, invl, dyp),
       prow + vrow + idx + 4.0 * (nv + 1))
    cmap = mgr._maps[key]
    rows, weights = L.interp_map(points, cmap.tkeys, cmap.tvals, 1)
    if c == CHANNELS[0]:
        op("interp_map", lambda: L.interp_map(points, cmap.tkeys, cmap.tvals, 1), lambda: H.field_interp_map(points, cmap.tkeys, cmap.tvals, 1),
           16.0 * n + 2 * 32.0 * n)
        rec["corners_present"] = round(float((rows >= 0).float().mean()), 4)
    rl = rows.long().clamp(min=0)
    have = (rows >= 0)

    def torch_interp():
        out = torch.zeros((n, c), device=dev)
        for k in range(8):
            out = out + torch.where(have[k][:, None], weights[k][:, None] * xv[rl[k]], torch.zeros((), device=dev))
        return out

    op("interp_fwd", lambda: L.interp_fwd(xv, rows, weights), torch_interp, 8 * prow * float(have.float().mean()) + prow + 64.0 * n)
    flat, wflat = rows.reshape(-1), weights.reshape(-1)

    def kernel_interp_bwd():
        o, p = L.group(flat, nv)
        return L.seg_rows(dyp, o, p, H.FIELD_SUM, w=wflat, src_mod=n)

    fl, ok = flat.long().clamp(min=0), flat >= 0

    def torch_interp_bwd():
        terms = torch.where(ok[:, None], wflat[:, None] * dyp.repeat(8, 1), torch.zeros((), device=dev))
        return torch.zeros((nv, c), device=dev).index_add_(0, fl, terms)

    op("interp_bwd", kernel_interp_bwd, torch_interp_bwd, 8 * prow * float(have.float().mean()) + vrow + 3 * 32.0 * n)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "field_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "field_time.py measures on the GPU; there is nothing to report without one"
    import pasco_amd.me as ME
    from pasco_amd.grad import host as H
    from pasco_amd.grad.fieldlib import field_lib
    from pasco_amd.me.backend import hip_backend
    dev = torch.device("cuda", 0)
    points = cloud(a.points).to(dev)
    field = ME.TensorField(torch.zeros(a.points, 1, device=dev), points)
    st = field.sparse()
    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "windows": a.windows, "points": a.points, "voxels": len(st),
           "points_per_voxel": round(a.points / len(st), 3), "channels": []}
    for c in CHANNELS:
        rec = run_channels(c, field, st, field_lib(), H, hip_backend(), lambda fn: device_timer(fn, a.reps, a.windows), points)
        print(json.dumps(rec), flush=True)
        out["channels"].append(rec)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
