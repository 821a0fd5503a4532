"""Generate tests/golden/sem_*.npz: the REFERENCE's compute_sem_compl_loss and compute_sem_compl_loss_kitti360 on three small
seeded scenes.

Runs only in the build container (needs the reference checkout; never collected by pytest).  The reference's modules are imported
with `MinkowskiEngine := pasco_amd.me` (make_golden.py sets that up; its pruning runs on the CPU oracle).  Each scene: a
32 x 32 x 8 label grid at scale 1 (16 x 16 x 4 and 8 x 8 x 2 at scales 2 and 4) with some voxels labelled 255, C = 20 or 19
classes, 300 to 1500 rows per scale of which some lie outside the box; scene c has two subnets, the second without a row in its
box at scale 4 (the KITTI function skips that pair).  The reference runs in fp32 only: its `fg.float()` meets a double in
`torch.dot`.

Stored (data only, nothing of the reference's source): the inputs (logits as float16-exact values), the class frequencies, which
function ran, its two fp32 losses, and per (scale, subnet) the fp32 gradients of the CE term and of the Lovasz term with respect
to the logits, from two backward calls.

    python tests/golden/make_golden_sem.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402,F401  (sets up sys.path, the MinkowskiEngine alias and the inert stubs)

import pasco_amd.me as ME  # noqa: E402
from pasco.loss import losses as ref_losses  # noqa: E402

DIMS = (32, 32, 8)
SCALES = (1, 2, 4)
SCENES = {"a": dict(c=20, fn="compute_sem_compl_loss", subnets=1, n=(1500, 700, 300), seed=1),
          "b": dict(c=19, fn="compute_sem_compl_loss_kitti360", subnets=1, n=(1200, 600, 300), seed=2),
          "c": dict(c=20, fn="compute_sem_compl_loss", subnets=2, n=(900, 500, 300), seed=3)}


def make_scene(c, fn, subnets, n, seed):
    g = torch.Generator().manual_seed(5200 + seed)
    s = dict(c=c, fn=fn, subnets=subnets, freq={}, targets={}, logits={}, coords={}, min_Cs=[], max_Cs=[])
    for i in range(subnets):
        lo = torch.tensor([-7 + 40 * i, -5, -3])
        s["min_Cs"].append(lo)
        s["max_Cs"].append(lo + torch.tensor(DIMS) - 1)
    for k, scale in enumerate(SCALES):
        dims = tuple(d // scale for d in DIMS)
        s["freq"][scale] = (torch.rand(c, generator=g).double() * 1e6 + 1e3).numpy()
        for i in range(subnets):
            t = torch.randint(0, c, dims, generator=g).to(torch.uint8)
            t[torch.rand(dims, generator=g) < 0.08] = 255
            # unique voxels of the box widened by 3 on every side, so that some rows fall outside on every face
            wide = tuple(d + 6 for d in DIMS)
            pick = torch.randperm(wide[0] * wide[1] * wide[2], generator=g)[:n[k]].sort().values
            xyz = torch.stack([pick // (wide[1] * wide[2]), (pick // wide[2]) % wide[1], pick % wide[2]], dim=1) - 3 + s["min_Cs"][i]
            if i == 1 and scale == 4:
                xyz[:, 2] = s["max_Cs"][i][2] + 1 + xyz[:, 2] % 3      # no row inside the box
                xyz = torch.unique(xyz, dim=0)
            coords = torch.cat([torch.zeros(len(xyz), 1, dtype=torch.long), xyz], dim=1).to(torch.int32)
            s["targets"][(scale, i)] = t
            s["coords"][(scale, i)] = coords
            s["logits"][(scale, i)] = (torch.randn(len(xyz), c, generator=g) * 2).half().float()
    return s


def run_reference(s):
    fn = getattr(ref_losses, s["fn"])
    leaves = {k: v.clone().requires_grad_(True) for k, v in s["logits"].items()}
    sem_labels = {f"1_{sc}": [s["targets"][(sc, i)] for i in range(s["subnets"])] for sc in SCALES}
    sem_logits = {sc: [ME.SparseTensor(features=leaves[(sc, i)], coordinates=s["coords"][(sc, i)].clone()) for i in range(s["subnets"])]
                  for sc in SCALES}
    freq = {f"1_{sc}": s["freq"][sc] for sc in SCALES}
    ce, lov = fn(sem_labels, sem_logits, s["min_Cs"], s["max_Cs"], freq)
    grads = {}
    for name, loss in (("ce", ce), ("lovasz", lov)):
        for v in leaves.values():
            v.grad = None
        loss.backward(retain_graph=True)
        for k, v in leaves.items():
            grads[(name,) + k] = torch.zeros_like(v) if v.grad is None else v.grad.clone()
    return ce.detach(), lov.detach(), grads


def main():
    for name, cfg in SCENES.items():
        s = make_scene(**cfg)
        ce, lov, grads = run_reference(s)
        out = dict(c=np.int64(s["c"]), fn=np.array(s["fn"]), subnets=np.int64(s["subnets"]), scales=np.array(SCALES),
                   min_Cs=torch.stack(s["min_Cs"]), max_Cs=torch.stack(s["max_Cs"]), ce32=ce, lovasz32=lov)
        for sc in SCALES:
            out[f"freq_{sc}"] = s["freq"][sc]
            for i in range(s["subnets"]):
                out[f"target_{sc}_{i}"] = s["targets"][(sc, i)]
                out[f"coords_{sc}_{i}"] = s["coords"][(sc, i)]
                out[f"logits_{sc}_{i}"] = s["logits"][(sc, i)].half()
                out[f"dce32_{sc}_{i}"] = grads[("ce", sc, i)]
                out[f"dlovasz32_{sc}_{i}"] = grads[("lovasz", sc, i)]
        path = os.path.join(HERE, f"sem_{name}.npz")
        np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
        print(name, s["fn"], "ce", float(ce), "lovasz", float(lov), [len(v) for v in s["logits"].values()], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
