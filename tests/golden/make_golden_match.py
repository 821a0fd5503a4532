"""Generate tests/golden/match_*.npz: the REFERENCE's HungarianMatcher and SetCriterion on three small seeded scenes.

Runs only in the build container (needs the reference checkout; never collected by pytest).  The reference's modules are imported
with `MinkowskiEngine := pasco_amd.me` (make_golden.py sets that up).  Each scene: Q = 100 queries over N voxels of a
32 x 32 x 8 grid with some unknown voxels, T = 7 / 12 / 30 targets, 20 classes; the last scene has two `aux_outputs` levels on
the same coordinates.  The criterion runs twice, in fp64 and in fp32; the script REFUSES a scene whose matches differ between the
two (a near-tie would make the fixture a coin toss).  The criterion's `compute_ssc_sparse_loss` is replaced by zeros: those
terms are not part of what `Net.step` optimises and are not recorded.

Stored (data only, nothing of the reference's source): the inputs (logits as float16-exact values), per level the matches, the
fp64 and fp32 losses, the fp64 and fp32 gradients with respect to the query logits and - in the matched columns only, every
other column was checked to be exactly zero - with respect to the voxel logits.

    python tests/golden/make_golden_match.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as G  # noqa: E402  (sets up sys.path, the MinkowskiEngine alias and the inert stubs)

import pasco_amd.me as ME  # noqa: E402
from pasco.loss.criterion_sparse import SetCriterion  # noqa: E402
from pasco.loss.matcher_sparse import HungarianMatcher  # noqa: E402

DIMS = (32, 32, 8)
Q, C = 100, 20
SCENES = {"a": dict(t=7, n=1500, aux=0, seed=1), "b": dict(t=12, n=1000, aux=0, seed=2), "c": dict(t=30, n=500, aux=2, seed=3)}
WEIGHTS = {"loss_ce": 2.0, "loss_mask": 40.0, "loss_dice": 1.5, "ssc_ce": 1.0, "ssc_lovasz": 1.0}


def make_scene(t, n, aux, seed):
    g = torch.Generator().manual_seed(4200 + seed)
    dx, dy, dz = DIMS
    vol = dx * dy * dz
    # targets: a seeded partition of the grid into t + 1 slabs of random voxels, slab t = in no target; then a few overlaps
    owner = torch.randint(0, t + 1, (vol,), generator=g)
    masks = torch.stack([(owner == k) for k in range(t)]).reshape(t, dx, dy, dz)
    masks[0] |= (torch.rand(dx, dy, dz, generator=g) < 0.02)
    unknown = torch.rand(dx, dy, dz, generator=g) < 0.15
    pick = torch.randperm(vol, generator=g)[:n].sort().values
    xyz = torch.stack([pick // (dy * dz), (pick // dz) % dy, pick % dz], dim=1).to(torch.int32)
    min_c = torch.tensor([8, -16, 4], dtype=torch.int32)
    coords = torch.cat([torch.zeros(n, 1, dtype=torch.int32), xyz + min_c], dim=1)
    # logits that know something about the targets, so that the matching is not a coin toss: query k < t leans to target k
    tgt_rows = masks.reshape(t, -1)[:, pick].t().float()                                 # [n, t]
    levels = []
    for _ in range(aux + 1):
        x = torch.randn(n, Q, generator=g) * 1.5 - 1.0
        x[:, :t] += 3.0 * tgt_rows[:, torch.randperm(t, generator=g)]
        levels.append((x.half().float(), torch.randn(1, Q, C + 1, generator=g)))
    labels = torch.randint(0, C, (t,), generator=g)
    class_weights = torch.rand(C + 1, generator=g) + 0.5
    return dict(masks=masks, unknown=unknown, coords=coords, min_c=min_c, levels=levels, labels=labels, class_weights=class_weights)


def run_reference(s, dtype):
    crit = SetCriterion(C, HungarianMatcher(1, 1, 1), WEIGHTS, 0.1, [s["class_weights"].to(dtype)], torch.ones(C))
    crit.compute_ssc_sparse_loss = lambda *a, **k: (0, 0)
    seen = []
    inner = crit.matcher.memory_efficient_forward

    def spy(*a, **k):
        r = inner(*a, **k)
        seen.append(r)
        return r
    crit.matcher.forward = spy
    leaves, outs = [], []
    for x, ql in s["levels"]:
        f = x.to(dtype).clone().requires_grad_(True)
        qlog = ql.to(dtype).clone().requires_grad_(True)
        leaves.append((f, qlog))
        outs.append({"voxel_logits": ME.SparseTensor(features=f, coordinates=s["coords"].clone()), "query_logits": qlog})
    outputs = dict(outs[0])
    if len(outs) > 1:
        outputs["aux_outputs"] = outs[1:]
    targets = [{"labels": s["labels"], "masks": s["masks"].to(dtype)}]
    losses = crit(None, outputs, targets, None, s["unknown"][None], 0, [], s["min_c"])
    assert set(crit.state_dict()) == {"empty_weight", "compl_labelweights"}
    per_level = []
    for lv in range(len(outs)):
        suffix = "" if lv == 0 else "_level{}".format(lv - 1)
        d = losses if lv == 0 else losses["loss_aux"]
        vals = [d["loss_ce" + suffix], d["loss_mask" + suffix], d["loss_dice" + suffix]]
        per_level.append(vals)
    total = sum(sum(v) for v in per_level)
    total.backward()
    return seen, per_level, leaves, sorted(losses.keys()), sorted(losses["loss_aux"].keys())


def main():
    for name, cfg in SCENES.items():
        s = make_scene(**cfg)
        seen64, l64, leaves64, keys, aux_keys = run_reference(s, torch.float64)
        seen32, l32, leaves32, _, _ = run_reference(s, torch.float32)
        out = dict(masks=s["masks"].to(torch.uint8), unknown=s["unknown"].to(torch.uint8), coords=s["coords"], min_c=s["min_c"],
                   labels=s["labels"], class_weights=s["class_weights"], n_levels=np.int64(len(s["levels"])),
                   keys=np.array(keys), aux_keys=np.array(aux_keys),
                   weight_names=np.array(list(WEIGHTS)), weight_values=np.array(list(WEIGHTS.values())))
        for lv, ((x, ql), (f, qlog), (f32, qlog32)) in enumerate(zip(s["levels"], leaves64, leaves32)):
            (s64, t64), (s32, t32) = seen64[lv], seen32[lv]
            assert torch.equal(s64, s32) and torch.equal(t64, t32), f"scene {name} level {lv}: fp32 and fp64 match differently"
            other = torch.ones(Q, dtype=torch.bool)
            other[s64] = False
            assert not bool(f.grad[:, other].any()), "an unmatched column has a gradient"
            out.update({f"logits{lv}": x.half(), f"query_logits{lv}": ql, f"src{lv}": s64, f"tgt{lv}": t64,
                        f"loss64_{lv}": torch.stack([v.detach() for v in l64[lv]]),
                        f"loss32_{lv}": torch.stack([v.detach() for v in l32[lv]]),
                        f"dlogits64_{lv}": f.grad[:, s64], f"dquery64_{lv}": qlog.grad[0],
                        f"dlogits32_{lv}": f32.grad[:, s64], f"dquery32_{lv}": qlog32.grad[0]})
        path = os.path.join(HERE, f"match_{name}.npz")
        np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
        print(name, "levels", len(s["levels"]), "matches", [len(a) for a, _ in seen64], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
