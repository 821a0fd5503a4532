"""Per-voxel torch-CPU restatement of the evaluation tables (the layout `SceneEvaluator.add_tables` takes), written from the
metric definitions with `torch.unique` and boolean masks - the checker of the HIP kernels of include/pasco_eval.h."""
import numpy as np
import torch

BINS = 16


def bins_of(conf):
    return (torch.bucketize(conf, torch.linspace(0, 1, BINS), right=True) - 1).clamp_min(0)


def binned(conf, correct):
    b = bins_of(conf)
    count = torch.stack([(b == i).sum() for i in range(BINS)]).numpy()
    cor = torch.stack([(correct & (b == i)).sum() for i in range(BINS)]).numpy()
    csum = np.array([conf[b == i].double().sum().item() for i in range(BINS)])
    return count, cor, csum


def ssc_tables(probs, conf, sem):
    """probs [S, C] fp32, conf [S] fp32, sem [S] uint8 -> cm / unknown / bins / nll."""
    C = probs.shape[1]
    known = sem != 255
    pred = probs.argmax(1)
    g, p = sem[known].long(), pred[known]
    pairs, cnt = torch.unique(g * C + p, return_counts=True)
    cm = np.zeros((C, C), np.int64)
    cm.reshape(-1)[pairs.numpy()] = cnt.numpy()
    out = {"cm": cm, "unknown": int((~known).sum())}
    bc, bk, bs, nll = [], [], [], []
    for grp in (p == 0, p != 0):
        c, k, s = binned(conf[known][grp], (p == g)[grp])
        bc.append(c); bk.append(k); bs.append(s)
        nll.append(float(-torch.log(probs[known][grp].gather(1, g[grp][:, None]) + 1e-12).double().sum()))
    out.update(bin_count=np.stack(bc), bin_correct=np.stack(bk), bin_conf=np.stack(bs), nll=np.array(nll))
    return out


def panoptic_tables(pan, vconf, sem, gt_id, gt_area, infos, n_classes):
    """pan [S] int32 pred ids and vconf [S] fp32 on the dense grid, gt_id [S] (0 at unknown), gt_area [G + 1]."""
    known = sem != 255
    P = max([int(e["id"]) for e in infos] + [int(pan.max()), 0])
    G = gt_area.shape[0] - 1
    pz = torch.where(known, pan, torch.zeros_like(pan)).long()
    area = np.zeros(P + 1, np.int64)
    ids, cnt = torch.unique(pz[known], return_counts=True)
    area[ids.numpy()] = cnt.numpy()
    inter = np.zeros((G + 1, P + 1), np.int64)
    keys, cnt = torch.unique(gt_id[known].long() * (P + 1) + pz[known], return_counts=True)
    inter.reshape(-1)[keys.numpy()] = cnt.numpy()
    mp = np.zeros(P + 1, np.int32)
    for p in range(1, P + 1):
        for g in range(1, G + 1):
            i = inter[g, p]
            if area[p] > 0 and i > 0 and 2 * i > area[p] + gt_area[g] - i:
                mp[p] = g
                break
    mapped = torch.from_numpy(mp).long()[pz]
    sel = (gt_id != 0) & (vconf != 0)
    mc, mk, ms = binned(vconf[sel], mapped[sel] == gt_id[sel].long())
    segs = [{"id": int(e["id"]), "category_id": int(e["category_id"]), "confidence": float(e["confidence"]),
             "logp": torch.log(torch.as_tensor(e["all_class_probs"]).float() + 1e-8).numpy()} for e in infos]
    return {"area": area, "inter": inter, "map": mp, "mask_count": mc, "mask_correct": mk, "mask_conf": ms, "segments": segs}


def scene_tables(probs, conf, sem, pan, vconf, gt_id, gt_area, infos, n_classes=20):
    t = ssc_tables(probs, conf, sem)
    t.update(panoptic_tables(pan, vconf, sem, gt_id, gt_area, infos, n_classes))
    return t
