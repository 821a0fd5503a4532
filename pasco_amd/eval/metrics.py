"""Scene-by-scene scoring of `PascoNet.step_inference` outputs: the numbers of the reference's three result tables
(README.md:392-460; printers in pasco/models/utils.py:22-117).

Per scene and output the device makes small tables (include/pasco_eval.h): the SSC confusion and calibration bins over the
dense sites, the (gt id, pred id) intersections and the pred areas over the sparse panoptic rows, the IoU > 0.5 match and the
mask calibration bins.  Everything after that is bookkeeping on those tables, here on the host, in the order and precision
the reference uses (`SSCMetrics`, `PQStat`, `UncertaintyMetrics`: pasco/models/metrics.py:74-691,
pasco/loss/panoptic_quality.py:15-236), so that the printed tables carry the same digits:
  * SSC: completion and per-class tp / fp / fn over the known sites; per-scene ECE (pred == 0 vs pred != 0 sites)
    averaged over scenes, NLL pooled over voxels;
  * PQ: pairs of the same category; a stuff pair adds its IoU to `all_iou` / `all_n` whatever the IoU and counts its pred as
    matched, any pair with IoU > 0.5 is a true positive; GT areas are the reference's whole-mask counts, pred areas are
    recounted after the unknown zeroing; the IoU and its sums are fp32 as the reference's tensors are;
  * uncertainty: per-segment confidence / correctness / NLL pooled over all segments of all scenes (the NLL label of an
    unmatched segment is n_classes, the log takes + 1e-8), the mask ECE averaged over scenes (0 for a scene without rows).
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .gt import GroundTruth
from .lib import BINS, ECE_COUNTS, ECE_SUMS, MAX_GT, MAX_PRED, SSC_SUMS, ssc_counts

F32 = np.float32
THING_IDS = (1, 2, 3, 4, 5, 6, 7, 8)
CLASS_NAMES = ("empty", "car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist", "motorcyclist",
               "road", "parking", "sidewalk", "other-ground", "building", "fence", "vegetation", "trunk", "terrain", "pole",
               "traffic-sign")


def calibration_error(count, correct, conf_sum) -> float:
    """L1 calibration error of uniform bins from per-bin (count, correct, sum of confidence): torchmetrics'
    binary_calibration_error on the samples the bins were counted from, as fp32 (0 / 0 = NaN for no sample)."""
    count = np.asarray(count, np.float64)
    total = count.sum()
    if total == 0:
        return float("nan")
    with np.errstate(invalid="ignore", divide="ignore"):
        conf_bin = np.nan_to_num(np.asarray(conf_sum, np.float64) / count)
        acc_bin = np.nan_to_num(np.asarray(correct, np.float64) / count)
    return float(F32(np.sum(np.abs(acc_bin - conf_bin) * (count / total))))


def _f32_add(a, b):
    """a + b with the reference's types: python floats stay double, anything that met a fp32 tensor is fp32."""
    if isinstance(a, F32) or isinstance(b, F32):
        return F32(F32(a) + F32(b))
    return a + b


def _f32_div(a, b):
    if isinstance(a, F32) or isinstance(b, F32):
        return F32(F32(a) / F32(b))
    return a / b


class _PQCat:
    __slots__ = ("iou", "all_iou", "all_n", "tp", "fp", "fn")

    def __init__(self):
        self.iou, self.all_iou, self.all_n, self.tp, self.fp, self.fn = 0.0, 0.0, 0.0, 0, 0, 0


class _Output:
    """Accumulators of one output (subnet i or the ensemble) over scenes."""

    def __init__(self, n_classes: int):
        C = n_classes
        self.compl = np.zeros(3, np.int64)
        self.tps, self.fps, self.fns = np.zeros(C), np.zeros(C), np.zeros(C)
        self.ece = np.zeros(2)              # empty, nonempty: sums of per-scene values
        self.ece_count = 0.0
        self.nll = np.zeros(2)
        self.n_vox = np.zeros(2)
        self.pq: "OrderedDict[int, _PQCat]" = OrderedDict()
        self.ins_conf: List[float] = []
        self.ins_correct: List[bool] = []
        self.ins_logp: List[float] = []
        self.mask_ece = 0.0
        self.count = 0.0

    def cat(self, c: int) -> _PQCat:
        if c not in self.pq:
            self.pq[c] = _PQCat()
        return self.pq[c]

    def __iadd__(self, o: "_Output"):
        self.compl += o.compl
        self.tps += o.tps
        self.fps += o.fps
        self.fns += o.fns
        self.ece += o.ece
        self.ece_count += o.ece_count
        self.nll += o.nll
        self.n_vox += o.n_vox
        for c, s in o.pq.items():
            d = self.cat(c)
            d.iou = _f32_add(d.iou, s.iou)
            d.tp += s.tp
            d.fp += s.fp
            d.fn += s.fn
            d.all_iou = _f32_add(d.all_iou, s.all_iou)
            d.all_n += s.all_n
        self.ins_conf += o.ins_conf
        self.ins_correct += o.ins_correct
        self.ins_logp += o.ins_logp
        self.mask_ece += o.mask_ece
        self.count += o.count
        return self


class SceneEvaluator:
    """Scores M + 1 outputs per scene (the M subnets, then the ensemble) as the reference's test loop does
    (`Net.step_inference(eval=True)` -> `evaluate_all`, net_panoptic_sparse.py:539-760).

        ev = SceneEvaluator(n_outputs=M + 1)
        outs, sem_probs, _ = net.step_inference(...)
        ev.add(outs, sem_probs, GroundTruth.from_labels(sem, ins, ev.thing_ids, device="cuda"))
        print(ev.tables())

    `add` launches the evaluation kernels for every output on the current stream and reads their tables back with one
    device->host copy.  `add_tables` takes the same tables from elsewhere (tests feed it a torch restatement)."""

    def __init__(self, n_classes: int = 20, thing_ids: Sequence[int] = THING_IDS, n_outputs: int = 2,
                 class_names: Optional[Sequence[str]] = None):
        self.n_classes = int(n_classes)
        self.thing_ids = tuple(int(t) for t in thing_ids)
        self.n_outputs = int(n_outputs)
        self.class_names = tuple(class_names) if class_names is not None else (
            CLASS_NAMES if n_classes == len(CLASS_NAMES) else tuple(f"class {i}" for i in range(n_classes)))
        self.out = [_Output(self.n_classes) for _ in range(self.n_outputs)]
        self.scenes = 0
        self._ws = {}
        self.last_add_tables = None

    # ---- device side ------------------------------------------------------------------------------------------------
    def _workspace(self, key, nbytes: int, device) -> torch.Tensor:
        t = self._ws.get((key, device))
        if t is None or t.numel() * 8 < nbytes:
            t = torch.empty(max(1, (nbytes + 7) // 8), dtype=torch.int64, device=device)
            self._ws[(key, device)] = t
        return t

    def add(self, outs: Sequence, sem_probs: Sequence[torch.Tensor], gt: GroundTruth,
            ssc_confidences: Optional[Sequence[torch.Tensor]] = None) -> None:
        """`outs`: the `PanopticResult`s of `PascoNet.panoptic` / `step_inference` (each holds "ssc_confidence" unless
        `ssc_confidences` is given); `sem_probs`: the [C, X, Y, Z] class probabilities of the same outputs."""
        from .lib import eval_lib
        if len(outs) != self.n_outputs or len(sem_probs) != self.n_outputs:
            raise ValueError(f"{len(outs)} outputs / {len(sem_probs)} probability grids, the evaluator holds {self.n_outputs}")
        lib = eval_lib()
        dev = sem_probs[0].device
        C = int(sem_probs[0].shape[0])
        if C != self.n_classes:
            raise ValueError(f"{C} classes in the probabilities, the evaluator scores {self.n_classes}")
        grid = tuple(int(v) for v in sem_probs[0].shape[1:])
        if grid != tuple(gt.shape):
            raise ValueError(f"output grid {grid} and ground-truth grid {tuple(gt.shape)} differ")
        self._check_labels(gt)
        S = gt.semantic.numel()
        G = gt.n_gt
        if G > MAX_GT:
            raise ValueError(f"{G} ground-truth segments, the evaluation kernels take at most {MAX_GT}")
        gt = gt.to(dev)
        plan, total = [], 0

        def region(n):
            nonlocal total
            off = total
            total += int(n)
            return off

        rows = []
        for i, o in enumerate(outs):
            coords, scene_size, min_C, pan, vconf = panoptic_rows(o)
            if tuple(int(v) for v in scene_size) != grid:
                raise ValueError(f"output {i}: panoptic rows on a {tuple(scene_size)} grid, probabilities on {grid}")
            infos = o["segments_infos"][0]
            P = max([int(e["id"]) for e in infos] + [0])       # rows carry ids of the table (the kernels skip any other)
            if P > MAX_PRED:
                raise ValueError(f"output {i}: segment id {P}, the evaluation kernels take at most {MAX_PRED}")
            rows.append((coords, min_C, pan, vconf, infos, P))
            plan.append(dict(ssc_c=region(ssc_counts(C)), ssc_s=region(SSC_SUMS), area=region(P + 1),
                             inter=region((G + 1) * (P + 1)), map=region((P + 2) // 2), ece_c=region(ECE_COUNTS),
                             ece_s=region(ECE_SUMS), logp=region((len(infos) * (C + 1) + 1) // 2)))
        buf = torch.zeros(max(total, 1), dtype=torch.int64, device=dev)
        base = buf.data_ptr()
        ptr = lambda off: base + 8 * off
        X, Y, Z = grid
        for i, (o, (coords, min_C, pan, vconf, infos, P)) in enumerate(zip(outs, rows)):
            p = plan[i]
            probs = _rows_of(sem_probs[i])
            conf = (ssc_confidences[i] if ssc_confidences is not None else o["ssc_confidence"]).reshape(-1)
            conf = conf.contiguous().float()
            ws = self._workspace("ssc", lib.ssc_workspace_bytes(S, C), dev)
            lib.ssc(probs, conf, gt.semantic, ws, ptr(p["ssc_c"]), ptr(p["ssc_s"]))
            c = coords[:, 1:].to(torch.int64) - min_C.to(device=dev, dtype=torch.int64).reshape(1, 3)
            inside = (c >= 0).all(1) & (c[:, 0] < X) & (c[:, 1] < Y) & (c[:, 2] < Z)
            site = torch.where(inside, (c[:, 0] * Y + c[:, 1]) * Z + c[:, 2], torch.full_like(c[:, 0], -1)).contiguous()
            pan32 = pan.to(torch.int32).contiguous()
            lib.panop_pairs(site, pan32, gt.semantic, gt.panoptic, P, G, ptr(p["area"]), ptr(p["inter"]))
            lib.match(ptr(p["area"]), gt.gt_area, ptr(p["inter"]), P, G, ptr(p["map"]))
            ws = self._workspace("ece", lib.ece_workspace_bytes(site.numel()), dev)
            lib.mask_ece(site, pan32, vconf.contiguous().float(), gt.panoptic, ptr(p["map"]), P, ws, ptr(p["ece_c"]),
                         ptr(p["ece_s"]))
            if infos:
                probs_k = torch.stack([e["all_class_probs"].to(dev).float() for e in infos])
                n = probs_k.numel()
                buf[p["logp"]:p["logp"] + (n + 1) // 2].view(torch.float32)[:n].copy_(torch.log(probs_k + 1e-8).reshape(-1))
        host = buf.cpu()                                              # the one device -> host copy of the scene
        tables = []
        for i, (coords, min_C, pan, vconf, infos, P) in enumerate(rows):
            p = plan[i]
            h = host.numpy()
            sc = h[p["ssc_c"]:p["ssc_c"] + ssc_counts(C)]
            ss = h[p["ssc_s"]:p["ssc_s"] + SSC_SUMS].view(np.float64)
            ec = h[p["ece_c"]:p["ece_c"] + ECE_COUNTS]
            es = h[p["ece_s"]:p["ece_s"] + ECE_SUMS].view(np.float64)
            logp = h[p["logp"]:p["logp"] + (len(infos) * (C + 1) + 1) // 2].view(np.float32)[:len(infos) * (C + 1)]
            tables.append({
                "cm": sc[:C * C].reshape(C, C).copy(), "unknown": int(sc[C * C]),
                "bin_count": sc[C * C + 1:C * C + 1 + 2 * BINS].reshape(2, BINS).copy(),
                "bin_correct": sc[C * C + 1 + 2 * BINS:].reshape(2, BINS).copy(),
                "bin_conf": ss[:2 * BINS].reshape(2, BINS).copy(), "nll": ss[2 * BINS:].copy(),
                "area": h[p["area"]:p["area"] + P + 1].copy(),
                "inter": h[p["inter"]:p["inter"] + (G + 1) * (P + 1)].reshape(G + 1, P + 1).copy(),
                "map": h[p["map"]:p["map"] + (P + 2) // 2].view(np.int32)[:P + 1].copy(),
                "mask_count": ec[:BINS].copy(), "mask_correct": ec[BINS:].copy(), "mask_conf": es.copy(),
                "segments": [{"id": int(e["id"]), "category_id": int(e["category_id"]), "confidence": float(e["confidence"]),
                              "logp": logp[k * (C + 1):(k + 1) * (C + 1)].copy()} for k, e in enumerate(infos)],
            })
        self.last_add_tables = tables
        self.add_tables(tables, gt)

    # ---- host side --------------------------------------------------------------------------------------------------
    def add_tables(self, tables: Sequence[Dict], gt: GroundTruth) -> None:
        """One scene from its tables (one dict per output, the layout `add` reads back; see tests/eval_restate.py)."""
        if len(tables) != self.n_outputs:
            raise ValueError(f"{len(tables)} outputs, the evaluator holds {self.n_outputs}")
        self._check_labels(gt)
        gt_cat = dict(zip(gt.seg_id.tolist(), gt.seg_cat.tolist()))
        gt_area = dict(zip(gt.seg_id.tolist(), gt.seg_area.tolist()))
        for acc, t in zip(self.out, tables):
            self._ssc(acc, t)
            self._panoptic(acc, t, gt, gt_cat, gt_area)
        self.scenes += 1

    def _check_labels(self, gt: GroundTruth) -> None:
        # pe_ssc skips a site labelled c <= label < 255: it would drop out of every table without a word
        if gt.max_label >= self.n_classes:
            raise ValueError(f"semantic label {gt.max_label} in the ground truth, the evaluator scores {self.n_classes} "
                             f"classes (0 .. {self.n_classes - 1}, 255 = unknown)")

    def _ssc(self, acc: _Output, t: Dict) -> None:
        cm = np.asarray(t["cm"], np.int64)
        tp = np.diag(cm)
        acc.tps += tp
        acc.fps += cm.sum(0) - tp
        acc.fns += cm.sum(1) - tp
        acc.compl += (cm[1:, 1:].sum(), cm[0, 1:].sum(), cm[1:, 0].sum())
        for g in range(2):
            acc.ece[g] += calibration_error(t["bin_count"][g], t["bin_correct"][g], t["bin_conf"][g])
        acc.ece_count += 1
        acc.nll += np.asarray(t["nll"], np.float64)
        acc.n_vox += np.asarray(t["bin_count"], np.float64).sum(1)

    def _panoptic(self, acc: _Output, t: Dict, gt: GroundTruth, gt_cat: Dict[int, int], gt_area: Dict[int, int]) -> None:
        area = np.asarray(t["area"], np.int64)
        inter = np.asarray(t["inter"], np.int64)
        pred_cat = {}
        for e in t["segments"]:
            if e["id"] < area.shape[0] and area[e["id"]] > 0:
                pred_cat[e["id"]] = e["category_id"]
        things = self.thing_ids
        gt_matched, pred_matched = set(), set()
        pred2gt = {}
        gs, ps = np.nonzero(inter)
        for g, p in zip(gs.tolist(), ps.tolist()):               # ascending (gt id, pred id): np.unique's order
            if g == 0 or p == 0 or g not in gt_cat or p not in pred_cat:
                continue
            it = int(inter[g, p])
            union = int(area[p]) + int(gt_area[g]) - it
            if 2 * it > union:                                    # find_matched_segment(threshold=0.5), any category
                pred2gt[p] = g
            if gt_cat[g] != pred_cat[p]:
                continue
            iou = F32(F32(it) / F32(union))
            c = acc.cat(gt_cat[g])
            if gt_cat[g] not in things:
                c.all_iou = _f32_add(c.all_iou, iou)
                c.all_n += 1
                pred_matched.add(p)
            if iou > 0.5:
                c.tp += 1
                c.iou = _f32_add(c.iou, iou)
                gt_matched.add(g)
                pred_matched.add(p)
        for g in gt.seg_id.tolist():
            if g not in gt_matched:
                acc.cat(gt_cat[g]).fn += 1
        for e in t["segments"]:
            if e["id"] in pred_cat and e["id"] not in pred_matched:
                acc.cat(e["category_id"]).fp += 1
        for e in t["segments"]:
            if e["id"] not in pred_cat:
                continue
            g = pred2gt.get(e["id"])
            label = self.n_classes if g is None else gt_cat[g]
            acc.ins_conf.append(float(F32(e["confidence"])))
            acc.ins_correct.append(g is not None and gt_cat[g] == e["category_id"])
            acc.ins_logp.append(float(e["logp"][label]))
        if int(np.sum(t["mask_count"])) == 0:
            acc.mask_ece += 0
        else:
            acc.mask_ece += calibration_error(t["mask_count"], t["mask_correct"], t["mask_conf"])
        acc.count += 1

    def __iadd__(self, other: "SceneEvaluator") -> "SceneEvaluator":
        if (other.n_classes, other.thing_ids, other.n_outputs) != (self.n_classes, self.thing_ids, self.n_outputs):
            raise ValueError("evaluators of different configurations")
        for a, b in zip(self.out, other.out):
            a += b
        self.scenes += other.scenes
        return self

    # ---- results ----------------------------------------------------------------------------------------------------
    def _ssc_stats(self, a: _Output, step_time: Optional[float]) -> Dict:
        tp, fp, fn = (int(v) for v in a.compl)
        if tp != 0:
            precision, recall, iou = tp / (tp + fp), tp / (tp + fn), tp / (tp + fp + fn)
        else:
            precision, recall, iou = 0, 0, 0
        iou_ssc = a.tps / (a.tps + a.fps + a.fns + 1e-5)
        n = a.ece_count
        return {"precision": precision, "recall": recall, "iou": iou, "iou_ssc": iou_ssc,
                "iou_ssc_mean": np.mean(iou_ssc[1:]),
                "empty_ece": a.ece[0] / n if n else 0, "nonempty_ece": a.ece[1] / n if n else 0,
                "empty_nll": a.nll[0] / a.n_vox[0] if a.n_vox[0] else 0,
                "nonempty_nll": a.nll[1] / a.n_vox[1] if a.n_vox[1] else 0,
                "inference_time": 0.0 if step_time is None else float(step_time)}

    def _pq_average(self, a: _Output, isthing: Optional[bool]):
        pq_dagger, pq, sq, rq, n = 0, 0, 0, 0, 0
        per_class = {}
        for label, s in a.pq.items():
            if label == 0:
                continue
            if isthing is not None and isthing != (label in self.thing_ids):
                continue
            if s.tp + s.fp + s.fn == 0:
                per_class[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
                continue
            n += 1
            den = s.tp + 0.5 * s.fp + 0.5 * s.fn
            pq_c = _f32_div(s.iou, den)
            sq_c = _f32_div(s.iou, s.tp) if s.tp != 0 else 0
            rq_c = s.tp / den
            per_class[label] = {"pq": pq_c, "sq": sq_c, "rq": rq_c}
            pq, sq, rq = _f32_add(pq, pq_c), _f32_add(sq, sq_c), rq + rq_c
            if isthing is None:
                pq_dagger = _f32_add(pq_dagger, pq_c if label in self.thing_ids else _f32_div(s.all_iou, max(s.all_n, 1)))
        n = max(n, 1)
        return {"pq_dagger": _f32_div(pq_dagger, n), "pq": _f32_div(pq, n), "sq": _f32_div(sq, n), "rq": rq / n,
                "n": n}, per_class

    def _uncertainty_stats(self, a: _Output) -> Dict:
        mask_ece = a.mask_ece / a.count if a.count else 0
        if a.ins_conf:
            nll = float(-np.mean(np.asarray(a.ins_logp, np.float64)))
            conf = torch.tensor(a.ins_conf, dtype=torch.float32)
            idx = (torch.bucketize(conf, torch.linspace(0, 1, BINS), right=True) - 1).clamp_min(0).numpy()
            cnt = np.bincount(idx, minlength=BINS)
            cor = np.bincount(idx, weights=np.asarray(a.ins_correct, np.float64), minlength=BINS)
            csum = np.bincount(idx, weights=conf.double().numpy(), minlength=BINS)
            ins_ece = F32(calibration_error(cnt, cor, csum))
        else:
            nll, ins_ece = 0.0, 0
        return {"mask_ece": mask_ece, "ins_ece": ins_ece, "ins_nll": nll, "count": len(a.ins_conf)}

    def stats(self, step_time: Optional[float] = None) -> List[Dict]:
        """Per output: {"ssc": SSCMetrics.get_stats keys, "pq": {"All" / "Things" / "Stuff": pq_average,
        "per_class": {class: {"pq", "sq", "rq"}}}, "uncertainty": {"ins_ece", "ins_nll", "count", "mask_ece"}}."""
        res = []
        for a in self.out:
            pq = {}
            for name, isthing in (("All", None), ("Things", True), ("Stuff", False)):
                pq[name], per_class = self._pq_average(a, isthing)
                if name == "All":
                    pq["per_class"] = per_class
            res.append({"ssc": self._ssc_stats(a, step_time), "pq": pq, "uncertainty": self._uncertainty_stats(a)})
        return res

    def tables(self, step_time: Optional[float] = None) -> str:
        """The reference's three tables (utils.py:22-117: panoptic + SSC, per-class PQ / SQ / RQ, uncertainty), rows
        `subnet i` and `ensemble`.  `step_time` fills the "inference time" column (the reference's caller passes 0)."""
        st = self.stats(step_time)
        pct = lambda v: F32(F32(v) * F32(100)) if isinstance(v, F32) else v * 100
        name = lambda i: "ensemble" if i == len(st) - 1 else "subnet {}".format(i)
        lines = ["=====================================",
                 "method, P, R, IoU, mIoU, All PQ dagger, All PQ, All SQ, All RQ, Thing PQ, Thing SQ, Thing RQ, Stuff PQ, "
                 "Stuff SQ, Stuff RQ"]
        for i, s in enumerate(st):
            ss, p = s["ssc"], s["pq"]
            vals = [ss["precision"] * 100, ss["recall"] * 100, ss["iou"] * 100, ss["iou_ssc_mean"] * 100,
                    pct(p["All"]["pq_dagger"])] + [pct(p[g][m]) for g in ("All", "Things", "Stuff") for m in ("pq", "sq", "rq")]
            lines.append(name(i) + ", " + ", ".join("{:0.2f}".format(v) for v in vals))
        lines.append("=====================================")
        for metric in ("pq", "sq", "rq"):
            lines.append("==> " + metric)
            lines.append("method" + ", " + ", ".join(self.class_names[1:]))
            for i, s in enumerate(st):
                pc = s["pq"]["per_class"]
                ts = [pc[c][metric] if c in pc else 0 for c in range(1, len(self.class_names))]
                lines.append(name(i) + ", " + ", ".join("{:0.2f}".format(pct(t)) for t in ts))
        lines.append("=====================================")
        lines.append("method, ins ece, ins nll, ssc nonempty ece, ssc empty ece, ssc nonempty nll, ssc empty nll,  count, "
                     "inference time")
        for i, s in enumerate(st):
            u, ss = s["uncertainty"], s["ssc"]
            lines.append("{},  {:0.4f}, {:0.4f}, {:0.4f}, {:0.4f}, {:0.4f}, {:0.4f}, {}, {:0.2f}".format(
                name(i), u["ins_ece"], u["ins_nll"], ss["nonempty_ece"], ss["empty_ece"], ss["nonempty_nll"],
                ss["empty_nll"], u["count"], ss["inference_time"]))
        return "\n".join(lines) + "\n"


def _rows_of(sem_prob: torch.Tensor) -> torch.Tensor:
    """[C, X, Y, Z] -> channels-last rows [S, C]: a view when the grid was made from such rows (PascoNet.ensemble keeps
    them as cache["sem_rows"]), a copy otherwise."""
    r = sem_prob.permute(1, 2, 3, 0)
    if not r.is_contiguous():
        r = r.contiguous()
    return r.reshape(-1, sem_prob.shape[0]).float()


def panoptic_rows(res):
    """(coords [N, 4] int32, scene_size, min_C, panoptic id [N], vox_conf [N]) of a panoptic output, from its sparse rows."""
    if hasattr(res, "sparse_rows"):
        got = res.sparse_rows()
        if got is not None:
            return got
    raise ValueError("the panoptic output holds no sparse rows (a device-path `PanopticResult` of one scene is needed)")
