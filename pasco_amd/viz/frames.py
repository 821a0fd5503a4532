"""A saved frame (the pickle of `viz.outputs`) -> its images, on the device (`DeviceOps`, the pv_* kernels) or on the host
(`HostOps`, the numpy restatement): the same sequence of calls either way, so both write the same bytes.

File names are the ones the reference's drawing script uses.  It names the panoptic, mask and confidence images after the
LAST scale of its semantic loop (a loop variable that outlives the loop); the names are kept so both sets line up."""
from __future__ import annotations

from typing import Dict, Iterator, Sequence, Tuple

import numpy as np

from . import host
from .camera import preset

VIEW_NAMES = ("semantic", "panoptic", "mask", "vox_conf", "ins_conf")
FACE_FACTORS = (200, 228, 256)            # x, y and z faces: (c * f) >> 8
BACKGROUND = (255, 255, 255)


def segment_table(infos: Sequence[dict]) -> np.ndarray:
    """`pred_segments_info` of one frame -> int32 [4, n]: id, isthing, category, confidence (fp32 bits)."""
    if len(infos) > host.MAX_SEGMENTS:
        raise ValueError(f"{len(infos)} segments, the view kernels take {host.MAX_SEGMENTS}")
    t = np.zeros((4, len(infos)), np.int32)
    for s, info in enumerate(infos):
        t[0, s], t[1, s], t[2, s] = int(info["id"]), int(bool(info["isthing"])), int(info["category_id"])
        t[3, s] = np.float32(info.get("confidence", 0.0)).view(np.int32)
    return t


class HostOps:
    name = "cpu"

    def __init__(self, label_palette: np.ndarray, ramp_palette: np.ndarray):
        self.palettes = {"label": label_palette, "ramp": ramp_palette}

    def upload(self, arrays: Dict[str, np.ndarray]):
        return dict(arrays)

    def pool(self, grid, k):
        out, status = host.majority_pool(grid, k)
        if status:
            raise ValueError("majority pooling: a label outside 0 .. 31 and 255")
        return out

    def filter(self, conf, op, mask):
        return host.window_filter(conf, op, mask)

    def minmax(self, conf, sem):
        sel = conf[sem != 0]
        return (float(sel.min()), float(sel.max())) if sel.size else (0.0, 0.0)

    def compose(self, view, shape, **kw):
        return host.compose(view, shape, **kw)

    def image(self, colour, cam, size, supersample, palette) -> np.ndarray:
        bits = host.bricks(colour)
        n = size * supersample
        _, _, rgb, status = host.render(colour, bits, cam, n, n, self.palettes[palette], FACE_FACTORS, BACKGROUND)
        if status:
            raise RuntimeError(f"render: status {status}")
        return host.downsample(rgb, supersample)


class DeviceOps:
    name = "cuda"

    def __init__(self, label_palette: np.ndarray, ramp_palette: np.ndarray, device="cuda"):
        import torch
        from .lib import view_lib
        self.torch, self.lib, self.dev = torch, view_lib(), torch.device(device)
        self.palettes = {"label": torch.from_numpy(label_palette).to(self.dev), "ramp": torch.from_numpy(ramp_palette).to(self.dev)}

    def upload(self, arrays: Dict[str, np.ndarray]):
        """One host-to-device copy for all the grids of a frame: packed into one buffer (16-byte aligned parts)."""
        torch = self.torch
        offs, total = {}, 0
        for k, a in arrays.items():
            offs[k] = total
            total += (a.nbytes + 15) // 16 * 16
        buf = np.zeros(max(total, 16), np.uint8)
        for k, a in arrays.items():
            buf[offs[k]:offs[k] + a.nbytes] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
        d = torch.from_numpy(buf).to(self.dev)
        dt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}
        return {k: d[offs[k]:offs[k] + a.nbytes].view(dt[a.dtype]).reshape(a.shape) for k, a in arrays.items()}

    def pool(self, grid, k):
        out, status = self.lib.majority_pool(grid, k)
        if int(status.item()):
            raise ValueError("majority pooling: a label outside 0 .. 31 and 255")
        return out

    def filter(self, conf, op, mask):
        return self.lib.window_filter(conf, op, mask)

    def minmax(self, conf, sem):
        torch = self.torch
        keep = sem != 0
        lo = torch.where(keep, conf, torch.full_like(conf, float("inf"))).min()
        hi = torch.where(keep, conf, torch.full_like(conf, float("-inf"))).max()
        lo, hi = torch.stack([lo, hi]).tolist()
        return (lo, hi) if lo <= hi else (0.0, 0.0)

    def compose(self, view, shape, **kw):
        return self.lib.compose(view, shape, **kw)

    def image(self, colour, cam, size, supersample, palette) -> np.ndarray:
        n = size * supersample
        bits = self.lib.bricks(colour)
        cam_d = self.torch.from_numpy(cam).to(self.dev)
        _, _, rgb, status = self.lib.render(colour, bits, cam_d, n, n, self.palettes[palette], FACE_FACTORS, BACKGROUND)
        out = self.lib.downsample(rgb, supersample)
        host_img = self.torch.cat([out.reshape(-1), status.view(self.torch.uint8)]).cpu().numpy()   # one copy per image
        if host_img[-4:].any():
            raise RuntimeError(f"render: status {host_img[-4:].view(np.int32)[0]}")
        return host_img[:-4].reshape(size, size, 3)


def frame_images(pred: dict, ops, method: str, frame: str, i_subnet: int, views: Sequence[str] = VIEW_NAMES,
                 scales: Sequence[int] = (1, 2, 4), camera: str = "behind", size: int = 1400, supersample: int = 2,
                 filt: str = "median") -> Iterator[Tuple[str, np.ndarray]]:
    """Yields (file name, uint8 [size, size, 3]) for every requested view of one saved frame."""
    pan = np.asarray(pred["pred_panoptic_seg"]).squeeze().astype(np.int32)
    shape = pan.shape
    arrays = {"conf": np.asarray(pred["vox_confidence_denses"], np.float32).reshape(shape),
              "pan": pan, "seg": segment_table(pred["pred_segments_info"][0]),
              "sem": np.asarray(pred["ssc_pred"]).reshape(shape).astype(np.uint8),
              "gt": np.asarray(pred["semantic_label_origin"]).reshape(shape).astype(np.uint8)}
    seg_host = arrays["seg"]
    n_seg = seg_host.shape[1]
    if n_seg == 0:
        arrays["seg"] = np.zeros((4, 1), np.int32)          # nothing of it is read
    d = ops.upload(arrays)
    seg = d["seg"] if n_seg else None
    cam = lambda shp: preset(camera, shp, size * supersample, size * supersample)
    last = scales[-1] if scales else 1

    if "semantic" in views:
        for k in scales:
            for src, tag in (("sem", "sem"), ("gt", "sem_gt")):
                grid = d[src] if k == 1 else ops.pool(d[src], k)
                colour = ops.compose("semantic", grid.shape, sem=grid)
                yield f"{method}_{tag}_{frame}_{k}_{i_subnet}.png", ops.image(colour, cam(grid.shape), size, supersample, "label")
    if "panoptic" in views:
        colour = ops.compose("panoptic", shape, panoptic=d["pan"], seg=seg, sem=d["sem"])
        yield f"{method}_panop_pred_{frame}_{last}_{i_subnet}.png", ops.image(colour, cam(shape), size, supersample, "label")
    if "mask" in views:
        colour = ops.compose("mask", shape, panoptic=d["pan"], seg=seg)
        yield f"{method}_mask_pred_{frame}_{last}_{i_subnet}.png", ops.image(colour, cam(shape), size, supersample, "label")
    if "vox_conf" in views:
        conf = d["conf"] if filt == "raw" else ops.filter(d["conf"], filt, d["sem"])
        vmin, vmax = ops.minmax(conf, d["sem"])
        colour = ops.compose("vox_conf", shape, sem=d["sem"], conf=conf, vmin=vmin, vmax=vmax)
        yield f"{method}_vox_conf_{frame}_{last}_{i_subnet}.png", ops.image(colour, cam(shape), size, supersample, "ramp")
    if "ins_conf" in views:
        things = seg_host[3, seg_host[1] != 0].view(np.float32)
        vmin, vmax = (float(things.min()), float(things.max())) if things.size else (0.0, 0.0)
        colour = ops.compose("ins_conf", shape, panoptic=d["pan"], seg=seg, vmin=vmin, vmax=vmax)
        yield f"{method}_ins_conf_{frame}_{last}_{i_subnet}.png", ops.image(colour, cam(shape), size, supersample, "ramp")
