"""Frame preparation on the device (include/pasco_frame.h) for both datasets.

The host path (`build_item` / `build_item_kitti360`) crops, voxelises and transforms the points once per subnet and
resamples both label grids under every subnet's transform, only to read the bounds min_C / max_C off them.  Here the raw
arrays go to the device as they were read, one copy each; `pf_points` makes the feature rows once (they do not depend on
T: the subnets share one tensor), `pf_transform_coords` the voxel indices of all subnets in one launch, and
`pf_label_bounds` the bounds without building any grid.  What comes back to the host is one copy of 1 + 6 M int64: the
kept count and the bounds.  Everything is bit-equal to the host path (tests/test_hip_frame.py)."""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from .frame_lib import BOUNDS, Segment, box_upper_bound, frame_lib
from .semantic_kitti import collate, completion_bounds

INT32_MAX = 2 ** 31 - 1


def upload(a, device) -> torch.Tensor:
    """A host array on the device as it is (one copy), fp32 if it is floating."""
    t = torch.as_tensor(a).to(device)
    return t.float() if t.is_floating_point() and t.dtype != torch.float32 else t


def prepare(pts: torch.Tensor, sem: torch.Tensor, ins: torch.Tensor, Ts: Sequence[torch.Tensor], *, lo, hi, lo_fp64,
            hi_fp64, origin, voxel: float, centre_fp64: bool, pre: Sequence[Segment] = (), post: Sequence[Segment] = (),
            complete_scale: int = 8, point_labels: Optional[torch.Tensor] = None) -> Dict:
    """pts fp32 [P, 4], sem / ins uint8 [X, Y, Z], the segments: all on one device.  -> the dict `collate` returns, its
    tensors on the device except the bounds (host int32, as the host path makes them)."""
    lib, dev, M = frame_lib(), pts.device, len(Ts)
    Ts = [torch.as_tensor(T).float().cpu() for T in Ts]
    args = lib.points_args(lo, hi, lo_fp64, hi_fp64, origin, voxel, centre_fp64, pre, post)
    small = torch.empty(1 + 6 * M, dtype=torch.int64, device=dev)     # kept count | M x 12 int32 bounds
    n = int(pts.shape[0])
    feat = torch.empty((n, lib.channels(args)), dtype=torch.float32, device=dev)
    vox = torch.empty((n, 3), dtype=torch.float64, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev) if point_labels is not None else None
    ws = torch.empty(max(int(lib.lib.pf_points_workspace_bytes(n)), 4), dtype=torch.uint8, device=dev)
    lib.points_into(pts, args, feat, vox, src, small[:1], ws)
    coords = lib.transform_coords(vox, Ts, n_dev=small[:1])
    bounds = small[1:].view(torch.int32).view(M, BOUNDS)
    lib.label_bounds(sem, ins, Ts, [torch.inverse(T) for T in Ts], box_upper_bound(tuple(sem.shape), Ts), out=bounds)
    host = small.cpu()
    K = int(host[0])
    hb = host[1:].view(torch.int32).view(M, BOUNDS)
    feat = feat[:K]
    xyz = feat[:, -3:].double() - torch.tensor(origin, dtype=torch.float64, device=dev)
    plab = None if point_labels is None else point_labels[src[:K].long()]
    items = []
    for m, T in enumerate(Ts):
        lo_c, hi_c = hb[m, 6:9].clone(), hb[m, 9:12].clone()
        if int(lo_c.max()) == INT32_MAX:
            raise ValueError("frame has no known voxel that survives the resampling under T (the host path fails there too)")
        min_c, max_c = completion_bounds(lo_c, hi_c, complete_scale)
        items.append({"in_feat": feat, "in_coord": coords[m, :K], "T": T, "min_C": min_c, "max_C": max_c, "xyz": xyz,
                      "input_pcd_instance_label": plab})
    return collate(items, complete_scale)
