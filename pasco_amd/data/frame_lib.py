"""ctypes binding of include/pasco_frame.h (the `pf_*` entry points of libpascohip.so): frame preparation on the device.

Kept apart from `me.backend` on purpose, like `eval.lib`: the CPU oracle binds `me.backend._SIGNATURES` and has no frame
kernels.  Every method takes device tensors, enqueues on the caller's current stream and returns nothing."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from .._clib import FamilyLib, shared

PF_ABI_VERSION = 1       # include/pasco_frame.h PF_ABI_VERSION this binding was written against
MAX_SEGMENTS = 4
MAX_M = 8
BOUNDS = 12


class Segment(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("row_stride", C.c_int64), ("col_stride", C.c_int64), ("width", C.c_int32)]


class PointsArgs(C.Structure):
    _fields_ = [("lo", C.c_double * 3), ("hi", C.c_double * 3), ("lo_fp64", C.c_int32 * 3), ("hi_fp64", C.c_int32 * 3),
                ("origin", C.c_double * 3), ("voxel", C.c_double), ("centre_fp64", C.c_int32), ("n_pre", C.c_int32),
                ("n_seg", C.c_int32), ("seg", Segment * MAX_SEGMENTS)]


_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "points_channels": [C.POINTER(PointsArgs)],
    "points_workspace_bytes": [_i64],
    "points": [_vp, _i64, C.POINTER(PointsArgs), _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "transform_coords": [_vp, _i32, _i64, _vp, _vp, _i32, _vp, _vp],
    "bounds_workspace_bytes": [_i32],
    "label_bounds": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "points_workspace_bytes": _i64, "bounds_workspace_bytes": _i64}


def _seg(t: torch.Tensor, width: int, row_stride: int, col_stride: int) -> Segment:
    assert t.dtype == torch.float32 and t.is_cuda
    return Segment(t.data_ptr(), row_stride, col_stride, width)


def segment(t: torch.Tensor) -> Segment:
    """A [P, w] (any strides) fp32 device tensor as a pass-through segment."""
    return _seg(t, int(t.shape[1]), int(t.stride(0)), int(t.stride(1)))


def _mats(Ts: Sequence[torch.Tensor]):
    if not 1 <= len(Ts) <= MAX_M:
        raise ValueError(f"pf: {len(Ts)} transforms, 1..{MAX_M} supported")
    flat = torch.stack([torch.as_tensor(T, dtype=torch.float32).cpu().reshape(4, 4) for T in Ts]).reshape(-1)
    return (C.c_float * flat.numel())(*flat.tolist())


class FrameLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pf_", PF_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    @staticmethod
    def points_args(lo, hi, lo_fp64, hi_fp64, origin, voxel: float, centre_fp64: bool,
                    pre: Sequence[Segment] = (), post: Sequence[Segment] = ()) -> PointsArgs:
        segs = list(pre) + list(post)
        if len(segs) > MAX_SEGMENTS:
            raise ValueError(f"pf_points: {len(segs)} segments, at most {MAX_SEGMENTS}")
        a = PointsArgs()
        a.lo[:], a.hi[:] = [float(v) for v in lo], [float(v) for v in hi]
        a.lo_fp64[:], a.hi_fp64[:] = [int(bool(v)) for v in lo_fp64], [int(bool(v)) for v in hi_fp64]
        a.origin[:] = [float(v) for v in origin]
        a.voxel, a.centre_fp64, a.n_pre, a.n_seg = float(voxel), int(bool(centre_fp64)), len(pre), len(segs)
        for i, s in enumerate(segs):
            a.seg[i] = s
        return a

    def channels(self, args: PointsArgs) -> int:
        return int(self.lib.pf_points_channels(C.byref(args)))

    def points(self, pts: torch.Tensor, args: PointsArgs, want_src: bool = False):
        """pts fp32 [P, 4] on the device -> (feat fp32 [P, C], voxel fp64 [P, 3], src int32 [P] or None, kept int64 [1]),
        all on the device; rows >= kept are not written."""
        assert pts.is_cuda and pts.dtype == torch.float32 and pts.is_contiguous() and pts.dim() == 2 and pts.shape[1] == 4
        n, dev = int(pts.shape[0]), pts.device
        feat = torch.empty((n, self.channels(args)), dtype=torch.float32, device=dev)
        voxel = torch.empty((n, 3), dtype=torch.float64, device=dev)
        src = torch.empty(n, dtype=torch.int32, device=dev) if want_src else None
        kept = torch.empty(1, dtype=torch.int64, device=dev)
        ws = torch.empty(max(int(self.lib.pf_points_workspace_bytes(n)), 4), dtype=torch.uint8, device=dev)
        self.points_into(pts, args, feat, voxel, src, kept, ws)
        return feat, voxel, src, kept

    def points_into(self, pts, args, feat, voxel, src, kept, ws):
        self._ok(self.lib.pf_points(pts.data_ptr(), int(pts.shape[0]), C.byref(args), feat.data_ptr(), voxel.data_ptr(),
                                    None if src is None else src.data_ptr(), kept.data_ptr(), ws.data_ptr(),
                                    ws.numel(), self._stream(pts)), "points")

    def transform_coords(self, coords: torch.Tensor, Ts: Sequence[torch.Tensor], n_dev: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """coords fp64 or int64 [n, 3] on the device -> int64 [M, n, 3]; with `n_dev` (int64 [1] on the device) rows from
        n_dev[0] on are not written."""
        assert coords.is_cuda and coords.is_contiguous() and coords.dtype in (torch.float64, torch.int64)
        n = int(coords.shape[0])
        if out is None:
            out = torch.empty((len(Ts), n, 3), dtype=torch.int64, device=coords.device)
        self._ok(self.lib.pf_transform_coords(coords.data_ptr(), int(coords.dtype == torch.int64), n,
                                              None if n_dev is None else n_dev.data_ptr(), _mats(Ts), len(Ts),
                                              out.data_ptr(), self._stream(coords)), "transform_coords")
        return out

    def label_bounds(self, sem: torch.Tensor, ins: torch.Tensor, Ts: Sequence[torch.Tensor], Tinvs: Sequence[torch.Tensor],
                     box_bound: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sem / ins uint8 [X, Y, Z] on the device -> int32 [M, 12] on the device (see pasco_frame.h); `box_bound` int32
        [M, 6] host tensor sizing the second pass."""
        assert sem.is_cuda and sem.dtype == torch.uint8 and ins.dtype == torch.uint8 and sem.shape == ins.shape
        assert sem.is_contiguous() and ins.is_contiguous() and sem.dim() == 3
        M = len(Ts)
        if out is None:
            out = torch.empty((M, BOUNDS), dtype=torch.int32, device=sem.device)
        ws = torch.empty(int(self.lib.pf_bounds_workspace_bytes(M)), dtype=torch.uint8, device=sem.device)
        bb = box_bound.to(torch.int32).contiguous().reshape(-1)
        X, Y, Z = (int(v) for v in sem.shape)
        self._ok(self.lib.pf_label_bounds(sem.data_ptr(), ins.data_ptr(), X, Y, Z, _mats(Ts), _mats(Tinvs), M,
                                          (C.c_int32 * bb.numel())(*bb.tolist()), out.data_ptr(), ws.data_ptr(),
                                          ws.numel(), self._stream(sem)), "label_bounds")
        return out


def frame_lib() -> FrameLib:
    """The process-wide binding of libpascohip.so's frame kernels (a missing library is an error)."""
    return shared(FrameLib)


def box_upper_bound(grid: Tuple[int, int, int], Ts: Sequence[torch.Tensor], margin: int = 2) -> torch.Tensor:
    """Host-side upper bound of each subnet's sample box: the eight corners of the whole grid under T (fp64) plus a margin.
    It only sizes the launch of pf_label_bounds' second pass; the exact box is read on the device."""
    out = []
    corners = torch.tensor([[x, y, z] for x in (0, grid[0] - 1) for y in (0, grid[1] - 1) for z in (0, grid[2] - 1)],
                           dtype=torch.float64)
    mb = torch.tensor([0.0, -25.6, -2.0], dtype=torch.float64)
    for T in Ts:
        T = torch.as_tensor(T).double().cpu().reshape(4, 4)
        p = corners * 0.2 + 0.1 + mb
        q = (p @ T[:3, :3].T + T[:3, 3] - mb - 0.1) / 0.2
        out.append(torch.cat([torch.floor(q.min(0)[0]) - margin, torch.ceil(q.max(0)[0]) + margin]))
    return torch.stack(out).to(torch.int32)
