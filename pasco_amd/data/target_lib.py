"""ctypes binding of include/pasco_target.h (the `pt_*` entry points of libpascohip.so): the training targets on the device.

Like `frame_lib`: every method takes device tensors, enqueues on the caller's current stream and reads nothing back;
`data.targets` is the surface that uses it."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .._clib import FamilyLib, shared
from .frame_lib import _mats

PT_ABI_VERSION = 1       # include/pasco_target.h PT_ABI_VERSION this binding was written against
MAX_M = 8
BOUNDS = 18
CROP_BOUNDS = 12
TABLE = 768
MAX_T = 128


class SubnetOut(C.Structure):
    _fields_ = [("semantic", C.c_void_p), ("instance", C.c_void_p), ("geo_1", C.c_void_p), ("geo_2", C.c_void_p),
                ("geo_4", C.c_void_p), ("sem_2", C.c_void_p), ("sem_4", C.c_void_p), ("min_C", C.c_int32 * 3),
                ("scene", C.c_int32 * 3)]


_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "resample_workspace_bytes": [_i32],
    "resample": [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp],
    "crop_bounds": [_vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp],
    "labels": [_vp, _vp, _i64, _vp, _i32, _vp, C.POINTER(SubnetOut), _i32, _vp, _vp],
    "presence": [_vp, _vp, _i64, _vp, _vp],
    "masks": [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp],
    "target_pack": [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "resample_workspace_bytes": _i64}


def _u8(t: torch.Tensor, what: str) -> int:
    assert t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous(), f"{what}: a contiguous uint8 device tensor"
    return t.data_ptr()


def _host_i32(t: torch.Tensor):
    flat = t.to(torch.int32).reshape(-1).tolist()
    return (C.c_int32 * len(flat))(*flat)


def _host_f64(t: Optional[torch.Tensor]):
    if t is None:
        return None
    flat = t.to(torch.float64).reshape(-1).tolist()
    return (C.c_double * len(flat))(*flat)


class TargetLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pt_", PT_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def resample(self, sem: torch.Tensor, ins: torch.Tensor, Ts: Sequence[torch.Tensor], Tinvs: Sequence[torch.Tensor],
                 box_bound: torch.Tensor, sem_box: torch.Tensor, ins_box: torch.Tensor, bounds: torch.Tensor):
        """sem / ins uint8 [X, Y, Z]; box_bound int32 [M, 6] (host); sem_box / ins_box uint8 [M, stride]; bounds int32
        [M, 18] - all but box_bound on the device."""
        assert sem.dim() == 3 and sem.shape == ins.shape and sem_box.shape == ins_box.shape and sem_box.shape[0] == len(Ts)
        assert bounds.is_cuda and bounds.dtype == torch.int32 and bounds.is_contiguous() and bounds.numel() == len(Ts) * BOUNDS
        M = len(Ts)
        ws = torch.empty(int(self.lib.pt_resample_workspace_bytes(M)), dtype=torch.uint8, device=sem.device)
        X, Y, Z = (int(v) for v in sem.shape)
        self._ok(self.lib.pt_resample(_u8(sem, "sem"), _u8(ins, "ins"), X, Y, Z, _mats(Ts), _mats(Tinvs), M, _host_i32(box_bound),
                                      _u8(sem_box, "sem_box"), _u8(ins_box, "ins_box"), int(sem_box.shape[1]),
                                      bounds.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(sem)), "resample")

    def crop_bounds(self, sem_box, ins_box, box_bound, windows: torch.Tensor, out: torch.Tensor):
        """windows fp64 [M, 4] (host) -> out int32 [M, 12] on the device."""
        M = int(sem_box.shape[0])
        assert out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and out.numel() == M * CROP_BOUNDS
        self._ok(self.lib.pt_crop_bounds(_u8(sem_box, "sem_box"), _u8(ins_box, "ins_box"), int(sem_box.shape[1]),
                                         _host_i32(box_bound), M, _host_f64(windows), out.data_ptr(), self._stream(sem_box)),
                 "crop_bounds")

    def labels(self, sem_box, ins_box, box_bound, windows: Optional[torch.Tensor], outs: Sequence[dict], n_classes: int,
               table: torch.Tensor):
        """outs: per subnet {"semantic", "instance", "geo_1", "geo_2", "geo_4", "sem_2", "sem_4": uint8 device tensors,
        "min_C", "scene": three ints each}; table int32 [M, 768] on the device."""
        M = int(sem_box.shape[0])
        assert len(outs) == M and table.is_cuda and table.dtype == torch.int32 and table.is_contiguous()
        assert table.numel() >= M * TABLE
        arr = (SubnetOut * M)()
        for m, o in enumerate(outs):
            sx, sy, sz = (int(v) for v in o["scene"])
            assert tuple(o["semantic"].shape) == (sx, sy, sz) == tuple(o["instance"].shape) == tuple(o["geo_1"].shape)
            for s in (2, 4):
                assert tuple(o[f"geo_{s}"].shape) == (sx // s, sy // s, sz // s) == tuple(o[f"sem_{s}"].shape)
            for k in ("semantic", "instance", "geo_1", "geo_2", "geo_4", "sem_2", "sem_4"):
                setattr(arr[m], k, _u8(o[k], k))
            arr[m].min_C[:] = [int(v) for v in o["min_C"]]
            arr[m].scene[:] = [sx, sy, sz]
        self._ok(self.lib.pt_labels(_u8(sem_box, "sem_box"), _u8(ins_box, "ins_box"), int(sem_box.shape[1]), _host_i32(box_bound),
                                    M, _host_f64(windows), arr, int(n_classes), table.data_ptr(), self._stream(sem_box)), "labels")

    def presence(self, semantic: torch.Tensor, instance: torch.Tensor, table: torch.Tensor):
        """The presence table int32 [768] of a pair of uint8 grids of one shape."""
        assert semantic.shape == instance.shape and table.is_cuda and table.dtype == torch.int32 and table.is_contiguous()
        assert table.numel() == TABLE
        self._ok(self.lib.pt_presence(_u8(semantic, "semantic"), _u8(instance, "instance"), semantic.numel(), table.data_ptr(),
                                      self._stream(semantic)), "presence")

    def masks(self, semantic: torch.Tensor, instance: torch.Tensor, cls_slot: torch.Tensor, ins_slot: torch.Tensor, t: int):
        """-> bool [t, *semantic.shape]; cls_slot / ins_slot int32 [256] on the device."""
        assert semantic.shape == instance.shape
        for s in (cls_slot, ins_slot):
            assert s.is_cuda and s.dtype == torch.int32 and s.is_contiguous() and s.numel() == 256
        out = torch.empty((t,) + tuple(semantic.shape), dtype=torch.bool, device=semantic.device)
        self._ok(self.lib.pt_masks(_u8(semantic, "semantic"), _u8(instance, "instance"), semantic.numel(), cls_slot.data_ptr(),
                                   ins_slot.data_ptr(), int(t), out.data_ptr(), self._stream(semantic)), "masks")
        return out

    def target_pack(self, semantic, instance, cls_slot, ins_slot, unknown, coords, t: int, origin=(0, 0, 0)):
        """-> (tbits int32 [N, 4], flags uint8 [N], oob int32 [1]) as `MatchLib.target_pack`, read off the two label grids."""
        dx, dy, dz = (int(v) for v in semantic.shape)
        assert semantic.shape == instance.shape and coords.dim() == 2 and coords.shape[1] == 4
        assert coords.is_cuda and coords.dtype == torch.int32 and coords.is_contiguous()
        assert unknown is None or tuple(unknown.shape) == (dx, dy, dz), "unknown: [X, Y, Z]"
        n, dev = int(coords.shape[0]), coords.device
        tbits = torch.empty((n, 4), dtype=torch.int32, device=dev)
        flags = torch.empty((n,), dtype=torch.uint8, device=dev)
        oob = torch.empty((1,), dtype=torch.int32, device=dev)
        self._ok(self.lib.pt_target_pack(_u8(semantic, "semantic"), _u8(instance, "instance"), cls_slot.data_ptr(),
                                         ins_slot.data_ptr(), None if unknown is None else _u8(unknown, "unknown"),
                                         coords.data_ptr(), n, int(t), dx, dy, dz, int(origin[0]), int(origin[1]), int(origin[2]),
                                         tbits.data_ptr(), flags.data_ptr(), oob.data_ptr(), self._stream(coords)), "target_pack")
        return tbits, flags, oob


def target_lib() -> TargetLib:
    """The process-wide binding of libpascohip.so's target kernels (a missing library is an error)."""
    return shared(TargetLib)
