"""ctypes binding of include/pasco_label.h (the `pl_*` entry points of libpascohip.so): label generation on the device.

Kept apart from `me.backend` like `data.frame_lib`: the CPU oracle binds `me.backend._SIGNATURES` and has no label kernels.
Every method takes device tensors and enqueues on the caller's current stream; nothing synchronises."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .._clib import FamilyLib, shared

PL_ABI_VERSION = 1       # include/pasco_label.h PL_ABI_VERSION this binding was written against
MAX_THINGS = 32
RECORD = 4
REC_INSTANCES, REC_DROPPED, REC_UNKNOWN, REC_STATUS = 0, 1, 2, 3
STATUS_RAW_RANGE, STATUS_LOOP_CAP = 1, 2

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "semantic_grid": [_vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp],
    "instances_workspace_bytes": [_i32, _i32, _i32, _i32],
    "instances": [_vp, _i32, _i32, _i32, C.POINTER(_i32), _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "instances_workspace_bytes": _i64}


class LabelLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pl_", PL_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def semantic_grid(self, raw: torch.Tensor, invalid: torch.Tensor, lut: torch.Tensor,
                      status: Optional[torch.Tensor] = None):
        """raw uint16 [S] (or int16 holding the same bits), invalid uint8 [S / 8], lut uint8 [n] on the device ->
        (sem uint8 [S], status int32 [1]); a non-zero status means a raw label outside the table (see pasco_label.h)."""
        assert raw.is_cuda and raw.dtype in (torch.uint16, torch.int16) and raw.is_contiguous() and raw.dim() == 1
        assert invalid.is_cuda and invalid.dtype == torch.uint8 and invalid.is_contiguous()
        assert lut.is_cuda and lut.dtype == torch.uint8 and lut.is_contiguous()
        S = int(raw.numel())
        if invalid.numel() * 8 != S:
            raise ValueError(f"pl_semantic_grid: {S} labels but {invalid.numel()} bytes of invalid bits")
        sem = torch.empty(S, dtype=torch.uint8, device=raw.device)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=raw.device)
        self.semantic_grid_into(raw, invalid, lut, sem, status)
        return sem, status

    def semantic_grid_into(self, raw: torch.Tensor, invalid: torch.Tensor, lut: torch.Tensor, sem: torch.Tensor,
                           status: torch.Tensor):
        """`semantic_grid` into the caller's `sem` uint8 [S] and `status` int32 [1] (zeroed by the caller); any alignment."""
        assert sem.is_cuda and sem.dtype == torch.uint8 and sem.is_contiguous() and sem.numel() == raw.numel()
        assert status.is_cuda and status.dtype == torch.int32
        self._ok(self.lib.pl_semantic_grid(raw.data_ptr(), invalid.data_ptr(), lut.data_ptr(), int(lut.numel()),
                                           int(raw.numel()), sem.data_ptr(), status.data_ptr(), self._stream(raw)),
                 "semantic_grid")

    def workspace_bytes(self, shape: Sequence[int], n_things: int) -> int:
        X, Y, Z = (int(v) for v in shape)
        n = int(self.lib.pl_instances_workspace_bytes(X, Y, Z, int(n_things)))
        if n < 0:
            raise ValueError(f"pl_instances: grid {X} x {Y} x {Z} with {n_things} thing ids is not supported")
        return n

    def instances(self, sem: torch.Tensor, thing_ids: Sequence[int], min_size: int = 8, sizes_cap: int = 0,
                  ws: Optional[torch.Tensor] = None):
        """sem uint8 [X, Y, Z] on the device -> (instance int32 [X, Y, Z], semantic uint8 [X, Y, Z], record int32 [4],
        sizes int32 [sizes_cap] or None), all on the device."""
        assert sem.is_cuda and sem.dtype == torch.uint8 and sem.is_contiguous() and sem.dim() == 3
        ids = [int(t) for t in thing_ids]
        need = self.workspace_bytes(sem.shape, len(ids))
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=sem.device)
        assert ws.is_cuda and ws.dtype == torch.uint8 and ws.is_contiguous()
        ins = torch.empty(sem.shape, dtype=torch.int32, device=sem.device)
        out = torch.empty_like(sem)
        rec = torch.empty(RECORD, dtype=torch.int32, device=sem.device)
        sizes = torch.zeros(sizes_cap, dtype=torch.int32, device=sem.device) if sizes_cap > 0 else None
        self.instances_into(sem, ids, min_size, ins, out, rec, sizes, sizes_cap, ws)
        return ins, out, rec, sizes

    def instances_into(self, sem: torch.Tensor, thing_ids: Sequence[int], min_size: int, instance: torch.Tensor,
                       semantic_out: torch.Tensor, record: torch.Tensor, sizes: Optional[torch.Tensor], sizes_cap: int,
                       ws: torch.Tensor):
        """`instances` into the caller's tensors (any alignment but the workspace's 16 bytes): instance int32 [X, Y, Z],
        semantic_out uint8 [X, Y, Z], record int32 [4], sizes int32 [>= sizes_cap] or None."""
        ids = [int(t) for t in thing_ids]
        assert instance.is_cuda and instance.dtype == torch.int32 and instance.is_contiguous() and instance.shape == sem.shape
        assert semantic_out.is_cuda and semantic_out.dtype == torch.uint8 and semantic_out.is_contiguous()
        assert semantic_out.shape == sem.shape and record.dtype == torch.int32 and record.numel() >= RECORD
        assert sizes is None or (sizes.dtype == torch.int32 and sizes.numel() >= sizes_cap)
        X, Y, Z = (int(v) for v in sem.shape)
        self._ok(self.lib.pl_instances(sem.data_ptr(), X, Y, Z, (_i32 * max(len(ids), 1))(*ids), len(ids), int(min_size),
                                       instance.data_ptr(), semantic_out.data_ptr(), record.data_ptr(),
                                       None if sizes is None else sizes.data_ptr(), int(sizes_cap), ws.data_ptr(),
                                       ws.numel(), self._stream(sem)), "instances")


def label_lib() -> LabelLib:
    """The process-wide binding of libpascohip.so's label kernels (a missing library is an error)."""
    return shared(LabelLib)
