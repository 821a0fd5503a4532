"""ctypes binding of include/pasco_match.h (the `pm_*` entry points of libpascohip.so): the targets as 128-bit words per voxel,
the per-pair sums of the matcher and the mask losses, the gradient of the losses, and the assignment on the host.

Kept apart from `me.backend` like `grad.attnlib`.  Every device method takes device tensors and enqueues on the caller's current
stream; nothing synchronises.  The scratch of `pair_sums` is a buffer of the product backend's per-stream scratch table
(`hip_backend().scratch`, "pair_sums"): reused from call to call in stream order and dropped by `release_stream`.  `assign` takes a CPU tensor: it is
the one host entry point."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PM_ABI_VERSION = 1       # include/pasco_match.h PM_ABI_VERSION this binding was written against
PM_MAX_Q = 128
PM_MAX_T = 128
FLAG_KNOWN, FLAG_MATCHABLE = 1, 2
BIT_KNOWN, BIT_MATCHABLE = 0, 1

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "target_pack": [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp],
    "pair_sums_ranges": [_i64, _i32, _i32],
    "pair_sums_workspace_bytes": [_i64, _i32, _i32],
    "pair_sums": [_vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "mask_loss_bwd": [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp],
    "assign": [_vp, _i32, _i32, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "pair_sums_ranges": _i64, "pair_sums_workspace_bytes": _i64}

MIN_RANGE_ROWS = 128
MAX_RANGES = 256


def geometry(n: int, q: int, t: int) -> dict:
    """The launch geometry of pm_pair_sums, restated from csrc/match.hip: `range_rows` rows per range (a multiple of 32, at
    least 128, so that there are at most 256 ranges), `ranges` of them, `floats` per range's partials, `workspace_bytes`."""
    if not (n >= 0 and 1 <= q <= PM_MAX_Q and 1 <= t <= PM_MAX_T):
        return {"range_rows": 0, "ranges": 0, "floats": 0, "workspace_bytes": 0}
    rr = max(MIN_RANGE_ROWS, -(-(-(-n // MAX_RANGES)) // 32) * 32)
    ranges = -(-n // rr)
    qp, tp = -(-q // 32) * 32, -(-t // 32) * 32
    floats = 2 * qp * tp + 2 * qp + tp + 4
    return {"range_rows": rr, "ranges": ranges, "floats": floats, "workspace_bytes": 4 * floats * ranges}


def check_counts(q: int, t: int):
    if not (1 <= q <= PM_MAX_Q and 1 <= t <= PM_MAX_T):
        raise ValueError(f"panoptic match: {q} queries and {t} targets not served (1..{PM_MAX_Q} queries, 1..{PM_MAX_T} targets)")


class MatchLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pm_", PM_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def workspace_bytes(self, n: int, q: int, t: int) -> int:
        return int(self.lib.pm_pair_sums_workspace_bytes(int(n), int(q), int(t)))

    def ranges(self, n: int, q: int, t: int) -> int:
        return int(self.lib.pm_pair_sums_ranges(int(n), int(q), int(t)))

    def _workspace(self, need: int, device: torch.device) -> torch.Tensor:
        from ..me.backend import hip_backend
        return hip_backend().scratch.bytes("pair_sums", device, need, floor=4)

    def target_pack(self, masks, unknown, coords, origin=(0, 0, 0)):
        """masks uint8 [T,X,Y,Z], unknown uint8 [X,Y,Z] | None, coords int32 [N,4] -> (tbits int32 [N,4], flags uint8 [N],
        oob int32 [1]).  Nothing is read back: the caller looks at `oob` when it synchronises anyway."""
        t, dx, dy, dz = (int(x) for x in masks.shape)
        n = int(coords.shape[0])
        check_counts(1, t)
        assert coords.dim() == 2 and coords.shape[1] == 4, "coords: [N, 4]"
        assert unknown is None or tuple(unknown.shape) == (dx, dy, dz), "unknown: [X, Y, Z]"
        dev = coords.device
        tbits = torch.empty((n, 4), dtype=torch.int32, device=dev)
        flags = torch.empty((n,), dtype=torch.uint8, device=dev)
        oob = torch.empty((1,), dtype=torch.int32, device=dev)
        u8, i32 = torch.uint8, torch.int32
        self._ok(self.lib.pm_target_pack(_dev(masks, u8, "masks"), None if unknown is None else _dev(unknown, u8, "unknown"),
                                         _dev(coords, i32, "coords"), n, t, dx, dy, dz, int(origin[0]), int(origin[1]),
                                         int(origin[2]), tbits.data_ptr(), flags.data_ptr(), oob.data_ptr(),
                                         self._stream(coords)), "target_pack")
        return tbits, flags, oob

    def pair_sums(self, logits, tbits, flags, flag_bit: int, t: int):
        """logits fp32 [N,Q], tbits int32 [N,4], flags uint8 [N] -> (focal_sum [Q,T], dice [Q,T], stats [Q,T,3], count int32 [1])."""
        n, q = (int(x) for x in logits.shape)
        check_counts(q, t)
        assert tuple(tbits.shape) == (n, 4) and tuple(flags.shape) == (n,)
        dev = logits.device
        focal_sum = torch.empty((q, t), dtype=torch.float32, device=dev)
        dice = torch.empty((q, t), dtype=torch.float32, device=dev)
        stats = torch.empty((q, t, 3), dtype=torch.float32, device=dev)
        count = torch.empty((1,), dtype=torch.int32, device=dev)
        need = self.workspace_bytes(n, q, t)
        ws = self._workspace(need, dev)
        f32 = torch.float32
        self._ok(self.lib.pm_pair_sums(_dev(logits, f32, "logits"), _dev(tbits, torch.int32, "tbits"),
                                       _dev(flags, torch.uint8, "flags"), int(flag_bit), n, q, int(t), focal_sum.data_ptr(),
                                       dice.data_ptr(), stats.data_ptr(), count.data_ptr(), ws.data_ptr(), ws.numel(),
                                       self._stream(logits)), "pair_sums")
        return focal_sum, dice, stats, count

    def mask_loss_bwd(self, logits, tbits, flags, tgt_of_query, coef, t: int):
        """-> dlogits fp32 [N,Q].  tgt_of_query int32 [Q], coef fp32 [Q,3]."""
        n, q = (int(x) for x in logits.shape)
        check_counts(q, t)
        assert tuple(tgt_of_query.shape) == (q,) and tuple(coef.shape) == (q, 3)
        dlogits = torch.empty_like(logits)
        f32 = torch.float32
        self._ok(self.lib.pm_mask_loss_bwd(_dev(logits, f32, "logits"), _dev(tbits, torch.int32, "tbits"),
                                           _dev(flags, torch.uint8, "flags"), _dev(tgt_of_query, torch.int32, "tgt_of_query"),
                                           _dev(coef, f32, "coef"), n, q, int(t), dlogits.data_ptr(), self._stream(logits)),
                 "mask_loss_bwd")
        return dlogits

    def assign(self, cost: torch.Tensor):
        """cost [Q,T] on the CPU (any float dtype) -> (row int64 [K], col int64 [K]), K = min(Q, T), rows ascending."""
        assert not cost.is_cuda and cost.dim() == 2, "assign: a CPU matrix"
        c = cost.detach().to(torch.float64).contiguous()
        q, t = (int(x) for x in c.shape)
        k = min(q, t)
        row = torch.empty((k,), dtype=torch.int32)
        col = torch.empty((k,), dtype=torch.int32)
        self._ok(self.lib.pm_assign(c.data_ptr(), q, t, row.data_ptr(), col.data_ptr()), "assign")
        return row.to(torch.int64), col.to(torch.int64)


def match_lib() -> MatchLib:
    """The process-wide binding of libpascohip.so's matcher and mask-loss kernels (a missing library is an error)."""
    return shared(MatchLib)
