"""ctypes binding of include/pasco_eval.h (the `pe_*` entry points of libpascohip.so).

Kept apart from `me.backend` on purpose: the CPU oracle binds `me.backend._SIGNATURES` too and has no evaluation kernels."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, shared

PE_ABI_VERSION = 1       # include/pasco_eval.h PE_ABI_VERSION this binding was written against
BINS = 16
MAX_CLASSES = 32
MAX_PRED = 128
MAX_GT = 1023
MAX_SITES = 1 << 27


def ssc_counts(c: int) -> int:
    return c * c + 1 + 4 * BINS


SSC_SUMS = 2 * BINS + 2
ECE_COUNTS = 2 * BINS
ECE_SUMS = BINS

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "ssc_workspace_bytes": [_i64, _i32],
    "ece_workspace_bytes": [_i64],
    "ssc": [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _vp],
    "panop_pairs": [_vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp],
    "match": [_vp, _vp, _vp, _i32, _i32, _vp, _vp],
    "mask_ece": [_vp, _vp, _vp, _i64, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "ssc_workspace_bytes": _i64, "ece_workspace_bytes": _i64}


class EvalLib(FamilyLib):
    """The evaluation kernels on the caller's current stream.  Every method takes device tensors and returns nothing: the
    results land in the caller's output tensors (one buffer per scene, read back once)."""

    def __init__(self, path: Optional[str] = None):
        super().__init__("pe_", PE_ABI_VERSION, _SIGNATURES, _RESTYPES, path)
        self._edges = (C.c_float * BINS)(*torch.linspace(0, 1, BINS).tolist())

    def ssc_workspace_bytes(self, n_sites: int, c: int) -> int:
        return int(self.lib.pe_ssc_workspace_bytes(n_sites, c))

    def ece_workspace_bytes(self, n_rows: int) -> int:
        return int(self.lib.pe_ece_workspace_bytes(n_rows))

    def ssc(self, probs, conf, gt, ws, counts_ptr: int, sums_ptr: int):
        n, c = probs.shape
        assert probs.is_contiguous() and probs.dtype == torch.float32 and conf.dtype == torch.float32 and gt.dtype == torch.uint8
        assert conf.numel() == n and gt.numel() == n
        self._ok(self.lib.pe_ssc(probs.data_ptr(), conf.data_ptr(), gt.data_ptr(), n, c, self._edges, ws.data_ptr(),
                                 ws.numel() * ws.element_size(), counts_ptr, sums_ptr, self._stream(probs)), "ssc")

    def panop_pairs(self, site, pred, gt_sem, gt_id, n_pred: int, n_gt: int, area_ptr: int, inter_ptr: int):
        assert site.dtype == torch.int64 and pred.dtype == torch.int32 and site.numel() == pred.numel()
        self._ok(self.lib.pe_panop_pairs(site.data_ptr(), pred.data_ptr(), site.numel(), gt_sem.data_ptr(), gt_id.data_ptr(),
                                         gt_sem.numel(), n_pred, n_gt, area_ptr, inter_ptr, self._stream(gt_sem)),
                 "panop_pairs")

    def match(self, area_ptr: int, gt_area, inter_ptr: int, n_pred: int, n_gt: int, map_ptr: int):
        self._ok(self.lib.pe_match(area_ptr, gt_area.data_ptr(), inter_ptr, n_pred, n_gt, map_ptr, self._stream(gt_area)),
                 "match")

    def mask_ece(self, site, pred, conf, gt_id, map_ptr: int, n_pred: int, ws, counts_ptr: int, sums_ptr: int):
        assert conf.dtype == torch.float32 and conf.numel() == site.numel()
        self._ok(self.lib.pe_mask_ece(site.data_ptr(), pred.data_ptr(), conf.data_ptr(), site.numel(), gt_id.data_ptr(),
                                      gt_id.numel(), map_ptr, n_pred, self._edges, ws.data_ptr(),
                                      ws.numel() * ws.element_size(), counts_ptr, sums_ptr, self._stream(conf)), "mask_ece")


def eval_lib() -> EvalLib:
    """The process-wide binding of libpascohip.so's evaluation kernels (a missing library is an error)."""
    return shared(EvalLib)
