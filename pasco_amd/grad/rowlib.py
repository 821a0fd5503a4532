"""ctypes binding of include/pasco_rowgrad.h (the `pr_*` entry points of libpascohip.so): the adjoints of `SparseTensor.dense()`
and `to_sparse()` and the backward of local max pooling.

Kept apart from `me.backend` like `grad.lib`: the CPU oracle binds `me.backend._SIGNATURES` and has no gradient kernels.  Every
method takes device tensors and enqueues on the caller's current stream; nothing synchronises."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PR_ABI_VERSION = 1       # include/pasco_rowgrad.h PR_ABI_VERSION this binding was written against
PR_MAX_KVOL = 64

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "dense_rows": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp],
    "rows_dense": [_vp, _i64, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "maxpool_arg": [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _vp, _vp],
    "maxpool_bwd": [_vp, _i64, _i32, _vp, _vp, _i32, _i64, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p}


class RowGradLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pr_", PR_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def dense_rows(self, dense: torch.Tensor, coords: torch.Tensor, min3, ts: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dense fp32 [B, C, X, Y, Z], coords int32 [n, 4] -> rows fp32 [n, C] (overwritten): the adjoint of `to_dense`."""
        B, c, X, Y, Z = (int(v) for v in dense.shape)
        n = int(coords.shape[0])
        assert tuple(coords.shape) == (n, 4)
        out = torch.empty((n, c), dtype=torch.float32, device=dense.device) if out is None else out
        assert tuple(out.shape) == (n, c)
        mx, my, mz = (int(v) for v in min3)
        self._ok(self.lib.pr_dense_rows(_dev(dense, torch.float32, "dense"), c, B, X, Y, Z, _dev(coords, torch.int32, "coords"),
                                        n, mx, my, mz, int(ts), _dev(out, torch.float32, "rows"), self._stream(dense)),
                 "dense_rows")
        return out

    def rows_dense(self, rows: torch.Tensor, site_coords: torch.Tensor, shape5, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """rows fp32 [n, C], site_coords int32 [n, 4] (distinct sites) -> dense fp32 `shape5` (overwritten): the adjoint of
        `dense_gather`."""
        B, c, X, Y, Z = (int(v) for v in shape5)
        n = int(rows.shape[0])
        assert tuple(rows.shape) == (n, c) and tuple(site_coords.shape) == (n, 4)
        out = torch.empty((B, c, X, Y, Z), dtype=torch.float32, device=rows.device) if out is None else out
        assert tuple(out.shape) == (B, c, X, Y, Z)
        self._ok(self.lib.pr_rows_dense(_dev(rows, torch.float32, "rows"), n, c, _dev(site_coords, torch.int32, "site_coords"),
                                        B, X, Y, Z, _dev(out, torch.float32, "dense"), self._stream(rows)), "rows_dense")
        return out

    def maxpool_arg(self, x: torch.Tensor, nbr: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """x fp32 [n_in, C], nbr int32 [K, n_out], out fp32 [n_out, C] = maxpool_fwd(x, nbr) -> arg int32 [n_out, C]."""
        (n_in, c), (K, n_out) = (int(v) for v in x.shape), (int(v) for v in nbr.shape)
        assert tuple(out.shape) == (n_out, c)
        arg = torch.empty((n_out, c), dtype=torch.int32, device=x.device)
        self._ok(self.lib.pr_maxpool_arg(_dev(x, torch.float32, "in"), n_in, c, _dev(nbr, torch.int32, "nbr"), K, n_out,
                                         _dev(out, torch.float32, "out"), _dev(arg, torch.int32, "arg"), self._stream(x)),
                 "maxpool_arg")
        return arg

    def maxpool_bwd(self, dy: torch.Tensor, arg: torch.Tensor, inv: torch.Tensor, n_in: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dy fp32 [n_out, C], arg int32 [n_out, C], inv int32 [K, n_in] -> dx fp32 [n_in, C] (overwritten)."""
        (n_out, c), K, n_in = (int(v) for v in dy.shape), int(inv.shape[0]), int(n_in)
        assert tuple(arg.shape) == (n_out, c) and tuple(inv.shape) == (K, n_in)
        out = torch.empty((n_in, c), dtype=torch.float32, device=dy.device) if out is None else out
        assert tuple(out.shape) == (n_in, c)
        self._ok(self.lib.pr_maxpool_bwd(_dev(dy, torch.float32, "dy"), n_out, c, _dev(arg, torch.int32, "arg"),
                                         _dev(inv, torch.int32, "inv"), K, n_in, _dev(out, torch.float32, "dx"),
                                         self._stream(dy)), "maxpool_bwd")
        return out


def rowgrad_lib() -> RowGradLib:
    """The process-wide binding of libpascohip.so's dense / pooling gradient kernels (a missing library is an error)."""
    return shared(RowGradLib)
