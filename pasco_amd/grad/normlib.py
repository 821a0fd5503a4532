"""ctypes binding of include/pasco_norm.h (the `pn_*` entry points of libpascohip.so): training-mode batch normalisation over
feature rows - moments records, their merge, the normalisation with its activation, and the backward.

Kept apart from `me.backend` like `grad.rowlib`.  Every method takes device tensors and enqueues on the caller's current stream;
nothing synchronises.  The autograd operator over it is `grad.norm.batch_norm_rows`."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PN_ABI_VERSION = 1       # include/pasco_norm.h PN_ABI_VERSION this binding was written against
PN_TILE_ROWS = 128       # rows of one partial record
PN_MAX_C = 1 << 20

_vp, _i64, _i32, _f32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_double
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "ws_bytes": [_i64, _i32],
    "moments": [_vp, _i64, _i32, _vp, _i64, _vp, _vp],
    "moments_merge": [_vp, _i32, _i32, _vp, _vp],
    "finish": [_vp, _i32, _f64, _f64, _vp, _vp, _vp, _vp],
    "apply": [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _f32, _vp, _vp],
    "bwd_sums": [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _f32, _vp, _i64, _vp, _vp],
    "sums_merge": [_vp, _i32, _i32, _vp, _vp],
    "bwd_dx": [_vp, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _f32, _vp, _vp, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "ws_bytes": C.c_int64}

_f4, _f8 = torch.float32, torch.float64


def _opt(t: Optional[torch.Tensor], c: int, what: str):
    """An optional fp32 [c] vector (weight, bias, running statistics): its pointer, or NULL."""
    if t is None:
        return None
    assert tuple(t.shape) == (c,), f"{what}: [{c}]"
    return _dev(t, _f4, what)


class NormLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pn_", PN_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def ws_bytes(self, n: int, c: int) -> int:
        b = int(self.lib.pn_ws_bytes(int(n), int(c)))
        if b < 0:
            raise RuntimeError(f"pn_ws_bytes: n = {n}, c = {c} outside the served range")
        return b

    def _ws(self, x: torch.Tensor):
        n, c = (int(v) for v in x.shape)
        nbytes = self.ws_bytes(n, c)
        return torch.empty(max(nbytes // 8, 1), dtype=_f8, device=x.device), nbytes

    def moments(self, x: torch.Tensor) -> torch.Tensor:
        """x fp32 [n, c] -> the moments record fp64 [3, c] = (count, mean, M2) of its rows."""
        n, c = (int(v) for v in x.shape)
        ws, nbytes = self._ws(x)
        rec = torch.empty((3, c), dtype=_f8, device=x.device)
        self._ok(self.lib.pn_moments(_dev(x, _f4, "x"), n, c, ws.data_ptr(), nbytes, rec.data_ptr(), self._stream(x)), "moments")
        return rec

    def moments_merge(self, recs: torch.Tensor) -> torch.Tensor:
        """recs fp64 [r, 3, c] -> fp64 [3, c]: merged in ascending r, records of count 0 skipped."""
        r, three, c = (int(v) for v in recs.shape)
        assert three == 3
        out = torch.empty((3, c), dtype=_f8, device=recs.device)
        self._ok(self.lib.pn_moments_merge(_dev(recs, _f8, "recs"), r, c, out.data_ptr(), self._stream(recs)), "moments_merge")
        return out

    def finish(self, rec: torch.Tensor, eps: float, momentum: float, running_mean: Optional[torch.Tensor],
               running_var: Optional[torch.Tensor]) -> torch.Tensor:
        """rec fp64 [3, c] -> mean_rstd fp32 [2, c]; the running statistics (fp32 [c] or None) are updated IN PLACE."""
        c = int(rec.shape[1])
        assert tuple(rec.shape) == (3, c)
        out = torch.empty((2, c), dtype=_f4, device=rec.device)
        self._ok(self.lib.pn_finish(_dev(rec, _f8, "rec"), c, float(eps), float(momentum), _opt(running_mean, c, "running_mean"),
                                    _opt(running_var, c, "running_var"), out.data_ptr(), self._stream(rec)), "finish")
        return out

    def apply(self, x: torch.Tensor, mean_rstd: torch.Tensor, weight, bias, act: int, slope: float) -> torch.Tensor:
        """y fp32 [n, c] = act(((x - mean) * rstd) * weight + bias)."""
        n, c = (int(v) for v in x.shape)
        assert tuple(mean_rstd.shape) == (2, c)
        y = torch.empty_like(x)
        self._ok(self.lib.pn_apply(_dev(x, _f4, "x"), n, c, _dev(mean_rstd, _f4, "mean_rstd"), _opt(weight, c, "weight"),
                                   _opt(bias, c, "bias"), int(act), float(slope), y.data_ptr(), self._stream(x)), "apply")
        return y

    def bwd_sums(self, dy: torch.Tensor, x: torch.Tensor, mean_rstd: torch.Tensor, weight, bias, act: int,
                 slope: float) -> torch.Tensor:
        """-> the sums record fp64 [2, c] = (sum g, sum g * xhat) over the rows."""
        n, c = (int(v) for v in x.shape)
        assert tuple(dy.shape) == (n, c) and tuple(mean_rstd.shape) == (2, c)
        ws, nbytes = self._ws(x)
        sums = torch.empty((2, c), dtype=_f8, device=x.device)
        self._ok(self.lib.pn_bwd_sums(_dev(dy, _f4, "dy"), _dev(x, _f4, "x"), n, c, _dev(mean_rstd, _f4, "mean_rstd"),
                                      _opt(weight, c, "weight"), _opt(bias, c, "bias"), int(act), float(slope), ws.data_ptr(),
                                      nbytes, sums.data_ptr(), self._stream(x)), "bwd_sums")
        return sums

    def sums_merge(self, sums: torch.Tensor) -> torch.Tensor:
        """sums fp64 [r, 2, c] -> fp64 [2, c]: added in ascending r."""
        r, two, c = (int(v) for v in sums.shape)
        assert two == 2
        out = torch.empty((2, c), dtype=_f8, device=sums.device)
        self._ok(self.lib.pn_sums_merge(_dev(sums, _f8, "sums"), r, c, out.data_ptr(), self._stream(sums)), "sums_merge")
        return out

    def bwd_dx(self, dy: torch.Tensor, x: torch.Tensor, mean_rstd: torch.Tensor, weight, bias, act: int, slope: float,
               total_sums: torch.Tensor, total_rec: torch.Tensor) -> torch.Tensor:
        """-> dx fp32 [n, c]; the count N is read from `total_rec` on the device."""
        n, c = (int(v) for v in x.shape)
        assert tuple(dy.shape) == (n, c) and tuple(total_sums.shape) == (2, c) and tuple(total_rec.shape) == (3, c)
        dx = torch.empty_like(x)
        self._ok(self.lib.pn_bwd_dx(_dev(dy, _f4, "dy"), _dev(x, _f4, "x"), n, c, _dev(mean_rstd, _f4, "mean_rstd"),
                                    _opt(weight, c, "weight"), _opt(bias, c, "bias"), int(act), float(slope),
                                    _dev(total_sums, _f8, "total_sums"), _dev(total_rec, _f8, "total_rec"), dx.data_ptr(),
                                    self._stream(x)), "bwd_dx")
        return dx


def norm_lib() -> NormLib:
    """The process-wide binding of libpascohip.so's batch-normalisation kernels (a missing library is an error)."""
    return shared(NormLib)
