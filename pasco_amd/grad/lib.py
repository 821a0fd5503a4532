"""ctypes binding of include/pasco_grad.h (the `pg_*` entry points of libpascohip.so): the training kernels of the sparse
convolution family.

Kept apart from `me.backend` like `waffle.lib`: the CPU oracle binds `me.backend._SIGNATURES` and has no gradient kernels.
Every method takes device tensors and enqueues on the caller's current stream; nothing synchronises.  Workspaces are torch
allocations of the call (the caching allocator keeps them alive until the stream has passed the launch)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PG_ABI_VERSION = 1       # include/pasco_grad.h PG_ABI_VERSION this binding was written against
PG_MAX_KVOL = 64

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "nbr_invert": [_vp, _i32, _i64, _i64, _vp, _vp],
    "wgrad_slab_rows": [_i32, _i32, _i32, _i64],
    "wgrad_workspace_bytes": [_i32, _i32, _i32, _i64],
    "conv_wgrad": [_vp, _i64, _i32, _vp, _i64, _i32, _vp, _i32, _vp, _vp, _i64, _vp],
    "colsum_workspace_bytes": [_i64, _i32],
    "colsum": [_vp, _i64, _i32, _vp, _vp, _i64, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "wgrad_slab_rows": _i64, "wgrad_workspace_bytes": _i64, "colsum_workspace_bytes": _i64}


class GradLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pg_", PG_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def nbr_invert(self, nbr: torch.Tensor, n_in: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """nbr int32 [K, n_out] -> inv int32 [K, n_in] (include/pasco_grad.h states the precondition on the table)."""
        K, n_out = (int(v) for v in nbr.shape)
        n_in = int(n_in)
        out = torch.empty((K, n_in), dtype=torch.int32, device=nbr.device) if out is None else out
        assert tuple(out.shape) == (K, n_in)
        self._ok(self.lib.pg_nbr_invert(_dev(nbr, torch.int32, "nbr"), K, n_out, n_in, _dev(out, torch.int32, "inv"),
                                        self._stream(nbr)), "nbr_invert")
        return out

    def wgrad_slab_rows(self, K: int, cin: int, cout: int, n_out: int) -> int:
        """Output rows per slab of `conv_wgrad` at this shape."""
        return int(self.lib.pg_wgrad_slab_rows(int(K), int(cin), int(cout), int(n_out)))

    def wgrad_workspace_bytes(self, K: int, cin: int, cout: int, n_out: int) -> int:
        return int(self.lib.pg_wgrad_workspace_bytes(int(K), int(cin), int(cout), int(n_out)))

    def conv_wgrad(self, x: torch.Tensor, dy: torch.Tensor, nbr: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x fp32 [n_in, cin], dy fp32 [n_out, cout], nbr int32 [K, n_out] -> dw fp32 [K, cin, cout] (overwritten)."""
        (n_in, cin), (n_out, cout), K = (int(v) for v in x.shape), (int(v) for v in dy.shape), int(nbr.shape[0])
        assert tuple(nbr.shape) == (K, n_out), f"nbr {tuple(nbr.shape)} != {(K, n_out)}"
        out = torch.empty((K, cin, cout), dtype=torch.float32, device=x.device) if out is None else out
        assert tuple(out.shape) == (K, cin, cout)
        need = self.wgrad_workspace_bytes(K, cin, cout, n_out)
        if need < 0:
            raise ValueError(f"conv_wgrad: K = {K}, cin = {cin}, cout = {cout}, n_out = {n_out} is outside the served range")
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=x.device)
        self._ok(self.lib.pg_conv_wgrad(_dev(x, torch.float32, "x"), n_in, cin, _dev(dy, torch.float32, "dy"), n_out, cout,
                                        _dev(nbr, torch.int32, "nbr"), K, _dev(out, torch.float32, "dw"), ws.data_ptr(),
                                        ws.numel(), self._stream(x)), "conv_wgrad")
        return out

    def colsum(self, dy: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """dy fp32 [n, c] -> fp32 [c]."""
        n, c = (int(v) for v in dy.shape)
        out = torch.empty(c, dtype=torch.float32, device=dy.device) if out is None else out
        assert out.numel() == c
        need = int(self.lib.pg_colsum_workspace_bytes(n, c))
        if need < 0:
            raise ValueError(f"colsum: n = {n}, c = {c} is outside the served range")
        ws = torch.empty(max(need, 4), dtype=torch.uint8, device=dy.device)
        self._ok(self.lib.pg_colsum(_dev(dy, torch.float32, "dy"), n, c, _dev(out, torch.float32, "out"), ws.data_ptr(),
                                    ws.numel(), self._stream(dy)), "colsum")
        return out


def grad_lib() -> GradLib:
    """The process-wide binding of libpascohip.so's gradient kernels (a missing library is an error)."""
    return shared(GradLib)
