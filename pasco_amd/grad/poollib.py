"""ctypes binding of include/pasco_pool.h (the `pp_*` entry points of libpascohip.so): per-batch reductions, broadcast, local
sum / average pooling and the channel-wise convolution, each with its backward.

Kept apart from `me.backend` like `grad.rowlib`: the CPU oracle binds `me.backend._SIGNATURES` and has none of these kernels
(`pasco_amd.grad.host` restates them).  Every method takes device tensors and enqueues on the caller's current stream; nothing
synchronises.  The workspaces are buffers of the product backend's per-stream scratch table (`hip_backend().scratch`, "pool"),
reused from call to call in stream order."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PP_ABI_VERSION = 1       # include/pasco_pool.h PP_ABI_VERSION this binding was written against
PP_MAX_KVOL = 64
PP_MAX_BATCH = 64
PP_SEG_ROWS = 256
SUM, AVG, MAX = 0, 1, 2
BC_ADD, BC_MUL, BC_CAT, BC_COPY = 0, 1, 2, 3

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "seg_workspace_bytes": [_i64, _i32, _i32],
    "seg_reduce": [_vp, _i64, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _vp],
    "seg_max_bwd": [_vp, _vp, _i32, _i32, _i64, _vp, _vp],
    "broadcast": [_vp, _i64, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp],
    "broadcast_mul_bwd": [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _vp],
    "pool": [_vp, _i64, _i32, _vp, _i32, _i64, _i32, _vp, _vp, _vp],
    "pool_bwd": [_vp, _i64, _i32, _vp, _vp, _i32, _i64, _i32, _vp, _vp],
    "chconv_fwd": [_vp, _i64, _i32, _vp, _i32, _i64, _vp, _vp, _vp, _vp],
    "chconv_wgrad_workspace_bytes": [_i32, _i32, _i64],
    "chconv_wgrad": [_vp, _i64, _i32, _vp, _i64, _vp, _i32, _vp, _vp, _i64, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "seg_workspace_bytes": _i64, "chconv_wgrad_workspace_bytes": _i64}


def _f32(t: Optional[torch.Tensor], what: str) -> Optional[int]:
    """The address of a fp32 row matrix that may start anywhere on a 4-byte boundary (a view into a larger buffer)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: the pp_* kernels serve fp32 rows, got {t.dtype}")
    return _dev(t, torch.float32, what)


class PoolLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pp_", PP_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    @staticmethod
    def _scratch(device, need: int) -> torch.Tensor:
        from ..me.backend import hip_backend
        return hip_backend().scratch.bytes("pool", device, max(int(need), 16))

    def seg_workspace_bytes(self, n: int, c: int, B: int) -> int:
        return int(self.lib.pp_seg_workspace_bytes(int(n), int(c), int(B)))

    def _seg_ws(self, what: str, n: int, c: int, B: int, device) -> torch.Tensor:
        if not 1 <= B <= PP_MAX_BATCH:
            raise ValueError(f"{what}: {B} batch indices, at most {PP_MAX_BATCH} (PP_MAX_BATCH) are served")
        need = self.seg_workspace_bytes(n, c, B)
        if need < 0:
            raise ValueError(f"{what}: n = {n}, c = {c}, B = {B} is outside the served range (n < 2^24)")
        return self._scratch(device, need)

    def seg_reduce(self, x: torch.Tensor, coords: torch.Tensor, B: int, mode: int):
        """x fp32 [n, c] (a column slice of a contiguous matrix is taken as it is), coords int32 [n, 4] ->
        (out fp32 [B, c], count fp32 [B], arg int32 [B, c] | None)."""
        n, c = (int(v) for v in x.shape)
        B = int(B)
        assert tuple(coords.shape) == (n, 4)
        if x.dtype != torch.float32:
            raise TypeError(f"seg_reduce: the pp_* kernels serve fp32 rows, got {x.dtype}")
        if n and (x.stride(1) != 1 or x.stride(0) < c):
            x = x.contiguous()
        ldx = int(x.stride(0)) if n > 1 else c
        assert x.is_cuda
        ws = self._seg_ws("seg_reduce", n, c, B, x.device)
        out = torch.empty((B, c), dtype=torch.float32, device=x.device)
        count = torch.empty(B, dtype=torch.float32, device=x.device)
        arg = torch.empty((B, c), dtype=torch.int32, device=x.device) if mode == MAX else None
        self._ok(self.lib.pp_seg_reduce(x.data_ptr(), n, c, ldx, _dev(coords, torch.int32, "coords"), B, int(mode),
                                        out.data_ptr(), count.data_ptr(), None if arg is None else arg.data_ptr(),
                                        ws.data_ptr(), ws.numel(), self._stream(x)), "seg_reduce")
        return out, count, arg

    def seg_max_bwd(self, dy: torch.Tensor, arg: torch.Tensor, n: int) -> torch.Tensor:
        """dy fp32 [B, c], arg int32 [B, c] -> dx fp32 [n, c]."""
        B, c = (int(v) for v in dy.shape)
        assert tuple(arg.shape) == (B, c)
        dx = torch.empty((int(n), c), dtype=torch.float32, device=dy.device)
        self._ok(self.lib.pp_seg_max_bwd(_f32(dy, "dy"), _dev(arg, torch.int32, "arg"), B, c, int(n), dx.data_ptr(),
                                         self._stream(dy)), "seg_max_bwd")
        return dx

    def broadcast(self, x: Optional[torch.Tensor], g: torch.Tensor, coords: torch.Tensor, mode: int,
                  cnt: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x fp32 [n, c] (None for BC_COPY), g fp32 [B, cg], coords int32 [n, 4] -> out fp32 [n, c | c + cg | cg]."""
        n = int(coords.shape[0])
        B, cg = (int(v) for v in g.shape)
        c = 0 if x is None else int(x.shape[1])
        assert (x is None) == (mode == BC_COPY) and (x is None or int(x.shape[0]) == n) and tuple(coords.shape) == (n, 4)
        if not 1 <= B <= PP_MAX_BATCH:
            raise ValueError(f"broadcast: {B} batch indices, at most {PP_MAX_BATCH} (PP_MAX_BATCH) are served")
        width = {BC_ADD: c, BC_MUL: c, BC_CAT: c + cg, BC_COPY: cg}[mode]
        out = torch.empty((n, width), dtype=torch.float32, device=g.device)
        self._ok(self.lib.pp_broadcast(_f32(x, "x"), n, c, _f32(g, "g"), cg, _dev(coords, torch.int32, "coords"), B,
                                       _f32(cnt, "cnt"), int(mode), out.data_ptr(), self._stream(g)), "broadcast")
        return out

    def broadcast_mul_bwd(self, dy: torch.Tensor, x: torch.Tensor, g: torch.Tensor, coords: torch.Tensor, need_x: bool = True,
                          need_g: bool = True):
        """dy, x fp32 [n, c], g fp32 [B, c] -> (dx fp32 [n, c] | None, dg fp32 [B, c] | None)."""
        n, c = (int(v) for v in dy.shape)
        B = int(g.shape[0])
        assert tuple(x.shape) == (n, c) and tuple(g.shape) == (B, c) and tuple(coords.shape) == (n, 4)
        ws = self._seg_ws("broadcast_mul_bwd", n, c, B, dy.device)
        dx = torch.empty((n, c), dtype=torch.float32, device=dy.device) if need_x else None
        dg = torch.empty((B, c), dtype=torch.float32, device=dy.device) if need_g else None
        self._ok(self.lib.pp_broadcast_mul_bwd(_f32(dy, "dy"), _f32(x, "x"), _f32(g, "g"), _dev(coords, torch.int32, "coords"), n, c,
                                               B, None if dx is None else dx.data_ptr(), None if dg is None else dg.data_ptr(),
                                               ws.data_ptr(), ws.numel(), self._stream(dy)), "broadcast_mul_bwd")
        return dx, dg

    def pool(self, x: torch.Tensor, nbr: torch.Tensor, mode: int):
        """x fp32 [n_in, c], nbr int32 [K, n_out] -> (out fp32 [n_out, c], cnt fp32 [n_out])."""
        (n_in, c), (K, n_out) = (int(v) for v in x.shape), (int(v) for v in nbr.shape)
        out = torch.empty((n_out, c), dtype=torch.float32, device=x.device)
        cnt = torch.empty(n_out, dtype=torch.float32, device=x.device)
        self._ok(self.lib.pp_pool(_f32(x, "x"), n_in, c, _dev(nbr, torch.int32, "nbr"), K, n_out, int(mode), out.data_ptr(),
                                  cnt.data_ptr(), self._stream(x)), "pool")
        return out, cnt

    def pool_bwd(self, dy: torch.Tensor, cnt: Optional[torch.Tensor], inv: torch.Tensor, n_in: int, mode: int) -> torch.Tensor:
        """dy fp32 [n_out, c], cnt fp32 [n_out] (AVG), inv int32 [K, n_in] -> dx fp32 [n_in, c]."""
        (n_out, c), K, n_in = (int(v) for v in dy.shape), int(inv.shape[0]), int(n_in)
        assert tuple(inv.shape) == (K, n_in) and (cnt is None or int(cnt.numel()) == n_out)
        dx = torch.empty((n_in, c), dtype=torch.float32, device=dy.device)
        self._ok(self.lib.pp_pool_bwd(_f32(dy, "dy"), n_out, c, _f32(cnt, "cnt"), _dev(inv, torch.int32, "inv"), K, n_in, int(mode),
                                      dx.data_ptr(), self._stream(dy)), "pool_bwd")
        return dx

    def chconv_fwd(self, x: torch.Tensor, nbr: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x fp32 [n_in, c], nbr int32 [K, n_out], w fp32 [K, c], bias fp32 [c] | None -> out fp32 [n_out, c]."""
        (n_in, c), (K, n_out) = (int(v) for v in x.shape), (int(v) for v in nbr.shape)
        assert tuple(w.shape) == (K, c) and (bias is None or int(bias.numel()) == c)
        out = torch.empty((n_out, c), dtype=torch.float32, device=x.device)
        self._ok(self.lib.pp_chconv_fwd(_f32(x, "x"), n_in, c, _dev(nbr, torch.int32, "nbr"), K, n_out, _f32(w, "w"),
                                        _f32(bias, "bias"), out.data_ptr(), self._stream(x)), "chconv_fwd")
        return out

    def chconv_wgrad(self, x: torch.Tensor, dy: torch.Tensor, nbr: torch.Tensor) -> torch.Tensor:
        """x fp32 [n_in, c], dy fp32 [n_out, c], nbr int32 [K, n_out] -> dw fp32 [K, c]."""
        (n_in, c), (K, n_out) = (int(v) for v in x.shape), (int(v) for v in nbr.shape)
        assert tuple(dy.shape) == (n_out, c)
        need = int(self.lib.pp_chconv_wgrad_workspace_bytes(K, c, n_out))
        if need < 0:
            raise ValueError(f"chconv_wgrad: K = {K} (at most {PP_MAX_KVOL}), c = {c}, n_out = {n_out} is outside the served range")
        ws = self._scratch(x.device, need)
        dw = torch.empty((K, c), dtype=torch.float32, device=x.device)
        self._ok(self.lib.pp_chconv_wgrad(_f32(x, "x"), n_in, c, _f32(dy, "dy"), n_out, _dev(nbr, torch.int32, "nbr"), K,
                                          dw.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(x)), "chconv_wgrad")
        return dw


def pool_lib() -> PoolLib:
    """The process-wide binding of libpascohip.so's pooling / broadcast / channel-wise kernels (a missing library is an error)."""
    return shared(PoolLib)
