"""ctypes binding of include/pasco_attngrad.h (the `pa_*` entry points of libpascohip.so): the backward of the masked
cross-attention `ph_attn_cross_fwd`.

Kept apart from `me.backend` like `grad.lib` and `grad.rowlib`: the CPU oracle binds `me.backend._SIGNATURES` and has no gradient
kernels.  Every method takes device tensors and enqueues on the caller's current stream; nothing synchronises.  The scratch is a
buffer of the product backend's per-stream scratch table (`hip_backend().scratch`, "attn_bwd"), as the forward's ("attn") is: it is reused from call to call
in stream order and dropped by `release_stream`."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PA_ABI_VERSION = 1       # include/pasco_attngrad.h PA_ABI_VERSION this binding was written against
PA_DH = 48
PA_MAX_Q = 128

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "attn_bwd_workspace_bytes": [_i64, _i32, _i32, _i32, _i32],
    "attn_bwd_stats": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _vp],
    "attn_cross_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i64, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "attn_bwd_workspace_bytes": _i64}


def _opt(t: Optional[torch.Tensor], dtype, what: str):
    return None if t is None else _dev(t, dtype, what)


class AttnGradLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pa_", PA_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def workspace_bytes(self, n: int, b: int, h: int, qn: int, dh: int = PA_DH) -> int:
        return int(self.lib.pa_attn_bwd_workspace_bytes(int(n), int(b), int(h), int(qn), int(dh)))

    def _workspace(self, need: int, device: torch.device) -> torch.Tensor:
        from ..me.backend import hip_backend
        return hip_backend().scratch.bytes("attn_bwd", device, need)

    @staticmethod
    def _shape(q, k):
        b, h, qn, dh = (int(x) for x in q.shape)
        n = int(k.shape[1])
        assert tuple(k.shape) == (b, n, h * dh), "k: [B, N, H*Dh]"
        if dh != PA_DH or not 1 <= qn <= PA_MAX_Q:
            raise ValueError(f"attention backward: head dim {dh} / {qn} queries not served (head dim {PA_DH}, 1..{PA_MAX_Q} queries)")
        return b, h, qn, dh, n

    def attn_bwd_stats(self, q, k, bits, any_, out, dout):
        """-> (lse, delta) fp32 [B, H, Qn]: the statistics pass alone."""
        b, h, qn, dh, n = self._shape(q, k)
        lse = torch.empty((b, h, qn), dtype=torch.float32, device=q.device)
        delta = torch.empty_like(lse)
        need = self.workspace_bytes(n, b, h, qn, dh)
        ws = self._workspace(need, q.device)
        f32, i32 = torch.float32, torch.int32
        self._ok(self.lib.pa_attn_bwd_stats(_dev(q, f32, "q"), _dev(k, f32, "k"), _opt(bits, i32, "bits"), _opt(any_, i32, "any"),
                                            _dev(out, f32, "out"), _dev(dout, f32, "dout"), _dev(lse, f32, "lse"),
                                            _dev(delta, f32, "delta"), n, b, h, qn, dh, ws.data_ptr(), ws.numel(),
                                            self._stream(q)), "attn_bwd_stats")
        return lse, delta

    def attn_cross_bwd(self, q, k, v, bits, any_, out, dout, need_q: bool = True, need_k: bool = True, need_v: bool = True):
        """q [B,H,Qn,48] (pre-scaled), k / v [B,N,H*48], bits int32 [B,N,4] | None, any int32 [B,4] | None, out / dout
        [B,Qn,H*48] -> (dq, dk, dv), None where not needed."""
        b, h, qn, dh, n = self._shape(q, k)
        assert tuple(v.shape) == tuple(k.shape) and tuple(out.shape) == (b, qn, h * dh) and tuple(dout.shape) == tuple(out.shape)
        assert bits is None or tuple(bits.shape) == (b, n, 4)
        assert any_ is None or tuple(any_.shape) == (b, 4)
        dq = torch.empty_like(q) if need_q else None
        dk = torch.empty_like(k) if need_k else None
        dv = torch.empty_like(v) if need_v else None
        need = self.workspace_bytes(n, b, h, qn, dh)
        ws = self._workspace(need, q.device)
        f32, i32 = torch.float32, torch.int32
        self._ok(self.lib.pa_attn_cross_bwd(_dev(q, f32, "q"), _dev(k, f32, "k"), _dev(v, f32, "v"), _opt(bits, i32, "bits"),
                                            _opt(any_, i32, "any"), _dev(out, f32, "out"), _dev(dout, f32, "dout"),
                                            _opt(dq, f32, "dq"), _opt(dk, f32, "dk"), _opt(dv, f32, "dv"), n, b, h, qn, dh,
                                            ws.data_ptr(), ws.numel(), self._stream(q)), "attn_cross_bwd")
        return dq, dk, dv


def attn_grad_lib() -> AttnGradLib:
    """The process-wide binding of libpascohip.so's attention gradient kernels (a missing library is an error)."""
    return shared(AttnGradLib)
