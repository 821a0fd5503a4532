"""ctypes binding of include/pasco_field.h (the `pq_*` entry points of libpascohip.so): the grouping of list entries by segment,
segment sums / averages / maxima, the weighted gather and the eight-corner interpolation - what `TensorField`, the quantisation
modes, `SparseTensor.slice` and `MinkowskiInterpolation` of `pasco_amd.me` run on the device.

Kept apart from `me.backend` like `grad.poollib`: the CPU oracle binds `me.backend._SIGNATURES` and has none of these kernels
(`pasco_amd.grad.host` restates them).  Every method takes device tensors and enqueues on the caller's current stream; nothing
synchronises.  The grouping's workspace is a buffer of the product backend's per-stream scratch table (`hip_backend().scratch`,
"field"), reused from call to call in stream order."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PQ_ABI_VERSION = 1       # include/pasco_field.h PQ_ABI_VERSION this binding was written against
PQ_SEG_ROWS = 64
PQ_CORNERS = 8
SUM, AVG, MAX = 0, 1, 2
MAX_LIST = 1 << 24       # list entries of one grouping / one pq_seg_rows call (the count is exact in fp32)
MAX_POINTS = 1 << 28     # points of one interpolation

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "group_workspace_bytes": [_i64, _i64],
    "group": [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp],
    "seg_rows": [_vp, _i64, _i32, _vp, _vp, _i64, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _vp],
    "seg_max_bwd": [_vp, _vp, _i64, _i32, _i64, _i64, _vp, _vp],
    "gather_w": [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _vp],
    "interp_map": [_vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "interp_fwd": [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "group_workspace_bytes": _i64}


def _f32(t: Optional[torch.Tensor], what: str) -> Optional[int]:
    """The address of a fp32 row matrix that may start anywhere on a 4-byte boundary (a view into a larger buffer)."""
    if t is None:
        return None
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: the pq_* kernels serve fp32 rows, got {t.dtype}")
    return _dev(t, torch.float32, what)


def _i32p(t: torch.Tensor, what: str) -> int:
    return _dev(t, torch.int32, what)


class FieldLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pq_", PQ_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    @staticmethod
    def _scratch(device, need: int) -> torch.Tensor:
        from ..me.backend import hip_backend
        return hip_backend().scratch.bytes("field", device, max(int(need), 16))

    def group_workspace_bytes(self, n: int, n_seg: int) -> int:
        return int(self.lib.pq_group_workspace_bytes(int(n), int(n_seg)))

    def group(self, keys: torch.Tensor, n_seg: int):
        """keys int32 [n] (absent: negative or >= n_seg) -> (offsets int32 [n_seg + 1], perm int32 [n]): the stable sort by key."""
        n, n_seg = int(keys.numel()), int(n_seg)
        if n >= MAX_LIST:
            raise ValueError(f"group: {n} list entries, fewer than 2^24 are served")
        if not 0 <= n_seg < (1 << 31):
            raise ValueError(f"group: {n_seg} segments, 0 .. 2^31 - 1 are served")
        ws = self._scratch(keys.device, self.group_workspace_bytes(n, n_seg))
        offsets = torch.empty(n_seg + 1, dtype=torch.int32, device=keys.device)
        perm = torch.empty(n, dtype=torch.int32, device=keys.device)
        self._ok(self.lib.pq_group(_i32p(keys, "keys"), n, n_seg, offsets.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel(),
                                   self._stream(keys)), "group")
        return offsets, perm

    def seg_rows(self, x: torch.Tensor, offsets: torch.Tensor, perm: torch.Tensor, mode: int, w: Optional[torch.Tensor] = None,
                 src_mod: Optional[int] = None):
        """x fp32 [n_src, c], (offsets, perm) of `group` -> (out fp32 [n_seg, c], cnt fp32 [n_seg], arg int32 [n_seg, c] | None)."""
        n_src, c = (int(v) for v in x.shape)
        n_seg, n_list = int(offsets.numel()) - 1, int(perm.numel())
        if n_list >= MAX_LIST:
            raise ValueError(f"seg_rows: {n_list} list entries, fewer than 2^24 are served")
        if c < 1:
            raise ValueError("seg_rows: rows of at least one channel are served")
        assert w is None or int(w.numel()) == n_list
        src_mod = max(n_list, 1) if src_mod is None else int(src_mod)
        out = torch.empty((n_seg, c), dtype=torch.float32, device=x.device)
        cnt = torch.empty(n_seg, dtype=torch.float32, device=x.device)
        arg = torch.empty((n_seg, c), dtype=torch.int32, device=x.device) if mode == MAX else None
        self._ok(self.lib.pq_seg_rows(_f32(x, "x"), n_src, c, _i32p(offsets, "offsets"), _i32p(perm, "perm"), n_list, n_seg,
                                      _f32(w, "w"), src_mod, int(mode), out.data_ptr(), cnt.data_ptr(),
                                      None if arg is None else arg.data_ptr(), self._stream(x)), "seg_rows")
        return out, cnt, arg

    def seg_max_bwd(self, dy: torch.Tensor, arg: torch.Tensor, n_src: int, src_mod: Optional[int] = None) -> torch.Tensor:
        """dy fp32 [n_seg, c], arg int32 [n_seg, c] -> dx fp32 [n_src, c]."""
        n_seg, c = (int(v) for v in dy.shape)
        assert tuple(arg.shape) == (n_seg, c)
        n_src = int(n_src)
        src_mod = max(n_src, 1) if src_mod is None else int(src_mod)
        dx = torch.empty((n_src, c), dtype=torch.float32, device=dy.device)
        self._ok(self.lib.pq_seg_max_bwd(_f32(dy, "dy"), _i32p(arg, "arg"), n_seg, c, n_src, src_mod, dx.data_ptr(),
                                         self._stream(dy)), "seg_max_bwd")
        return dx

    def gather_w(self, x: torch.Tensor, idx: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
        """x fp32 [n_src, c], idx int32 [n], d fp32 [n_src] -> out fp32 [n, c] = x[idx] * (1 / d[idx])."""
        n_src, c = (int(v) for v in x.shape)
        n = int(idx.numel())
        assert int(d.numel()) == n_src
        out = torch.empty((n, c), dtype=torch.float32, device=x.device)
        self._ok(self.lib.pq_gather_w(_f32(x, "x"), n_src, c, _i32p(idx, "idx"), n, _f32(d, "d"), out.data_ptr(), self._stream(x)),
                 "gather_w")
        return out

    def interp_map(self, points: torch.Tensor, tkeys: torch.Tensor, tvals: torch.Tensor, ts: int):
        """points fp32 [m, 4], a coordinate map's table -> (rows int32 [8, m], weights fp32 [8, m])."""
        m = int(points.shape[0])
        assert tuple(points.shape) == (m, 4)
        if m >= MAX_POINTS:
            raise ValueError(f"interp_map: {m} points, fewer than 2^28 are served")
        rows = torch.empty((PQ_CORNERS, m), dtype=torch.int32, device=points.device)
        weights = torch.empty((PQ_CORNERS, m), dtype=torch.float32, device=points.device)
        self._ok(self.lib.pq_interp_map(_f32(points, "points"), m, _dev(tkeys, torch.int64, "tkeys"), _i32p(tvals, "tvals"),
                                        int(tkeys.numel()), int(ts), rows.data_ptr(), weights.data_ptr(), self._stream(points)),
                 "interp_map")
        return rows, weights

    def interp_fwd(self, x: torch.Tensor, rows: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
        """x fp32 [n_in, c], rows int32 [8, m], weights fp32 [8, m] -> out fp32 [m, c]."""
        n_in, c = (int(v) for v in x.shape)
        m = int(rows.shape[1])
        assert tuple(rows.shape) == (PQ_CORNERS, m) == tuple(weights.shape)
        out = torch.empty((m, c), dtype=torch.float32, device=x.device)
        self._ok(self.lib.pq_interp_fwd(_f32(x, "x"), n_in, c, _i32p(rows, "rows"), _f32(weights, "weights"), m, out.data_ptr(),
                                        self._stream(x)), "interp_fwd")
        return out


def field_lib() -> FieldLib:
    """The process-wide binding of libpascohip.so's point <-> voxel kernels (a missing library is an error)."""
    return shared(FieldLib)
