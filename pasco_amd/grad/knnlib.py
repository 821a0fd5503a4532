"""ctypes binding of include/pasco_knn.h (the `pk_*` entry points of libpascohip.so): the exact bipartite k-nearest-neighbour
search over a uniform grid, the inverse-squared-distance weights and the weighted row gather - what `pasco_amd.grad.knn.knn_up`
runs on the device.

Kept apart from `me.backend` like `grad.fieldlib`: the CPU oracle has none of these kernels (`pasco_amd.grad.host` restates them:
knn_search, knn_weights, knn_interp).  Every method takes device tensors and enqueues on the caller's current stream; nothing
synchronises.  `csr` builds the search structure with the kernels two other families already own: `pw_grid_cells`
(include/pasco_waffle.h) and `pq_group` (include/pasco_field.h), whose offsets / perm are the CSR's start / order."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared
from ..waffle.host import SearchGrid

PK_ABI_VERSION = 1       # include/pasco_knn.h PK_ABI_VERSION this binding was written against
PK_MAX_K = 16
PK_QUERY_BLOCK = 64
PK_MAX_CELLS = 1 << 24
MAX_LIST = 1 << 24       # k * m of one backward: the list entries pq_group serves

_vp, _i64, _i32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
_GRID = [_f64, _f64, _f64, _f64, _i32, _i32, _i32]
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "knn": [_vp, _i32, _i64, _vp, _vp, *_GRID, _vp, _i32, _i64, _i32, _vp, _vp, _vp],
    "weights": [_vp, _vp, _i32, _i64, _vp, _vp],
    "interp_fwd": [_vp, _i64, _i32, _vp, _vp, _i32, _i64, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p}


def _xyz(t: torch.Tensor, what: str):
    """A 2-D fp32 device tensor of at least three columns whose rows are contiguous (a column slice of a wider matrix is fine:
    column 1 of a [N, 4] batched-coordinate matrix) -> (pointer, ld)."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise TypeError(f"{what}: the pk_* kernels serve fp32 device tensors, got {t.dtype} on {t.device}")
    assert t.dim() == 2 and t.shape[1] >= 3 and t.stride(1) == 1, f"{what}: rows of x, y, z with unit column stride"
    return t.data_ptr(), int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


def _f32(t: torch.Tensor, what: str) -> int:
    if t.dtype != torch.float32:
        raise TypeError(f"{what}: the pk_* kernels serve fp32 rows, got {t.dtype}")
    return _dev(t, torch.float32, what)


def _check_k(k: int) -> int:
    k = int(k)
    if not 1 <= k <= PK_MAX_K:
        raise ValueError(f"k = {k}: 1 .. {PK_MAX_K} neighbours are served")
    return k


class KnnLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pk_", PK_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    @staticmethod
    def _g(g: SearchGrid):
        return (float(g.lo[0]), float(g.lo[1]), float(g.lo[2]), float(g.h), int(g.G[0]), int(g.G[1]), int(g.G[2]))

    def csr(self, cand: torch.Tensor, g: SearchGrid, status: torch.Tensor):
        """cand fp32 [n, >= 3] -> (start int32 [ncell + 1], order int32 [n]) of the candidates over `g`; a candidate outside the grid
        ORs PW_STATUS_OFF_GRID into `status` (int32 [1], the caller's).  n < 2^24: `pq_group`'s range, narrower than the n < 2^31
        pk_knn itself takes (`knn.knn_search` refuses more by name)."""
        from ..waffle.lib import waffle_lib
        from .fieldlib import field_lib
        cell = waffle_lib().grid_cells(cand, g, status)
        return field_lib().group(cell, g.ncell)

    def knn(self, cand: torch.Tensor, start: torch.Tensor, order: torch.Tensor, g: SearchGrid, q: torch.Tensor, k: int):
        """-> (idx int32 [k, m], d2 fp32 [k, m]), nearest first; -1 / +inf where fewer than k candidates exist."""
        k = _check_k(k)
        cptr, ldc = _xyz(cand, "cand")
        qptr, ldq = _xyz(q, "q")
        n, m = int(cand.shape[0]), int(q.shape[0])
        assert start.numel() >= g.ncell + 1 and order.numel() >= n
        idx = torch.empty((k, m), dtype=torch.int32, device=q.device)
        d2 = torch.empty((k, m), dtype=torch.float32, device=q.device)
        self._ok(self.lib.pk_knn(cptr, ldc, n, _dev(start, torch.int32, "start"), _dev(order, torch.int32, "order"), *self._g(g),
                                 qptr, ldq, m, k, idx.data_ptr(), d2.data_ptr(), self._stream(q)), "knn")
        return idx, d2

    def weights(self, d2: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """d2 fp32 [k, m], idx int32 [k, m] -> w fp32 [k, m]."""
        k, m = (int(v) for v in idx.shape)
        _check_k(k)
        assert tuple(d2.shape) == (k, m)
        w = torch.empty((k, m), dtype=torch.float32, device=d2.device)
        self._ok(self.lib.pk_weights(_f32(d2, "d2"), _dev(idx, torch.int32, "idx"), k, m, w.data_ptr(), self._stream(d2)), "weights")
        return w

    def interp_fwd(self, x: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
        """x fp32 [n, c], idx int32 [k, m], w fp32 [k, m] -> out fp32 [m, c]."""
        n, c = (int(v) for v in x.shape)
        k, m = (int(v) for v in idx.shape)
        _check_k(k)
        assert tuple(w.shape) == (k, m)
        if c < 1:
            raise ValueError("interp_fwd: rows of at least one channel are served")
        out = torch.empty((m, c), dtype=torch.float32, device=x.device)
        self._ok(self.lib.pk_interp_fwd(_f32(x, "x"), n, c, _dev(idx, torch.int32, "idx"), _f32(w, "w"), k, m, out.data_ptr(),
                                        self._stream(x)), "interp_fwd")
        return out

    def interp_bwd(self, dy: torch.Tensor, idx: torch.Tensor, w: torch.Tensor, n: int) -> torch.Tensor:
        """dy fp32 [m, c] -> dx fp32 [n, c]: dx[i] = the sum over the entries (j, p) with idx[j][p] == i, in ascending (j, p), of
        w[j][p] * dy[p] - `pq_group` over the flattened table, then `pq_seg_rows` with src_mod = m."""
        from .fieldlib import SUM, field_lib
        k, m = (int(v) for v in idx.shape)
        if k * m >= MAX_LIST:
            raise ValueError(f"knn_up backward: k * m = {k} * {m} = {k * m} list entries, fewer than 2^24 are served (split the points)")
        L = field_lib()
        offsets, perm = L.group(idx.reshape(-1), int(n))
        return L.seg_rows(dy, offsets, perm, SUM, w=w.reshape(-1), src_mod=max(m, 1))[0]


def knn_lib() -> KnnLib:
    """The process-wide binding of libpascohip.so's k-nearest-neighbour kernels (a missing library is an error)."""
    return shared(KnnLib)
