"""ctypes binding of include/pasco_waffle.h (the `pw_*` entry points of libpascohip.so): WaffleIron point features on the device.

Kept apart from `me.backend` like `viz.lib`: the CPU oracle binds `me.backend._SIGNATURES` and has no waffle kernels.
Every method takes device tensors and enqueues on the caller's current stream; nothing synchronises.  The one piece of torch
plumbing is the stable sort in `cells_build` (the kernel checks the permutation it is given)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared
from .host import SearchGrid

PW_ABI_VERSION = 1       # include/pasco_waffle.h PW_ABI_VERSION this binding was written against

_vp, _i64, _i32, _f32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_double
_GRID = [_f64, _f64, _f64, _f64, _i32, _i32, _i32]
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "voxel_keys": [_vp, _i32, _i64, _vp, _f32, _vp, _vp, _vp],
    "cell_index": [_vp, _i32, _i64, _i32, _i32, _f64, _f64, _f64, _f64, _i32, _i32, _vp, _vp, _vp],
    "grid_cells": [_vp, _i32, _i64, *_GRID, _vp, _vp, _vp],
    "cells_build": [_vp, _vp, _i64, _i32, _vp, _vp, _vp],
    "knn": [_vp, _i32, _i64, _vp, _vp, *_GRID, _i32, _vp, _vp],
    "nearest": [_vp, _i32, _i64, _vp, _vp, *_GRID, _vp, _i32, _i64, _vp, _vp],
    "flatten": [_vp, _i64, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "dwconv3x3": [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "inflate": [_vp, _i64, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp],
    "neigh_rows": [_vp, _i64, _i32, _vp, _i32, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp],
    "group_max": [_vp, _i64, _i32, _i32, _vp, _i32, _vp],
}
_RESTYPES = {"last_error": C.c_char_p}


def _rows(t: torch.Tensor, what: str):
    """A 2-D fp32 device tensor whose rows are contiguous (a column slice of a wider matrix is fine) -> (pointer, ld)."""
    assert t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), what
    return t.data_ptr(), int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


class WaffleLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pw_", PW_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    @staticmethod
    def new_status(device) -> torch.Tensor:
        return torch.zeros(1, dtype=torch.int32, device=device)

    @staticmethod
    def _g(g: SearchGrid):
        return (float(g.lo[0]), float(g.lo[1]), float(g.lo[2]), float(g.h), int(g.G[0]), int(g.G[1]), int(g.G[2]))

    # ---- preparation ----------------------------------------------------------------------------------------------
    def voxel_keys(self, pc: torch.Tensor, mn: torch.Tensor, voxel: float, status: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pc fp32 [n, >= 3], mn fp32 [3] -> int32 [n, 3]."""
        ptr, ld = _rows(pc, "pc")
        n = int(pc.shape[0])
        out = torch.empty((n, 3), dtype=torch.int32, device=pc.device) if out is None else out
        assert out.numel() >= 3 * n and mn.numel() == 3
        self._ok(self.lib.pw_voxel_keys(ptr, ld, n, _dev(mn, torch.float32, "mn"), float(voxel), _dev(out, torch.int32, "key"),
                                        _dev(status, torch.int32, "status"), self._stream(pc)), "voxel_keys")
        return out

    def cell_index(self, pc: torch.Tensor, dims, lo, res, shape, status: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pc fp32 [n, ld] -> int32 [n]: the cell on the 2-D grid `shape` of the plane `dims`."""
        ptr, ld = _rows(pc, "pc")
        n = int(pc.shape[0])
        out = torch.empty(n, dtype=torch.int32, device=pc.device) if out is None else out
        assert out.numel() >= n
        self._ok(self.lib.pw_cell_index(ptr, ld, n, int(dims[0]), int(dims[1]), float(lo[0]), float(lo[1]), float(res[0]),
                                        float(res[1]), int(shape[0]), int(shape[1]), _dev(out, torch.int32, "cell"),
                                        _dev(status, torch.int32, "status"), self._stream(pc)), "cell_index")
        return out

    def grid_cells(self, xyz: torch.Tensor, g: SearchGrid, status: torch.Tensor,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
        ptr, ld = _rows(xyz, "xyz")
        n = int(xyz.shape[0])
        out = torch.empty(n, dtype=torch.int32, device=xyz.device) if out is None else out
        assert out.numel() >= n
        self._ok(self.lib.pw_grid_cells(ptr, ld, n, *self._g(g), _dev(out, torch.int32, "cell"),
                                        _dev(status, torch.int32, "status"), self._stream(xyz)), "grid_cells")
        return out

    def cells_build(self, cell: torch.Tensor, ncell: int, status: torch.Tensor, start: Optional[torch.Tensor] = None,
                    order: Optional[torch.Tensor] = None):
        """cell int32 [n] -> (start int32 [ncell + 1], order int32 [n]); `order` given = the caller's own permutation."""
        n = int(cell.shape[0])
        if order is None:
            order = torch.sort(cell, stable=True)[1].to(torch.int32)
        start = torch.empty(ncell + 1, dtype=torch.int32, device=cell.device) if start is None else start
        assert start.numel() >= ncell + 1 and order.numel() >= n
        self._ok(self.lib.pw_cells_build(_dev(cell, torch.int32, "cell"), _dev(order, torch.int32, "order"), n, int(ncell),
                                         _dev(start, torch.int32, "start"), _dev(status, torch.int32, "status"),
                                         self._stream(cell)), "cells_build")
        return start, order

    def knn(self, xyz: torch.Tensor, start: torch.Tensor, order: torch.Tensor, g: SearchGrid, k: int,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
        ptr, ld = _rows(xyz, "xyz")
        n = int(xyz.shape[0])
        out = torch.empty((n, k), dtype=torch.int32, device=xyz.device) if out is None else out
        assert out.numel() >= n * k and start.numel() >= g.ncell + 1 and order.numel() >= n
        self._ok(self.lib.pw_knn(ptr, ld, n, _dev(start, torch.int32, "start"), _dev(order, torch.int32, "order"), *self._g(g),
                                 int(k), _dev(out, torch.int32, "out"), self._stream(xyz)), "knn")
        return out

    def nearest(self, xyz: torch.Tensor, start: torch.Tensor, order: torch.Tensor, g: SearchGrid, q: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        ptr, ld = _rows(xyz, "xyz")
        qptr, ldq = _rows(q, "q")
        n, m = int(xyz.shape[0]), int(q.shape[0])
        out = torch.empty(m, dtype=torch.int32, device=xyz.device) if out is None else out
        assert out.numel() >= m and start.numel() >= g.ncell + 1 and order.numel() >= n
        self._ok(self.lib.pw_nearest(ptr, ld, n, _dev(start, torch.int32, "start"), _dev(order, torch.int32, "order"),
                                     *self._g(g), qptr, ldq, m, _dev(out, torch.int32, "out"), self._stream(xyz)), "nearest")
        return out

    # ---- network ---------------------------------------------------------------------------------------------------
    def flatten(self, tokens: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, start: torch.Tensor, order: torch.Tensor,
                ncell: int, status: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        n, Cn = (int(v) for v in tokens.shape)
        out = torch.empty((ncell, Cn), dtype=torch.float32, device=tokens.device) if out is None else out
        assert out.numel() >= ncell * Cn and scale.numel() == Cn == shift.numel() and start.numel() >= ncell + 1
        assert order.numel() >= n
        self._ok(self.lib.pw_flatten(_dev(tokens, torch.float32, "tokens"), n, Cn, _dev(scale, torch.float32, "scale"),
                                     _dev(shift, torch.float32, "shift"), _dev(start, torch.int32, "start"),
                                     _dev(order, torch.int32, "order"), int(ncell), _dev(out, torch.float32, "grid"),
                                     _dev(status, torch.int32, "status"), self._stream(tokens)), "flatten")
        return out

    def dwconv3x3(self, grid: torch.Tensor, H: int, W: int, w: torch.Tensor, bias: torch.Tensor, relu: bool,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """grid fp32 [H * W, C] (or [H, W, C]), w fp32 [9, C] -> fp32 of the same shape."""
        Cn = int(grid.shape[-1])
        out = torch.empty_like(grid) if out is None else out
        assert grid.numel() == H * W * Cn and out.numel() >= grid.numel() and tuple(w.shape) == (9, Cn) and bias.numel() == Cn
        self._ok(self.lib.pw_dwconv3x3(_dev(grid, torch.float32, "in"), int(H), int(W), Cn, _dev(w, torch.float32, "w"),
                                       _dev(bias, torch.float32, "bias"), int(bool(relu)), _dev(out, torch.float32, "out"),
                                       self._stream(grid)), "dwconv3x3")
        return out

    def inflate(self, tokens: torch.Tensor, scale: torch.Tensor, grid: torch.Tensor, cell: torch.Tensor, status: torch.Tensor,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        n, Cn = (int(v) for v in tokens.shape)
        ncell = grid.numel() // Cn
        out = torch.empty_like(tokens) if out is None else out
        assert out.numel() >= n * Cn and scale.numel() == Cn and cell.numel() >= n
        self._ok(self.lib.pw_inflate(_dev(tokens, torch.float32, "tokens"), n, Cn, _dev(scale, torch.float32, "scale"),
                                     _dev(grid, torch.float32, "grid"), _dev(cell, torch.int32, "cell"), ncell,
                                     _dev(out, torch.float32, "out"), _dev(status, torch.int32, "status"),
                                     self._stream(tokens)), "inflate")
        return out

    def neigh_rows(self, feat: torch.Tensor, knn: torch.Tensor, p0: int, np_: int, A: torch.Tensor, b: torch.Tensor,
                   status: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        n, F = (int(v) for v in feat.shape)
        k, Cn = int(knn.shape[1]), int(A.shape[1])
        out = torch.empty((np_ * k, Cn), dtype=torch.float32, device=feat.device) if out is None else out
        assert out.numel() >= np_ * k * Cn and tuple(A.shape) == (F, Cn) and b.numel() == Cn and knn.shape[0] == n
        self._ok(self.lib.pw_neigh_rows(_dev(feat, torch.float32, "feat"), n, F, _dev(knn, torch.int32, "knn"), k, int(p0),
                                        int(np_), _dev(A, torch.float32, "A"), _dev(b, torch.float32, "b"), Cn,
                                        _dev(out, torch.float32, "rows"), _dev(status, torch.int32, "status"),
                                        self._stream(feat)), "neigh_rows")
        return out

    def group_max(self, rows: torch.Tensor, np_: int, k: int, out: torch.Tensor) -> torch.Tensor:
        """rows fp32 [np * k, C] -> out fp32 [np, C] (rows of `out` may be a column slice of a wider matrix)."""
        Cn = int(rows.shape[1])
        optr, ld = _rows(out, "out")
        assert rows.numel() >= np_ * k * Cn and tuple(out.shape) == (np_, Cn)
        self._ok(self.lib.pw_group_max(_dev(rows, torch.float32, "rows"), int(np_), int(k), Cn, optr, ld, self._stream(rows)),
                 "group_max")
        return out


def waffle_lib() -> WaffleLib:
    """The process-wide binding of libpascohip.so's waffle kernels (a missing library is an error)."""
    return shared(WaffleLib)
