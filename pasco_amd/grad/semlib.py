"""ctypes binding of include/pasco_semloss.h (the `ps_*` entry points of libpascohip.so): the rows of the semantic completion
losses (box test, labels, cross-entropy sums, sort keys), the segmented descending radix sort, the Lovasz increments along the
sorted order, and the gradient of both losses in one pass.

Kept apart from `me.backend` like `grad.matchlib`.  Every method takes device tensors and enqueues on the caller's current
stream; nothing synchronises.  The scratch of a forward (keys, order and the three stages' partials: `geometry(n, c)`) is ONE
buffer of the product backend's per-stream scratch table (`hip_backend().scratch`, "semloss"): reused from call to call in stream order and
dropped by `release_stream`."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared

PS_ABI_VERSION = 1       # include/pasco_semloss.h PS_ABI_VERSION this binding was written against
PS_MIN_C, PS_MAX_C = 2, 32
PS_MAX_N = 1 << 24
LABEL_IGNORE, LABEL_OUTSIDE = 255, 254
SORT_TILE = 2048
MIN_RANGE_ROWS = 256
MAX_RANGES = 256
PART_WORDS = 40
GEOMETRY_WORDS = ("tile", "tiles", "range_rows", "ranges", "keys_bytes", "perm_bytes", "sort_bytes", "rows_bytes", "lovasz_bytes",
                  "workspace_bytes")

_vp, _i64, _i32 = C.c_void_p, C.c_int64, C.c_int32
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "geometry": [_i64, _i32, _vp],
    "workspace_bytes": [_i64, _i32],
    "sort_workspace_bytes": [_i64, _i64],
    "rows_fwd": [_vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "sort_desc": [_vp, _i64, _i64, _vp, _vp, _i64, _vp],
    "lovasz_fwd": [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp],
    "loss_bwd": [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "workspace_bytes": _i64, "sort_workspace_bytes": _i64}


def _pad256(v: int) -> int:
    return -(-v // 256) * 256


def sort_workspace_bytes(s: int, m: int) -> int:
    """The scratch of ps_sort_desc, restated from csrc/semloss.hip: two key buffers, one index buffer, the digit counts."""
    if not (1 <= s <= 65535 and 0 <= m <= PS_MAX_N):
        return 0
    return 3 * _pad256(4 * s * m) + _pad256(4 * s * -(-m // SORT_TILE) * 256)


def geometry(n: int, c: int) -> dict:
    """The geometry of one forward, restated from csrc/semloss.hip: the sort's `tile` keys and `tiles` per class, `ranges` of
    `range_rows` rows in ps_rows_fwd (a multiple of 256, so that there are at most 256 ranges), and the bytes of the five parts of
    the workspace in their order, each padded to 256."""
    if not (0 <= n <= PS_MAX_N and PS_MIN_C <= c <= PS_MAX_C):
        return dict.fromkeys(GEOMETRY_WORDS, 0)
    tiles = -(-n // SORT_TILE)
    rr = max(MIN_RANGE_ROWS, -(-(-(-n // MAX_RANGES)) // MIN_RANGE_ROWS) * MIN_RANGE_ROWS)
    ranges = -(-n // rr)
    g = {"tile": SORT_TILE, "tiles": tiles, "range_rows": rr, "ranges": ranges, "keys_bytes": _pad256(4 * c * n),
         "perm_bytes": _pad256(4 * c * n), "sort_bytes": sort_workspace_bytes(c, n), "rows_bytes": _pad256(4 * PART_WORDS * ranges),
         "lovasz_bytes": _pad256(12 * c * tiles)}
    g["workspace_bytes"] = g["keys_bytes"] + g["perm_bytes"] + g["sort_bytes"] + g["rows_bytes"] + g["lovasz_bytes"]
    return g


def check_classes(c: int):
    if not (PS_MIN_C <= c <= PS_MAX_C):
        raise ValueError(f"semantic completion loss: {c} classes not served ({PS_MIN_C}..{PS_MAX_C})")


class SemLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("ps_", PS_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def geometry(self, n: int, c: int) -> dict:
        g = (C.c_int64 * len(GEOMETRY_WORDS))()
        self._ok(self.lib.ps_geometry(int(n), int(c), C.cast(g, C.c_void_p)), "geometry")
        return dict(zip(GEOMETRY_WORDS, (int(v) for v in g)))

    def workspace_bytes(self, n: int, c: int) -> int:
        return int(self.lib.ps_workspace_bytes(int(n), int(c)))

    def sort_workspace_bytes(self, s: int, m: int) -> int:
        return int(self.lib.ps_sort_workspace_bytes(int(s), int(m)))

    def _workspace(self, need: int, device: torch.device) -> torch.Tensor:
        from ..me.backend import hip_backend
        return hip_backend().scratch.bytes("semloss", device, need, floor=256)

    @staticmethod
    def parts(ws: torch.Tensor, n: int, c: int, g: dict):
        """The five parts of a forward's workspace as views: keys int32 [C, N], perm int32 [C, N], sort, rows, lovasz (bytes)."""
        o = 0
        out = []
        for name in ("keys_bytes", "perm_bytes", "sort_bytes", "rows_bytes", "lovasz_bytes"):
            out.append(ws[o:o + g[name]])
            o += g[name]
        keys = out[0][:4 * c * n].view(torch.int32).view(c, n)
        perm = out[1][:4 * c * n].view(torch.int32).view(c, n)
        return keys, perm, out[2], out[3], out[4]

    def rows_fwd(self, logits, coords, target, box, scale: int, weights, keys, ws):
        """logits fp32 [N,C], coords int32 [N,4], target uint8 [X,Y,Z], box int32 [6], weights fp32 [C]; keys int32 [C,N] and ws
        are written -> (label uint8 [N], ce fp32 [3], class_count int32 [C], info int32 [4])."""
        n, c = (int(x) for x in logits.shape)
        check_classes(c)
        assert tuple(coords.shape) == (n, 4) and target.dim() == 3 and tuple(box.shape) == (6,) and tuple(weights.shape) == (c,)
        assert tuple(keys.shape) == (c, n)
        dev = logits.device
        label = torch.empty((n,), dtype=torch.uint8, device=dev)
        ce = torch.empty((3,), dtype=torch.float32, device=dev)
        class_count = torch.empty((c,), dtype=torch.int32, device=dev)
        info = torch.empty((4,), dtype=torch.int32, device=dev)
        f32, i32 = torch.float32, torch.int32
        dx, dy, dz = (int(x) for x in target.shape)
        self._ok(self.lib.ps_rows_fwd(_dev(logits, f32, "logits"), _dev(coords, i32, "coords"), _dev(target, torch.uint8, "target"),
                                      _dev(box, i32, "box"), int(scale), _dev(weights, f32, "weights"), n, c, dx, dy, dz,
                                      label.data_ptr(), ce.data_ptr(), class_count.data_ptr(), info.data_ptr(),
                                      _dev(keys, i32, "keys"), ws.data_ptr(), ws.numel(), self._stream(logits)), "rows_fwd")
        return label, ce, class_count, info

    def sort_desc(self, keys, perm=None, ws=None):
        """keys int32 [S, M] holding uint32 bit patterns -> perm int32 [S, M]: descending (unsigned), ties in ascending index."""
        s, m = (int(x) for x in keys.shape)
        if perm is None:
            perm = torch.empty((s, m), dtype=torch.int32, device=keys.device)
        if ws is None:
            ws = torch.empty(max(self.sort_workspace_bytes(s, m), 4), dtype=torch.uint8, device=keys.device)
        self._ok(self.lib.ps_sort_desc(_dev(keys, torch.int32, "keys"), s, m, _dev(perm, torch.int32, "perm"), ws.data_ptr(),
                                       ws.numel(), self._stream(keys)), "sort_desc")
        return perm

    def lovasz_fwd(self, perm, label, keys, class_count, ws=None):
        """-> (loss_c fp32 [C], coef fp32 [N, C], lovasz fp32 [1], present int32 [1])."""
        c, n = (int(x) for x in keys.shape)
        check_classes(c)
        assert tuple(perm.shape) == (c, n) and tuple(label.shape) == (n,) and tuple(class_count.shape) == (c,)
        dev = keys.device
        if ws is None:
            ws = torch.empty(max(self.geometry(n, c)["lovasz_bytes"], 4), dtype=torch.uint8, device=dev)
        loss_c = torch.empty((c,), dtype=torch.float32, device=dev)
        coef = torch.empty((n, c), dtype=torch.float32, device=dev)
        lovasz = torch.empty((1,), dtype=torch.float32, device=dev)
        present = torch.empty((1,), dtype=torch.int32, device=dev)
        i32 = torch.int32
        self._ok(self.lib.ps_lovasz_fwd(_dev(perm, i32, "perm"), _dev(label, torch.uint8, "label"), _dev(keys, i32, "keys"),
                                        _dev(class_count, i32, "class_count"), n, c, loss_c.data_ptr(), coef.data_ptr(),
                                        lovasz.data_ptr(), present.data_ptr(), ws.data_ptr(), ws.numel(), self._stream(keys)),
                 "lovasz_fwd")
        return loss_c, coef, lovasz, present

    def loss_bwd(self, logits, label, coef, weights, ce, present, g):
        """-> dlogits fp32 [N, C].  g fp32 [2] = the incoming gradients of (ce, lovasz), on the device."""
        n, c = (int(x) for x in logits.shape)
        check_classes(c)
        assert tuple(coef.shape) == (n, c) and tuple(label.shape) == (n,) and tuple(g.shape) == (2,)
        dlogits = torch.empty_like(logits)
        f32 = torch.float32
        self._ok(self.lib.ps_loss_bwd(_dev(logits, f32, "logits"), _dev(label, torch.uint8, "label"), _dev(coef, f32, "coef"),
                                      _dev(weights, f32, "weights"), _dev(ce, f32, "ce"), _dev(present, torch.int32, "present"),
                                      _dev(g, f32, "g"), n, c, dlogits.data_ptr(), self._stream(logits)), "loss_bwd")
        return dlogits

    def forward(self, logits, coords, target, box, scale: int, weights, ws=None):
        """The three stages on one workspace -> a dict: label, ce [3], class_count, info [4], loss_c, coef, lovasz [1], present,
        and `keys` / `perm` as VIEWS of the workspace (valid until the next forward on this stream)."""
        n, c = (int(x) for x in logits.shape)
        check_classes(c)
        if n > PS_MAX_N:
            raise ValueError(f"semantic completion loss: {n} rows not served (at most {PS_MAX_N})")
        g = geometry(n, c)
        if ws is None:
            ws = self._workspace(g["workspace_bytes"], logits.device)
        keys, perm, ws_sort, ws_rows, ws_lov = self.parts(ws, n, c, g)
        label, ce, class_count, info = self.rows_fwd(logits, coords, target, box, scale, weights, keys, ws_rows)
        if n > 0:
            self.sort_desc(keys, perm, ws_sort)
        loss_c, coef, lovasz, present = self.lovasz_fwd(perm, label, keys, class_count, ws_lov)
        return {"label": label, "ce": ce, "class_count": class_count, "info": info, "loss_c": loss_c, "coef": coef,
                "lovasz": lovasz, "present": present, "keys": keys, "perm": perm}


def sem_lib() -> SemLib:
    """The process-wide binding of libpascohip.so's semantic completion loss kernels (a missing library is an error)."""
    return shared(SemLib)
