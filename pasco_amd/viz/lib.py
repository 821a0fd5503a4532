"""ctypes binding of include/pasco_view.h (the `pv_*` entry points of libpascohip.so): rendering on the device.

Kept apart from `me.backend` like `data.label_lib`: the CPU oracle binds `me.backend._SIGNATURES` and has no view kernels.
Every method takes device tensors and enqueues on the caller's current stream; nothing synchronises."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from .._clib import FamilyLib, dev_ptr as _dev, shared
from .host import OPS, VIEWS

PV_ABI_VERSION = 1       # include/pasco_view.h PV_ABI_VERSION this binding was written against

_vp, _i64, _i32, _u32, _f32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_float
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "majority_pool": [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "window_filter": [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "compose": [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp],
    "brick_words": [_i32, _i32, _i32],
    "bricks": [_vp, _i32, _i32, _i32, _vp, _vp],
    "render": [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _u32, _i32, _vp, _vp, _vp, _vp, _vp],
    "downsample": [_vp, _i32, _i32, _i32, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p, "brick_words": _i64}


class ViewLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("pv_", PV_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def majority_pool(self, grid: torch.Tensor, k: int, out: Optional[torch.Tensor] = None,
                      status: Optional[torch.Tensor] = None):
        """uint8 [X, Y, Z] -> (uint8 [X//k, Y//k, Z//k], status int32 [1])."""
        X, Y, Z = (int(v) for v in grid.shape)
        if out is None:
            out = torch.empty((X // k, Y // k, Z // k), dtype=torch.uint8, device=grid.device)
        if status is None:
            status = torch.zeros(1, dtype=torch.int32, device=grid.device)
        assert out.numel() >= (X // k) * (Y // k) * (Z // k)
        self._ok(self.lib.pv_majority_pool(_dev(grid, torch.uint8, "grid"), X, Y, Z, int(k), _dev(out, torch.uint8, "out"),
                                           _dev(status, torch.int32, "status"), self._stream(grid)), "majority_pool")
        return out, status

    def window_filter(self, grid: torch.Tensor, op: str, mask: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fp32 [X, Y, Z] (and a uint8 mask of the same shape, or None) -> fp32 [X, Y, Z]."""
        X, Y, Z = (int(v) for v in grid.shape)
        if out is None:
            out = torch.empty_like(grid)
        assert out.numel() >= grid.numel() and (mask is None or mask.shape == grid.shape)
        self._ok(self.lib.pv_window_filter(_dev(grid, torch.float32, "grid"),
                                           None if mask is None else _dev(mask, torch.uint8, "mask"), X, Y, Z, OPS[op],
                                           _dev(out, torch.float32, "out"), self._stream(grid)), "window_filter")
        return out

    def compose(self, view: str, shape: Sequence[int], panoptic: Optional[torch.Tensor] = None,
                seg: Optional[torch.Tensor] = None, sem: Optional[torch.Tensor] = None, conf: Optional[torch.Tensor] = None,
                vmin: float = 0.0, vmax: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> int32 [X, Y, Z] holding the uint32 colour indices.  seg: int32 [4, n_seg] on the device, or None."""
        X, Y, Z = (int(v) for v in shape)
        ref = next(t for t in (panoptic, sem, conf) if t is not None)
        if out is None:
            out = torch.empty((X, Y, Z), dtype=torch.int32, device=ref.device)
        n_seg = 0 if seg is None else int(seg.shape[1])
        for t in (panoptic, sem, conf):
            assert t is None or t.numel() == X * Y * Z
        assert out.numel() >= X * Y * Z and (seg is None or (seg.dim() == 2 and seg.shape[0] == 4))
        self._ok(self.lib.pv_compose(None if panoptic is None else _dev(panoptic, torch.int32, "panoptic"),
                                     None if seg is None or n_seg == 0 else _dev(seg, torch.int32, "seg"), n_seg,
                                     None if sem is None else _dev(sem, torch.uint8, "sem"),
                                     None if conf is None else _dev(conf, torch.float32, "conf"), X, Y, Z, VIEWS[view],
                                     float(vmin), float(vmax), _dev(out, torch.int32, "out"), self._stream(ref)), "compose")
        return out

    def brick_words(self, shape: Sequence[int]) -> int:
        n = int(self.lib.pv_brick_words(*(int(v) for v in shape)))
        if n < 0:
            raise ValueError(f"pv_bricks: grid {tuple(shape)} is not supported")
        return n

    def bricks(self, colour: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int32 [X, Y, Z] colour indices -> int32 [brick_words] occupancy bits."""
        X, Y, Z = (int(v) for v in colour.shape)
        if out is None:
            out = torch.empty(self.brick_words(colour.shape), dtype=torch.int32, device=colour.device)
        assert out.numel() >= self.brick_words(colour.shape)
        self._ok(self.lib.pv_bricks(_dev(colour, torch.int32, "colour"), X, Y, Z, _dev(out, torch.int32, "bits"),
                                    self._stream(colour)), "bricks")
        return out

    def render(self, colour: torch.Tensor, bits: torch.Tensor, cam: torch.Tensor, W: int, H: int, palette: torch.Tensor,
               factors=(256, 256, 256), background=(255, 255, 255), step_cap: int = 0, hit=None, face=None, rgb=None,
               status=None):
        """-> (hit int32 [H, W], face uint8 [H, W], rgb uint8 [H, W, 3], status int32 [1]), all on the device."""
        X, Y, Z = (int(v) for v in colour.shape)
        dev = colour.device
        hit = torch.empty((H, W), dtype=torch.int32, device=dev) if hit is None else hit
        face = torch.empty((H, W), dtype=torch.uint8, device=dev) if face is None else face
        rgb = torch.empty((H, W, 3), dtype=torch.uint8, device=dev) if rgb is None else rgb
        status = torch.zeros(1, dtype=torch.int32, device=dev) if status is None else status
        assert cam.numel() == 12 and bits.numel() >= self.brick_words(colour.shape) and palette.dim() == 2
        assert palette.shape[1] == 3 and hit.numel() >= W * H and face.numel() >= W * H and rgb.numel() >= 3 * W * H
        bg = int(background[0]) | int(background[1]) << 8 | int(background[2]) << 16
        self._ok(self.lib.pv_render(_dev(colour, torch.int32, "colour"), _dev(bits, torch.int32, "bits"), X, Y, Z,
                                    _dev(cam, torch.float32, "cam"), int(W), int(H), _dev(palette, torch.uint8, "palette"),
                                    int(palette.shape[0]), int(factors[0]), int(factors[1]), int(factors[2]), bg,
                                    int(step_cap), _dev(hit, torch.int32, "hit"), _dev(face, torch.uint8, "face"),
                                    _dev(rgb, torch.uint8, "rgb"), _dev(status, torch.int32, "status"), self._stream(colour)),
                 "render")
        return hit, face, rgb, status

    def downsample(self, img: torch.Tensor, s: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """uint8 [H*s, W*s, 3] -> uint8 [H, W, 3]."""
        if img.shape[0] % s or img.shape[1] % s:
            raise ValueError(f"pv_downsample: image {tuple(img.shape)} is no multiple of {s}")
        H, W = int(img.shape[0]) // s, int(img.shape[1]) // s
        if out is None:
            out = torch.empty((H, W, 3), dtype=torch.uint8, device=img.device)
        assert out.numel() >= 3 * W * H
        self._ok(self.lib.pv_downsample(_dev(img, torch.uint8, "img"), W, H, int(s), _dev(out, torch.uint8, "out"),
                                        self._stream(img)), "downsample")
        return out


def view_lib() -> ViewLib:
    """The process-wide binding of libpascohip.so's view kernels (a missing library is an error)."""
    return shared(ViewLib)
