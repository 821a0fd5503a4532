"""A perspective camera as the twelve fp32 numbers pv_render reads, and presets derived from the grid's extent.

The kernel does no trigonometry: the host works in fp64 and rounds once.  Pixel (i, j) (column, row; row 0 at the top) looks
along d = d0 + i*du + j*dv, which passes through the centre of that pixel on an image plane at distance 1."""
from __future__ import annotations

import math

import numpy as np

PRESETS = ("behind", "top", "oblique")


def camera(position, focal_point, view_up, view_angle_deg: float, width: int, height: int) -> np.ndarray:
    """-> fp32 [12]: origin, d0, du, dv.  `view_angle_deg` is the vertical field of view."""
    pos = np.asarray(position, np.float64)
    fwd = np.asarray(focal_point, np.float64) - pos
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(view_up, np.float64))
    if np.linalg.norm(right) < 1e-12:
        raise ValueError("view-up is parallel to the viewing direction")
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    half_h = math.tan(math.radians(view_angle_deg) / 2.0)
    px = 2.0 * half_h / height                      # size of a pixel on the plane at distance 1 (square pixels)
    du = right * px
    dv = -up * px
    d0 = fwd + du * (0.5 - width / 2.0) + dv * (0.5 - height / 2.0)
    return np.concatenate([pos, d0, du, dv]).astype(np.float32)


def preset(name: str, shape, width: int, height: int) -> np.ndarray:
    """Cameras placed from the grid's extent alone (x forward, y left, z up, in voxels):
      behind   behind the x = 0 face and above the grid, looking forward and down at its middle
      top      straight down on the centre, x pointing up in the image, far enough to see the longer side
      oblique  from the corner (0, 0), above, looking across the diagonal"""
    X, Y, Z = (float(v) for v in shape)
    centre = np.array([X / 2, Y / 2, Z / 2])
    span = max(X, Y)
    if name == "behind":
        return camera([-0.55 * span, Y / 2, Z + 0.45 * span], [0.45 * X, Y / 2, 0.0], [0, 0, 1], 40.0, width, height)
    if name == "top":
        dist = 0.5 * span / math.tan(math.radians(20.0)) * 1.08
        return camera([X / 2, Y / 2, Z + dist], centre, [1, 0, 0], 40.0, width, height)
    if name == "oblique":
        return camera([-0.35 * span, -0.35 * span, Z + 0.5 * span], [0.5 * X, 0.5 * Y, 0.0], [0, 0, 1], 40.0, width, height)
    raise ValueError(f"camera {name!r}: one of {', '.join(PRESETS)}")
