"""Palettes of the renderer (uint8 [n, 3] RGB, entry 0 unused because colour index 0 means empty).

Class colours come from the dataset yaml: `learning_map_inv` maps a class to a raw label, `color_map` gives that label's
colour as BGR.  The instance colours and the uncertainty ramp are formulas of this project:

  instance r (0-based): hue = frac(r * 0.61803398875) (golden-ratio steps: neighbours in the table are far apart on the colour
      wheel), saturation 0.55 + 0.15 * (r mod 3), value 0.95 - 0.12 * (floor(r / 3) mod 3), HSV -> RGB.
  ramp level q in 0 .. 255, u = q / 255: piecewise linear through dark blue, cyan, yellow, red at u = 0, 1/3, 2/3, 1.
"""
from __future__ import annotations

import colorsys

import numpy as np

from .host import INSTANCE_BASE, MAX_SEGMENTS, RAMP_BASE

RAMP_KNOTS = ((0.0, (24, 32, 120)), (1.0 / 3.0, (40, 200, 220)), (2.0 / 3.0, (250, 220, 50)), (1.0, (200, 24, 24)))


def class_colours(config_path: str, n_classes: int = INSTANCE_BASE) -> np.ndarray:
    """uint8 [n_classes, 3]: RGB of class c at row c (classes the yaml does not name stay mid grey)."""
    import yaml
    with open(config_path) as f:
        cfg = yaml.safe_load(f)
    out = np.full((n_classes, 3), 128, np.uint8)
    for cls, raw in cfg["learning_map_inv"].items():
        if 0 <= int(cls) < n_classes and raw in cfg["color_map"]:
            b, g, r = cfg["color_map"][raw]
            out[int(cls)] = (r, g, b)
    return out


def instance_colours(n: int = MAX_SEGMENTS) -> np.ndarray:
    out = np.empty((n, 3), np.uint8)
    for r in range(n):
        h = (r * 0.61803398875) % 1.0
        s = 0.55 + 0.15 * (r % 3)
        v = 0.95 - 0.12 * ((r // 3) % 3)
        out[r] = [int(round(255 * c)) for c in colorsys.hsv_to_rgb(h, s, v)]
    return out


def label_palette(config_path: str) -> np.ndarray:
    """The palette of the semantic, panoptic and mask views: classes at 0 .. 31, instances from INSTANCE_BASE on."""
    return np.concatenate([class_colours(config_path, INSTANCE_BASE), instance_colours(MAX_SEGMENTS)])


def ramp_palette() -> np.ndarray:
    """The palette of the two confidence views: level q at RAMP_BASE + q."""
    out = np.zeros((RAMP_BASE + 256, 3), np.uint8)
    for q in range(256):
        u = q / 255.0
        for (u0, c0), (u1, c1) in zip(RAMP_KNOTS[:-1], RAMP_KNOTS[1:]):
            if u <= u1:
                w = (u - u0) / (u1 - u0)
                out[RAMP_BASE + q] = [int(round(a + w * (b - a))) for a, b in zip(c0, c1)]
                break
    return out
