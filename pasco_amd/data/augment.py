"""The training augmentation's rigid-plus-scale transform (pasco/models/transform_utils.py:7-46), drawn from a numpy random
state in the reference's order, so that a seeded state gives the reference's T."""
from __future__ import annotations

import math

import numpy as np
import torch


def make_transformation(rot: float = 0.0, translation=(0.0, 0.0, 0.0), flip_dim=None, scale=1.0) -> torch.Tensor:
    """scale @ (rotation about z by `rot` degrees, then `translation` metres) @ flip, each factor rounded to fp32 before the
    product, as the reference builds it.  The reference asks scipy for the rotation of Euler xyz = (0, 0, rot); it is written out
    here through the unit quaternion, the way scipy forms it, so that the fp64 entries agree before the rounding to fp32 (equal
    to the reference on 200 seeded draws: tests/golden/make_golden_targets.py)."""
    flip = np.identity(4)
    if flip_dim is not None:
        flip[flip_dim, flip_dim] = -1
    half = math.radians(float(rot)) / 2      # the unit quaternion (0, 0, z, w)
    z, w = math.sin(half), math.cos(half)
    rigid = np.identity(4)
    rigid[:2, :2] = [[w * w - z * z, -2 * z * w], [2 * z * w, w * w - z * z]]
    rigid[:3, 3] = translation
    sc = np.identity(4)
    sc[[0, 1, 2], [0, 1, 2]] *= scale
    return torch.from_numpy(sc).float() @ torch.from_numpy(rigid).float() @ torch.from_numpy(flip).float()


def random_transformation(rng=np.random, max_angle=45, flip=True, scale_range=0.1, max_translation=(1.0, 1.0, 0.5)) -> torch.Tensor:
    """`rng`: a numpy.random.RandomState or the np.random module.  Draws, in this order: rand(3) translation, rand() angle,
    rand() flip (only when `flip`), rand(3) per-axis scale."""
    translation = (rng.rand(3) - 0.5) * np.asarray(max_translation, dtype=np.float64)
    rot = (rng.rand() - 0.5) * max_angle * 2
    flip_dim = 1 if (flip and rng.rand() > 0.5) else None
    scale = 1.0 + (rng.rand(3) - 0.5) * scale_range
    return make_transformation(rot=rot, translation=translation, flip_dim=flip_dim, scale=scale)
