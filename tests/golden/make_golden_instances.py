"""Fixture for the instance-label generator, produced by the REFERENCE's own program.

Runs only in the build container (needs the reference checkout; never collected by pytest).  Each synthetic grid is
written as a SemanticKITTI voxel file pair into a temporary tree, the reference's `DummyDataset.__getitem__`
(label_gen/gen_instance_labels.py: lookup, raster scan, flood fill, size filter, renumbering) runs on it with an identity
lookup table, and the pickle it wrote is read back.  Stored: the input grid, the thing ids and the two grids the reference
produced - data only, nothing of the reference's source.

    python tests/golden/make_golden_instances.py
"""
import os
import pickle
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("PASCO_REFERENCE", "/root/reference")
sys.path.insert(0, REFERENCE)
try:
    import imageio  # noqa: F401
except ImportError:
    sys.modules["imageio"] = types.ModuleType("imageio")

from label_gen.gen_instance_labels import DummyDataset  # noqa: E402

THINGS = [1, 2, 3, 4, 5, 6, 7, 8]


def noise(rng, shape, p, hi=20):
    g = rng.integers(0, hi, shape).astype(np.uint8)
    g[rng.random(shape) > p] = 0
    g[rng.random(shape) < 0.05] = 255
    return g


def cars(rng, shape, n):
    """Boxes of 1..200 voxels of classes 0..19 and 255 on an empty grid, later boxes overwrite earlier ones."""
    g = np.zeros(shape, np.uint8)
    for _ in range(n):
        e = [int(rng.integers(1, 7)), int(rng.integers(1, 7)), int(rng.integers(1, 6))]
        o = [int(rng.integers(0, s - d + 1)) for s, d in zip(shape, e)]
        g[o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]] = 255 if rng.random() < 0.1 else rng.integers(0, 20)
    return g


def handmade():
    g = np.zeros((20, 18, 40), np.uint8)
    g[0:2, 0:2, 0:2] = 1                  # 8 voxels: kept
    g[2, 2, 2] = 1                        # touches the cube only through a corner: one component of 9
    g[5, 5, 5:12] = 2                     # a bar of exactly 7: dropped
    g[5, 9, 5:13] = 2                     # a bar of exactly 8: kept
    g[10:12, 0:4, 0] = 3                  # two classes face to face: two components
    g[12:14, 0:4, 0] = 4
    g[7:9, 7:9, 30:34] = 5                # 16 voxels across z = 32
    g[15, 10:17, 20] = 6                  # seven in a row, then one more reached only diagonally: 8, kept
    g[16, 17, 21] = 6
    g[19, 17, 39] = 7                     # a single voxel in the far corner: dropped
    g[18, 0:3, 36:39] = 8                 # 9 voxels
    g[0, 17, 39] = 255
    g[3:6, 12:15, 0:3] = 11               # not a thing
    return g


def cases():
    rng = np.random.default_rng(20240607)
    out = [("noise_25", noise(rng, (24, 20, 8), 0.25), THINGS), ("noise_50", noise(rng, (16, 16, 6), 0.5, 6), THINGS),
           ("noise_12", noise(rng, (30, 30, 4), 0.12, 3), THINGS), ("noise_80", noise(rng, (12, 12, 12), 0.8), THINGS),
           ("noise_tall", noise(rng, (10, 8, 35), 0.3, 5), THINGS), ("cars", cars(rng, (40, 40, 16), 120), THINGS),
           ("cars_order", cars(rng, (24, 24, 8), 60), [5, 2, 8, 1]), ("handmade", handmade(), THINGS),
           ("kitti360_things", cars(rng, (24, 24, 8), 60), [1, 2, 3, 4, 5, 6])]
    return out


def run_reference(grid, thing_ids, tmp, tag):
    ds = object.__new__(DummyDataset)
    ds.preprocess_root, ds.scale, ds.scene_size = tmp, 1, tuple(grid.shape)
    ds.thing_ids = list(thing_ids)
    ds.remap_lut = np.arange(256, dtype=np.int32)            # raw value = class: the lookup itself has its own test
    label, invalid, out = (os.path.join(tmp, f"{tag}.{ext}") for ext in ("label", "invalid", "pkl"))
    grid.astype(np.uint16).tofile(label)
    assert grid.size % 8 == 0
    np.zeros(grid.size // 8, np.uint8).tofile(invalid)
    ds.scans = [(tag, "00", label, invalid, out)]
    ds[0]
    with open(out, "rb") as f:
        d = pickle.load(f)
    return d["instance_labels"], d["semantic_labels"]


def main():
    arrays = {"names": np.array([c[0] for c in cases()])}
    with tempfile.TemporaryDirectory() as tmp:
        for name, grid, things in cases():
            t0 = time.time()
            ins, sem = run_reference(grid, things, tmp, name)
            assert ins.dtype == np.float64 and sem.dtype == np.float32 and ins.shape == grid.shape
            assert (ins == 0).sum() >= 8, "the reference's background corner must stay out of the fixture"
            print(f"{name}: grid {grid.shape} instances {int(ins.max())} unknown added {int((sem == 255).sum() - (grid == 255).sum())}"
                  f" ({time.time() - t0:.1f} s)")
            arrays.update({f"{name}_grid": grid, f"{name}_things": np.array(things, np.int32),
                           f"{name}_instance": ins.astype(np.int32), f"{name}_semantic": sem.astype(np.uint8)})
    np.savez_compressed(os.path.join(HERE, "instances_ref.npz"), **arrays)


if __name__ == "__main__":
    main()
