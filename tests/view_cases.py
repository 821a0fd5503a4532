"""Inputs shared by tests/test_view_cpu.py and tests/test_hip_view.py, and the references the CPU tests hold the host
restatement (pasco_amd/viz/host.py) to.  The references are literal: one cell, one window, one ray-voxel pair at a time."""
import numpy as np

FULL = (256, 256, 32)
NEAR_TIE = 1e-5


# ---- scenes -----------------------------------------------------------------------------------------------------------
def blob_labels(seed, shape=FULL, n=700, classes=20, unknown=0.05):
    """Seeded boxes of classes 0 .. classes-1 (and a few of 255) on a ground sheet of class 9."""
    rng = np.random.default_rng(seed)
    g = np.zeros(shape, np.uint8)
    g[:, :, : max(1, shape[2] // 8)] = 9
    for _ in range(n):
        e = [int(rng.integers(1, 12)), int(rng.integers(1, 8)), int(rng.integers(1, 7))]
        o = [int(rng.integers(0, max(1, s - d + 1))) for s, d in zip(shape, e)]
        g[o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]] = 255 if rng.random() < unknown else rng.integers(0, classes)
    return g


def noise_labels(seed, shape, p=0.5, classes=20, unknown=0.1):
    rng = np.random.default_rng(seed)
    g = (rng.integers(0, classes, shape) * (rng.random(shape) < p)).astype(np.uint8)
    g[rng.random(shape) < unknown] = 255
    return g


def sparse_colour(seed, shape, p=0.06, top=20):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, top, shape) * (rng.random(shape) < p)).astype(np.uint32)


def conf_grid(seed, shape, sentinel=0.3):
    """fp32 confidences in [0, 1) with a share of voxels at the sentinel 255."""
    rng = np.random.default_rng(seed)
    g = rng.random(shape, dtype=np.float32)
    g[rng.random(shape) < sentinel] = 255.0
    return g


def synthetic_record(shape=(32, 32, 8), seed=0):
    """A saved frame as `viz.outputs.frame_record` makes it: blobs, five segments (four things, the road as stuff)."""
    from pasco_amd.viz import frame_record
    rng = np.random.default_rng(seed)
    sem = blob_labels(seed, shape, n=30, unknown=0.0)
    gt = blob_labels(seed + 1, shape, n=30)
    pan = np.zeros(shape, np.int32)
    infos = []
    for i, c in enumerate((1, 1, 4, 9, 5), start=1):
        m = sem == c if c == 9 else (sem == c) & (rng.random(shape) < 0.5) & (pan == 0)
        pan[m] = i
        infos.append({"id": i, "isthing": c < 9, "category_id": c, "confidence": float(np.float32(0.3 + 0.1 * i))})
    return frame_record(sem, pan, infos, rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32),
                            rng.random((50, 3), dtype=np.float32), pan, [{"id": 1, "isthing": True, "category_id": 1}], gt,
                            (pan * (sem < 9)).astype(np.uint8))


# ---- references ---------------------------------------------------------------------------------------------------------
def pool_reference(grid, k):
    """The rule of pv_majority_pool with `np.unique` per cell; a label in 32 .. 254 counts as 255 and raises the status."""
    X, Y, Z = (s // k for s in grid.shape)
    out = np.zeros((X, Y, Z), np.uint8)
    status = 0
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                cell = grid[x * k:(x + 1) * k, y * k:(y + 1) * k, z * k:(z + 1) * k].astype(np.int64).ravel()
                if ((cell >= 32) & (cell != 255)).any():
                    status = 1
                    cell = np.where(cell >= 32, 255, cell)
                unique, counts = np.unique(cell, return_counts=True)
                real = (unique != 0) & (unique != 255)
                if real.any():
                    out[x, y, z] = unique[real][np.argmax(counts[real])]       # sorted, first maximum: smallest label
                else:
                    out[x, y, z] = 0 if (unique == 0).any() else 255
    return out, status


def filter_reference(grid, op, mask=None):
    X, Y, Z = grid.shape
    out = np.zeros(grid.shape, np.float32)
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                vals = []
                for xx in range(max(x - 1, 0), min(x + 2, X)):
                    for yy in range(max(y - 1, 0), min(y + 2, Y)):
                        for zz in range(max(z - 1, 0), min(z + 2, Z)):
                            if grid[xx, yy, zz] != np.float32(255.0) and (mask is None or mask[xx, yy, zz] != 0):
                                vals.append(np.float32(grid[xx, yy, zz]))
                if not vals:
                    out[x, y, z] = 255.0
                elif op == "max":
                    out[x, y, z] = max(vals)
                elif op == "avg":
                    total = np.float32(0.0)
                    for v in vals:
                        total = np.float32(total + v)
                    out[x, y, z] = np.float32(total / np.float32(len(vals)))
                else:
                    s = sorted(vals)
                    n = len(s)
                    out[x, y, z] = s[n // 2] if n % 2 else np.float32(np.float32(s[n // 2 - 1] + s[n // 2]) * np.float32(0.5))
    return out


def brute_force(colour, cam, W, H):
    """fp64 slab intersection of every ray with every occupied voxel; the nearest hit wins.
    -> (hit int32 [H, W], face int32 [H, W] (6 = the origin lies inside the voxel, 255 = miss), near_tie bool [H, W]).
    A pixel is a near-tie when, relative to the t values compared (NEAR_TIE of the largest magnitude, at least 1):
    the two nearest candidates are that close in t; or the winner's two latest slab entries are that close (the ray enters
    next to an edge of the voxel, so the face is ambiguous); or some occupied voxel is grazed (its entry and exit that close:
    the ray passes next to one of its edges and hit / miss could flip)."""
    cam = np.asarray(cam, np.float32).astype(np.float64)
    o = cam[0:3]
    vox = np.argwhere(colour != 0).astype(np.float64)                # [V, 3]
    site = np.flatnonzero(colour.reshape(-1) != 0)
    hit = np.full((H, W), -1, np.int32)
    face = np.full((H, W), 255, np.int32)
    tie = np.zeros((H, W), bool)
    if vox.shape[0] == 0:
        return hit, face, tie
    for j in range(H):
        for i in range(W):
            d = cam[3:6] + i * cam[6:9] + j * cam[9:12]
            tn = np.full(vox.shape, -np.inf)
            tf = np.full(vox.shape, np.inf)
            ok = np.ones(vox.shape[0], bool)
            for a in range(3):
                if d[a] == 0.0:
                    ok &= (o[a] >= vox[:, a]) & (o[a] < vox[:, a] + 1)
                else:
                    t_lo, t_hi = (vox[:, a] - o[a]) / d[a], (vox[:, a] + 1 - o[a]) / d[a]
                    tn[:, a], tf[:, a] = np.minimum(t_lo, t_hi), np.maximum(t_lo, t_hi)
            near, far = tn.max(1), tf.min(1)
            scale = np.maximum(1.0, np.maximum(np.abs(near), np.abs(far)))
            ahead = far >= 0
            tie[j, i] = bool((ok & ahead & (np.abs(far - near) < NEAR_TIE * scale)).any())
            cand = np.flatnonzero(ok & ahead & (near <= far))
            if cand.size == 0:
                continue
            t = np.maximum(near[cand], 0.0)
            order = np.argsort(t, kind="stable")
            w = cand[order[0]]
            hit[j, i] = site[w]
            if near[w] < 0:
                face[j, i] = 6
            else:
                a = int(np.argmax(tn[w]))
                face[j, i] = 2 * a + (1 if d[a] < 0 else 0)
                two = np.sort(tn[w])[-2:]
                if two[1] - two[0] < NEAR_TIE * max(1.0, abs(two[1])):
                    tie[j, i] = True
            if cand.size > 1 and t[order[1]] - t[order[0]] < NEAR_TIE * max(1.0, abs(t[order[1]])):
                tie[j, i] = True
    return hit, face, tie
