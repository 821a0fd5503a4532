"""Case table of the point-feature stage (pasco_amd/waffle), shared by the CPU leg (tests/test_waffle_cpu.py: the restatement
`host.py` against independent references) and the GPU leg (tests/test_hip_waffle.py: the pw_* kernels against the
restatement and against fp64).  Both legs hand an `ops` object with the same methods (`HostOps` here, `DeviceOps` in the GPU
leg) to the `check_*` functions below.

Float bound.  Error of one output tensor: max|got - ref64| / max(1, max|ref64|).  REF_ERROR is the largest error of the
reference's own recorded fp32 results against tests/waffle_ref64.py in float64 over both golden nets and both golden scans
(measured: 8.5303e-7, the logits of the C = 256 net on the kitti_mini scan); BOUND is twice that, the rule DESIGN.md 4g uses.
test_waffle_cpu.py::test_bound_is_twice_the_reference_error recomputes the measurement and holds the constant to it."""
import functools
import os

import numpy as np
import torch

from pasco_amd.waffle import host, prep

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF_ERROR = 8.531e-7
BOUND = 2 * REF_ERROR
NETS = ("c256", "c32")
SCANS = ("synth", "mini")
SIZES = (17, 18, 63, 64, 65, 700, 5000)
FOV = np.array([[-50, -50, -3], [50, 50, 2]])
K = 16


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gold(name="waffle.npz"):
    z = np.load(os.path.join(GOLD, name))
    return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def state(net: str):
    """The golden net's state dict under the reference's key names, float32 tensors."""
    files = {"c256": ("waffle_mini_c256_embed.npz", "waffle_mini_c256_mix.npz"), "c32": ("waffle_mini_c32.npz",)}[net]
    st = {}
    for f in files:
        z = np.load(os.path.join(GOLD, f))
        st.update({k: torch.from_numpy(z[k].astype(np.float32) if z[k].dtype == np.float16 else z[k]) for k in z.files})
    return st


def config_path(net: str) -> str:
    return os.path.join(GOLD, f"waffle_{net}.yaml")


@functools.lru_cache(maxsize=None)
def settings(net: str):
    return prep.load_config(config_path(net))


def write_ckpt(path: str, net: str, module_prefix: bool = False) -> str:
    """A checkpoint file in the reference's format: {"net": state dict}."""
    st = state(net)
    torch.save({"net": {("module." + k if module_prefix else k): v for k, v in st.items()}}, path)
    return path


def mini_scan() -> np.ndarray:
    return np.fromfile(os.path.join(GOLD, "kitti_mini", "dataset", "sequences", "08", "velodyne", "000005.bin"),
                       dtype=np.float32).reshape(-1, 4)


def scan(name: str) -> np.ndarray:
    return gold()["scan_synth"] if name == "synth" else mini_scan()


def recorded(net: str, scan_name: str):
    """The reference's fp32 (embedding, tokens, logits) and the row step they were stored with."""
    src, step = (gold("waffle_c256.npz"), int(gold("waffle_c256.npz")["row_step"])) if net == "c256" else (gold(), 1)
    return [src[f"{scan_name}_{net}_{k}"] for k in ("embedding", "tokens", "logits")], step


@functools.lru_cache(maxsize=None)
def ref64(net: str, scan_name: str):
    """fp64 (embedding, tokens, logits) of a golden net on a golden scan's reference preparation.  Computed once, never
    written."""
    import waffle_ref64 as R
    g = gold()
    out = R.forward(state(net), settings(net)["grids"], g[f"{scan_name}_pc"][:, 3:], g[f"{scan_name}_{net}_cell_ind"],
                    g[f"{scan_name}_neigh"][1:].T, torch.float64)
    out = [t.numpy() for t in out]
    for a in out:
        a.setflags(write=False)
    return out


def err(got, ref) -> float:
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())) if ref.size else 0.0


def within_bound(got, ref, what):
    e = err(got, ref)
    print(f"{what}: error {e:.3e} (bound {BOUND:.3e})")
    assert e <= BOUND, f"{what}: error {e:.3e} > bound {BOUND:.3e}"


# ---- the restatement as an `ops` object ---------------------------------------------------------------------------------------
class HostOps:
    """Every method takes and returns numpy arrays; a status is returned beside the result where the entry point has one."""
    name = "host"
    voxel_keys = staticmethod(host.voxel_keys)
    cell_index = staticmethod(host.cell_index)
    grid_cells = staticmethod(host.grid_cells)
    knn = staticmethod(host.knn)
    nearest = staticmethod(host.nearest)
    dwconv3x3 = staticmethod(host.dwconv3x3)
    neigh_rows = staticmethod(host.neigh_rows)

    @staticmethod
    def cells_build(cell, ncell, order=None):
        return host.cells_build(cell, ncell, order)

    @staticmethod
    def flatten(tokens, scale, shift, start, order, ncell):
        return host.flatten(tokens, scale, shift, start, order, ncell), 0

    @staticmethod
    def inflate(tokens, scale, grid, cell):
        return host.inflate(tokens, scale, grid, cell), 0

    @staticmethod
    def group_max(rows, np_, k, ld_out):
        return host.group_max(rows, np_, k)


# ---- decisions ------------------------------------------------------------------------------------------------------------
def cloud(n: int, seed: int = 0, box=(10.0, 10.0, 3.0)) -> np.ndarray:
    rng = np.random.default_rng((seed, n))
    return ((rng.random((n, 3)) - 0.5) * np.array(box)).astype(np.float32)


def voxel_clouds():
    out = {f"n{n}": cloud(n, 1, (4.0, 4.0, 1.0)) for n in SIZES}
    out["one voxel"] = (np.float32(3.0) + cloud(40, 2, (0.05, 0.05, 0.05))).astype(np.float32)
    gx, gy, gz = np.meshgrid(np.arange(6), np.arange(5), np.arange(4), indexing="ij")
    lattice = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1) * 0.25 + 0.05
    out["one point per voxel"] = lattice[np.random.default_rng(3).permutation(lattice.shape[0])].astype(np.float32)
    return out


def check_voxel(ops):
    for name, xyz in voxel_clouds().items():
        pc = np.concatenate([xyz, np.arange(xyz.shape[0], dtype=np.float32)[:, None]], 1)
        shift = pc[:, :3] - pc[:, :3].min(0, keepdims=True)
        _, exp = np.unique((shift / 0.1).astype("int"), return_index=True, axis=0)       # the reference's Voxelize, verbatim maths
        key, st = ops.voxel_keys(pc, pc[:, :3].min(0), 0.1)
        assert st == 0, name
        got = host.first_of_keys(key)
        assert np.array_equal(got, exp), name
        if name == "one voxel":
            assert got.tolist() == [0]
        if name == "one point per voxel":
            assert got.shape[0] == xyz.shape[0]
    _, st = ops.voxel_keys(np.array([[0, 0, 0], [3e5, 0, 0]], np.float32), np.zeros(3, np.float32), 0.1)
    assert st == host.STATUS_KEY_RANGE


def crop_points():
    """Every bound, the bound moved by eps, and the fp32 neighbours of both."""
    rows = []
    for a in range(3):
        for side, sign in ((0, 1.0), (1, -1.0)):
            edge = np.float32(FOV[side][a] + sign * prep.EPS)
            for v in (np.float32(FOV[side][a]), edge, np.nextafter(edge, np.float32(1e9)), np.nextafter(edge, np.float32(-1e9))):
                p = np.zeros(3, np.float32)
                p[a] = v
                rows.append(p)
    return np.stack(rows)


def check_crop(mask_fn):
    pc = crop_points()
    exp, fov = None, FOV.tolist()                                        # Python numbers, as the yaml gives them to Crop
    for i in range(3):                                                   # the reference's Crop, verbatim maths
        t = (pc[:, i] > fov[0][i] + prep.EPS) & (pc[:, i] < fov[1][i] - prep.EPS)
        exp = t if exp is None else exp & t
    got = mask_fn(pc)
    assert np.array_equal(got, exp) and 0 < exp.sum() < exp.size


def grid_cases():
    """(name, dims, shape) with the published geometry and two narrow grids."""
    return [("250x250 z", (0, 1), (250, 250)), ("250x12 y", (0, 2), (250, 12)), ("250x12 x", (1, 2), (250, 12)),
            ("10x3 y", (0, 2), (10, 3)), ("10x10 z", (0, 1), (10, 10))]


def cell_points(n=700, seed=5):
    rng = np.random.default_rng(seed)
    pc = np.stack([rng.uniform(-49.99, 49.99, n), rng.uniform(-49.99, 49.99, n), rng.uniform(-2.99, 1.99, n)], 1).astype(np.float32)
    inside_hi = np.float32(FOV[1] - prep.EPS)
    inside_lo = np.float32(FOV[0] + prep.EPS)
    pc[0] = np.nextafter(inside_hi, np.float32(-1e9))        # the last row and the last column of every grid
    pc[1] = np.nextafter(inside_lo, np.float32(1e9))         # the first ones
    pc[2] = [np.nextafter(inside_hi[0], np.float32(-1e9)), pc[1, 1], 0.0]
    pc[3:70] = np.float32([10.1, -20.1, 0.5]) + rng.uniform(0, 0.05, (67, 3)).astype(np.float32)    # one cell with 67 points
    return pc


def geometry(dims, shape):
    res = (FOV[1, dims] - FOV[0, dims]) / np.array(shape)
    return [float(v) for v in FOV[0, dims]], [float(v) for v in res]


def check_cells(ops):
    pc = cell_points()
    for name, dims, shape in grid_cases():
        dims = list(dims)
        res = (FOV[1, dims] - FOV[0, dims]) / np.array(shape)[None]       # get_occupied_2d_cells, verbatim maths
        quant = ((pc[:, dims] - FOV[0, dims]) / res).astype("int")
        exp = quant[:, 0] * shape[1] + quant[:, 1]
        lo, r = geometry(dims, shape)
        cell, st = ops.cell_index(pc, dims, lo, r, shape)
        assert st == 0 and np.array_equal(cell, exp), name
        assert cell[0] == shape[0] * shape[1] - 1 and cell[1] == 0, name
        start, order, st = ops.cells_build(cell, shape[0] * shape[1])
        assert st == 0 and start[0] == 0 and start[-1] == pc.shape[0], name
        for c in np.unique(np.concatenate([cell, [0, shape[0] * shape[1] - 1]])):
            assert np.array_equal(order[start[c]:start[c + 1]], np.nonzero(cell == c)[0]), (name, c)
        assert (np.diff(start) >= 0).all() and np.diff(start).max() >= 67, name
    off = pc.copy()
    off[5, 0] = 50.0
    lo, r = geometry([0, 1], (250, 250))
    assert ops.cell_index(off, [0, 1], lo, r, (250, 250))[1] == host.STATUS_OFF_GRID         # refused, not clamped
    start, order, st = ops.cells_build(np.zeros(0, np.int32), 30)                             # an empty grid
    assert st == 0 and start.shape == (31,) and not start.any() and order.shape == (0,)
    cell = np.array([2, 0, 2, 1], np.int32)
    assert ops.cells_build(cell, 3, np.array([1, 3, 2, 0], np.int32))[2] == host.STATUS_ORDER  # sorted by cell, not by index


def search_cases():
    """name -> (points fp32 [n, 3], cell edge h)."""
    out = {f"n{n}": (cloud(n, 7), 1.0) for n in SIZES}
    rng = np.random.default_rng(8)
    dense = cloud(300, 9)
    dense[:120] = np.float32([1.2, 1.3, 0.4]) + (rng.random((120, 3)) * 0.2).astype(np.float32)
    out["cluster denser than a cell"] = (dense, 1.0)
    lone = cloud(200, 10, (4.0, 4.0, 2.0))
    lone[0] = [40.0, -35.0, 6.0]
    out["isolated point, many rings"] = (lone, 0.5)
    g = np.arange(-3, 4, dtype=np.float32)
    mx, my, mz = np.meshgrid(g, g, g[2:5], indexing="ij")
    lattice = np.stack([mx.ravel(), my.ravel(), mz.ravel()], 1).astype(np.float32)
    out["mirrored lattice (ties)"] = (lattice[np.random.default_rng(11).permutation(lattice.shape[0])], 1.5)
    out["flat sheet"] = (np.concatenate([cloud(400, 12, (30.0, 30.0, 0.0))[:, :2], np.zeros((400, 1), np.float32)], 1), 1.0)
    return out


def far_queries(xyz):
    lo, hi = xyz.min(0), xyz.max(0)
    mid = (lo + hi) / 2
    q = [mid]
    for a in range(3):
        for far in (5.0, 300.0):
            for sign in (-1, 1):
                p = mid.copy()
                p[a] = (lo[a] - far) if sign < 0 else (hi[a] + far)
                q.append(p)
    q.append(lo - 200.0)
    q.append(hi + 200.0)
    q.extend(xyz[:5] + np.float32(0.01))
    return np.stack(q).astype(np.float32)


def build_search(ops, xyz, h):
    g = host.SearchGrid.around(xyz.min(0), xyz.max(0), h)
    cell, st = ops.grid_cells(xyz, g)
    assert st == 0
    start, order, st = ops.cells_build(cell, g.ncell)
    assert st == 0
    return g, start, order


def check_search(ops, names=None):
    for name, (xyz, h) in search_cases().items():
        if names is not None and name not in names:
            continue
        g, start, order = build_search(ops, xyz, h)
        got = ops.knn(xyz, start, order, g, K)
        assert np.array_equal(got, host.knn_brute(xyz, xyz, K, True)), name
        q = far_queries(xyz)
        near = ops.nearest(xyz, start, order, g, q)
        assert np.array_equal(near, host.knn_brute(xyz, q, 1, False)[:, 0]), name
        if name.startswith("mirrored"):
            centre = int(np.nonzero((xyz == 0).all(1))[0][0])
            six = sorted(int(i) for i in np.nonzero(np.abs(xyz).sum(1) == 1)[0])
            assert got[centre, :6].tolist() == six                      # six points at d2 = 1: ascending index
    xyz, h = search_cases()["n700"]
    g, _, _ = build_search(ops, xyz, h)
    outside = xyz.copy()
    outside[3, 1] += 100.0
    assert ops.grid_cells(outside, g)[1] == host.STATUS_OFF_GRID


# ---- float kernels: inputs and fp64 references ----------------------------------------------------------------------------------
def tokens_case(n, C, seed):
    rng = np.random.default_rng((seed, n, C))
    return (rng.standard_normal((n, C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32),
            rng.standard_normal(C).astype(np.float32) * np.float32(0.3))


def flatten_cases():
    """(name, n, C, H, W): cells with more than 64 points, empty cells, W = 3 and 12, C below and above a wave, and a C that
    is no multiple of 4 (the kernels then take one channel per thread instead of four)."""
    return [("17 points 10x3", 17, 32, 10, 3), ("700 points 4x3, > 64 per cell", 700, 32, 4, 3),
            ("700 points 250x12", 700, 256, 250, 12), ("65 points 1x1", 65, 8, 1, 1), ("no point", 0, 32, 10, 3),
            ("63 points 10x3, C = 6: one channel per thread", 63, 6, 10, 3)]


def check_flatten_inflate(ops, bitwise_to_host=False):
    for name, n, C, H, W in flatten_cases():
        tok, sc, sh = tokens_case(n, C, 21)
        cell = np.random.default_rng((22, n)).integers(0, H * W, n).astype(np.int32)
        if n >= 700 and H * W > 100:
            cell[:80] = H * W - 1                                       # 80 points in the last cell
        start, order, _ = host.cells_build(cell, H * W)
        grid, st = ops.flatten(tok, sc, sh, start, order, H * W)
        assert st == 0 and grid.shape == (H * W, C), name
        t64 = tok.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)
        cnt = np.bincount(cell, minlength=H * W).astype(np.float64)
        ref = np.zeros((H * W, C))
        np.add.at(ref, cell, t64)
        ref = ref / (cnt + 1e-6)[:, None]
        within_bound(grid, ref, f"{ops.name} flatten {name}")
        assert not grid[cnt == 0].any(), name
        if bitwise_to_host:
            assert np.array_equal(grid.view(np.int32), host.flatten(tok, sc, sh, start, order, H * W).view(np.int32)), name
        if n:
            out, st = ops.inflate(tok, sc, grid, cell)
            within_bound(out, tok.astype(np.float64) + sc.astype(np.float64) * grid.astype(np.float64)[cell], f"{ops.name} inflate {name}")
            assert st == 0
            if bitwise_to_host:
                assert np.array_equal(out.view(np.int32), host.inflate(tok, sc, grid, cell).view(np.int32)), name


def dwconv_cases():
    return [(1, 1, 8), (1, 12, 8), (5, 3, 32), (3, 12, 32), (10, 10, 32), (250, 12, 256), (31, 12, 72), (5, 3, 6), (7, 12, 1)]


def dwconv64(g, H, W, w, b, relu):
    C = g.shape[-1]
    x = torch.from_numpy(g.reshape(H, W, C).astype(np.float64)).permute(2, 0, 1)[None]
    wt = torch.from_numpy(w.astype(np.float64)).t().reshape(C, 1, 3, 3)
    y = torch.nn.functional.conv2d(x, wt, torch.from_numpy(b.astype(np.float64)), padding=1, groups=C)
    y = torch.relu(y) if relu else y
    return y[0].permute(1, 2, 0).reshape(H * W, C).numpy()


def check_dwconv(ops, bitwise_to_host=False):
    for H, W, C in dwconv_cases():
        rng = np.random.default_rng((31, H, W, C))
        g = rng.standard_normal((H * W, C)).astype(np.float32)
        w = (rng.standard_normal((9, C)) / 3).astype(np.float32)
        b = rng.standard_normal(C).astype(np.float32)
        for relu in (False, True):
            out = ops.dwconv3x3(g, H, W, w, b, relu)
            within_bound(out, dwconv64(g, H, W, w, b, relu), f"{ops.name} dwconv {H}x{W}x{C} relu={relu}")
            if bitwise_to_host:
                assert np.array_equal(out.view(np.int32), host.dwconv3x3(g, H, W, w, b, relu).view(np.int32)), (H, W, C)


def check_neigh(ops, bitwise_to_host=False):
    for n, C, k, p0, np_ in ((17, 32, 16, 0, 17), (65, 256, 16, 3, 61), (700, 32, 16, 640, 60), (64, 8, 4, 0, 64)):
        rng = np.random.default_rng((41, n, C))
        feat = rng.standard_normal((n, 5)).astype(np.float32)
        knn = rng.integers(0, n, (n, k)).astype(np.int32)
        A = rng.standard_normal((5, C)).astype(np.float32)
        b = rng.standard_normal(C).astype(np.float32)
        rows = ops.neigh_rows(feat, knn, p0, np_, A, b)
        d = feat.astype(np.float64)[knn[p0:p0 + np_]] - feat.astype(np.float64)[p0:p0 + np_, None]
        ref = np.maximum(d.reshape(-1, 5) @ A.astype(np.float64) + b.astype(np.float64), 0.0)
        within_bound(rows, ref, f"{ops.name} neigh_rows n={n} C={C}")
        for ld in (C, 2 * C):
            mx = ops.group_max(rows, np_, k, ld)
            assert np.array_equal(mx, rows.reshape(np_, k, C).max(1)), (n, C, ld)
        if bitwise_to_host:
            assert np.array_equal(rows.view(np.int32), host.neigh_rows(feat, knn, p0, np_, A, b).view(np.int32)), (n, C)
