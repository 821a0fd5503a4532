"""Edge cases of the point-feature kernels (include/pasco_waffle.h, csrc/waffle.hip), numpy only, for both legs:
tests/test_waffle_edges_cpu.py hands `HostOps` (the restatement pasco_amd/waffle/host.py) to the `check_*` functions below,
tests/test_hip_waffle_edges.py hands `waffle_device.DeviceOps` (the pw_* kernels).  Every expected value comes from
tests/waffle_ref.py, which shares no code with the restatement, or is written out here by hand.

An argument may be a `Placed` array (tests/placed.py): the same values at a chosen place inside a larger allocation of the
test's own.  That is how a pointer 4 bytes past a 16-byte boundary, a row stride above 3 and the status paths are reached.  SAFETY RULE of the
status paths, which the GPU leg depends on: every array that a bad index would address is `mid(...)` - a slice in the middle
of a larger allocation filled with a sentinel - and every bad index is -1, n or a few entries past n, so a kernel that ignored
its guard would still land inside that allocation and show as a wrong value, never as a fault.  No far index is used."""
import contextlib

import numpy as np

import waffle_cases as WC
import waffle_ref as R
from placed import columns, mid, off16, plain
from pasco_amd.waffle import host

BOUND = WC.BOUND                      # twice the reference's own fp32 error; used as it stands
WORST = {}                            # kernel -> worst error against float64 seen by the checks below (printed by the legs)


# ---- the restatement as an `ops` object -------------------------------------------------------------------------------------
def _unwrapped(fn):
    return staticmethod(lambda *args, **kw: fn(*[plain(a) for a in args], **kw))


class HostOps:
    """`waffle_cases.HostOps` with the status of every entry point that has one, taking `Placed` arguments as their views."""
    name = "host"
    voxel_keys = _unwrapped(host.voxel_keys)
    cell_index = _unwrapped(host.cell_index)
    grid_cells = _unwrapped(host.grid_cells)
    cells_build = _unwrapped(host.cells_build)
    knn = _unwrapped(host.knn)
    nearest = _unwrapped(host.nearest)
    flatten = _unwrapped(host.flatten_checked)
    dwconv3x3 = _unwrapped(host.dwconv3x3)
    inflate = _unwrapped(host.inflate_checked)
    neigh_rows = _unwrapped(host.neigh_rows)
    neigh_rows_status = _unwrapped(host.neigh_rows_checked)
    group_max = staticmethod(lambda rows, np_, k, ld_out: host.group_max(plain(rows), np_, k))

    @contextlib.contextmanager
    def output_off16(self):
        """The GPU leg puts the output 4 bytes past a 16-byte boundary inside this block; the host has no addresses."""
        yield


# !! The functions of this section restate the launch arithmetic of csrc/waffle.hip.  They are used to CHOOSE shapes and to assert,
# !! at import, that the tables below reach every launch class - never to form an expected value: those come from
# !! tests/waffle_ref.py alone.  If a kernel's launch changes, the assertions say which class the tables lost.
BLOCK, SEARCH_BLOCK = 256, 128


def launch(threads, block=BLOCK):
    """(blocks, threads of the last block that have work; 0 = the last block is full)."""
    return -(-threads // block), threads % block


def width(C, aligned=True):
    """Channels per thread of k_flatten / k_dwconv / k_inflate: 4 where C % 4 == 0 and every pointer is 16-byte aligned."""
    return 4 if C % 4 == 0 and aligned else 1


def cells_build_threads(n, ncell):
    return max(n, ncell + 1)


def _need(table, pred, what):
    assert any(pred(row) for row in table), f"the table lost a launch class: {what}"


# ---- searches -----------------------------------------------------------------------------------------------------------------
# (name, n, ks, m of pw_nearest (0 = none), row stride of points and queries)
SEARCH_TABLE = ([(f"n{n}", n, (1, 2, 31, 32), 0, 3) for n in (33, 129, 300)]
                + [(f"k=n-1 n{n}", n, (n - 1,), 0, 3) for n in (2, 3, 17, 33)]
                + [("coincident groups", 100, (1, 16, 32), 30, 3), ("grid 1x1x1", 70, (32,), 12, 3),
                   ("column 1x1x200", 90, (16,), 14, 3), ("on the cell planes", 200, (16,), 25, 3), ("one query", 33, (5,), 1, 3),
                   ("tie across cells", 34, (1, 2), 0, 3)]
                + [(f"ld6 n{n}", n, (16,), n, 6) for n in (127, 128, 129)])

_need(SEARCH_TABLE, lambda r: 1 in r[2], "pw_knn, k = 1")
_need(SEARCH_TABLE, lambda r: R.MAX_K in r[2] and r[1] > R.MAX_K + 1, "pw_knn, k = PW_MAX_K with points to evict")
_need(SEARCH_TABLE, lambda r: r[1] - 1 in r[2] and r[1] - 1 == R.MAX_K, "pw_knn, k = n - 1 = PW_MAX_K")
_need(SEARCH_TABLE, lambda r: r[1] - 1 in r[2] and r[1] == 2, "pw_knn, k = n - 1 = 1")
_need(SEARCH_TABLE, lambda r: launch(r[1], SEARCH_BLOCK) == (1, 33), "pw_knn, one partial block")
_need(SEARCH_TABLE, lambda r: launch(r[1], SEARCH_BLOCK) == (2, 1), "pw_knn, one query in the last block")
_need(SEARCH_TABLE, lambda r: launch(r[1], SEARCH_BLOCK)[0] == 3, "pw_knn, three blocks")
for _tail in (127, 0, 1):
    _need(SEARCH_TABLE, lambda r: r[4] > 3 and launch(r[1], SEARCH_BLOCK)[1] == _tail and launch(r[3], SEARCH_BLOCK)[1] == _tail,
          f"pw_knn / pw_nearest with ld = ldq > 3 and {_tail} queries in the last block")
_need(SEARCH_TABLE, lambda r: r[3] == 1, "pw_nearest, m = 1")


def _queries(xyz, m, seed):
    """m queries: inside the cloud's box, up to two extents outside it, and some on top of points."""
    rng = np.random.default_rng((seed, m))
    lo, hi = xyz.min(0), xyz.max(0)
    span = hi - lo + np.float32(1.0)
    q = (lo - 2 * span + rng.random((m, 3)) * 5 * span).astype(np.float32)
    q[::3] = (lo + rng.random((len(q[::3]), 3)) * (hi - lo)).astype(np.float32)
    q[1::7] = xyz[rng.integers(0, xyz.shape[0], len(q[1::7]))]
    return q


def search_case(name):
    """-> dict(xyz fp32 [n, 3], grid, ks, q fp32 [m, 3] or None, ld, literal = None or a function of (lists, k))."""
    row = next(r for r in SEARCH_TABLE if r[0] == name)
    _, n, ks, m, ld = row
    literal = None
    if name == "coincident groups":
        rng = np.random.default_rng(61)
        xyz = WC.cloud(n, 61, (6.0, 6.0, 2.0))
        perm = rng.permutation(n)
        big, small = np.sort(perm[:40]), np.sort(perm[40:43])
        xyz[big] = np.float32([0.75, -1.25, 0.5])             # after voxelisation many points share one position
        xyz[small] = np.float32([-2.0, 2.0, -0.5])
        grid = host.SearchGrid.around(xyz.min(0), xyz.max(0), 1.0)

        def literal(lists, k):                                # d2 = 0 ties go to the lowest OTHER indices of the group
            for member in (big[0], big[5]):
                others = [int(i) for i in big if i != member]
                assert lists[member, :min(k, 39)].tolist() == others[:min(k, 39)], (member, k)
            assert lists[small[1], :min(k, 2)].tolist() == [int(small[0]), int(small[2])][:min(k, 2)]
    elif name == "grid 1x1x1":                                # rmax = 1: no shell beyond the home cell
        xyz = (np.random.default_rng(62).random((n, 3)) * 10.0).astype(np.float32)
        grid = host.SearchGrid((0.0, 0.0, 0.0), 16.0, (1, 1, 1))
    elif name == "column 1x1x200":                            # every shell is two end cells
        rng = np.random.default_rng(63)
        xyz = np.stack([rng.random(n) * 0.49, rng.random(n) * 0.49, rng.random(n) * 99.9], 1).astype(np.float32)
        grid = host.SearchGrid((0.0, 0.0, 0.0), 0.5, (1, 1, 200))
    elif name == "on the cell planes":                        # coordinates exactly lo + j * h, and the cloud's maximum
        rng = np.random.default_rng(64)
        xyz = (rng.random((n, 3)) * np.array([5.0, 4.0, 1.5])).astype(np.float32)
        xyz[0], xyz[1] = (0.0, 0.0, 0.0), (5.0, 4.0, 1.5)     # the first cell's corner and the last cell's
        for j in range(2, 40):
            xyz[j, j % 3] = np.float32(0.5 * (j % 4))
        xyz[40:44] = [(2.5, 2.0, 1.0), (2.5, 2.0, 0.5), (5.0, 0.0, 0.0), (0.0, 4.0, 1.5)]
        grid = host.SearchGrid.around(xyz.min(0), xyz.max(0), 0.5)
        assert grid.G == (11, 9, 4) and grid.lo == (0.0, 0.0, 0.0)
    elif name == "tie across cells":                          # equal d2 from two cells, the lower index in the cell read second
        xyz = (np.float32(4.0) + np.random.default_rng(66).random((n, 3)) * 3.0).astype(np.float32)
        xyz[31:34] = [(2.25, 2.25, 0.75), (2.75, 2.25, 0.75), (1.75, 2.25, 0.75)]
        grid = host.SearchGrid.around(xyz.min(0), xyz.max(0), 0.5)
        assert grid.lo == (1.75, 2.25, 0.75)                  # 33, 31 and 32 lie in the cells 0, 1 and 2 of the first row

        def literal(lists, k):
            assert lists[31].tolist() == [32, 33][:k]
    else:
        xyz = WC.cloud(n, 60)
        grid = host.SearchGrid.around(xyz.min(0), xyz.max(0), 1.0)
    q = None
    if name == "column 1x1x200":                              # far outside on one, two and three axes (1 000 and 5 000 cells)
        q = np.float32([[0.25, 0.25, -500.0], [0.25, 0.25, 2600.0], [500.0, 0.25, 50.0], [0.25, -2500.0, 50.0],
                        [500.0, -500.0, 50.0], [-500.0, 0.25, 2600.0], [0.25, 2500.0, -500.0], [600.0, 600.0, -600.0],
                        [-2500.0, 500.0, 2600.0], [0.25, 0.25, 50.0], [0.1, 0.4, 99.95], [0.3, 0.2, 0.0], [0.6, 0.25, 30.0],
                        [0.25, -0.1, 70.0]])
        assert q.shape[0] == m
    elif m:
        q = _queries(xyz, m, 65)
    return dict(xyz=xyz, grid=grid, ks=ks, q=q, ld=ld, literal=literal)


def check_search(ops, name):
    c = search_case(name)
    xyz, g, q = c["xyz"], c["grid"], c["q"]
    xyz_arg = columns(xyz, c["ld"], 1) if c["ld"] > 3 else xyz
    cell, st = ops.grid_cells(xyz_arg, g)
    assert st == 0 and np.array_equal(cell, R.search_cell(xyz, g.lo, g.h, g.G)), name
    start, order, st = ops.cells_build(cell, g.ncell)
    exp_start, exp_order = R.csr(cell, g.ncell)
    assert st == 0 and np.array_equal(start, exp_start) and np.array_equal(order, exp_order), name
    if name == "on the cell planes":
        assert cell[0] == 0 and cell[1] == g.ncell - 1
    for k in c["ks"]:
        got = ops.knn(xyz_arg, start, order, g, k)
        assert got.shape == (xyz.shape[0], k) and np.array_equal(got, R.all_pairs(xyz, xyz, k, True)), (name, k)
        if c["literal"] is not None:
            c["literal"](got, k)
    if q is not None:
        q_arg = columns(q, c["ld"], 1, seed=6) if c["ld"] > 3 else q
        near = ops.nearest(xyz_arg, start, order, g, q_arg)
        assert near.shape == (q.shape[0],) and np.array_equal(near, R.all_pairs(xyz, q, 1, False)[:, 0]), name


# ---- keys and cells -------------------------------------------------------------------------------------------------------------
def check_voxel_keys(ops):
    top = np.float32(R.KEY_BOUND - 1)
    ok = np.float32([[0.0, 0.0, 0.0], [top, 1.0, 2.0], [-0.0, 3.0, top], [7.0, top, -0.0]])
    for pc, status in ((ok, 0), (np.concatenate([ok, np.float32([[top + 1, 5.0, 6.0]])]), R.STATUS_KEY_RANGE),
                       (np.concatenate([ok, np.float32([[1.0, 1.0, top + 1]])]), R.STATUS_KEY_RANGE)):
        assert float(top + 1) == R.KEY_BOUND and (pc.min(0) == 0).all()
        key, st = ops.voxel_keys(pc, pc.min(0), 1.0)
        exp, exp_st = R.voxel_keys(pc, 1.0)
        assert st == exp_st == status and np.array_equal(key, exp)
        assert key[1, 0] == R.KEY_BOUND - 1 and key[2].tolist() == [0, 3, R.KEY_BOUND - 1]
        if status:
            assert sorted(key[4].tolist())[0] == 0 and sorted(key[4].tolist())[1] > 0      # that key alone is written as 0


CELL_FOV = ([-5.0, -9.0, -1.5], [5.0, 9.0, 1.5])      # a 10 x 3 grid over (x, z) with cells of edge 1: quotient = coordinate - lo
CELL_DIMS, CELL_SHAPE = (0, 2), (10, 3)


def cell_probes():
    """(axis, quotient as the coordinate gives it, accepted) on both axes of the 10 x 3 grid."""
    up, down = np.float32(1e9), np.float32(-1e9)
    out = []
    for axis, lo, size in ((0, np.float32(-5.0), 10), (1, np.float32(-1.5), 3)):
        for v, accepted in ((lo - np.float32(0.5), True), (np.nextafter(lo - np.float32(1.0), up), True),
                            (lo - np.float32(1.0), False), (np.nextafter(lo - np.float32(1.0), down), False),
                            (lo - np.float32(3.0), False), (lo + np.float32(size - 1 + 0.999), True),
                            (np.nextafter(lo + np.float32(size), down), True), (lo + np.float32(size), False)):
            out.append((axis, np.float32(v), accepted))
    return out


def check_cell_index(ops):
    lo = [CELL_FOV[0][d] for d in CELL_DIMS]
    res = [(CELL_FOV[1][d] - CELL_FOV[0][d]) / s for d, s in zip(CELL_DIMS, CELL_SHAPE)]
    for axis, v, accepted in cell_probes():
        pc = np.float32([[0.25, 0.0, 0.25], [0.25, 0.0, 0.25]])       # a point in the middle, and the probe
        pc[1, CELL_DIMS[axis]] = v
        cell, st = ops.cell_index(pc, list(CELL_DIMS), lo, res, CELL_SHAPE)
        exp, exp_st = R.cell_index(pc, CELL_DIMS, CELL_FOV[0], CELL_FOV[1], CELL_SHAPE)
        assert np.array_equal(cell, exp) and st == exp_st == (0 if accepted else R.STATUS_OFF_GRID), (axis, v)
        assert cell[0] == 5 * 3 + 1
        if accepted and v < lo[axis]:                                 # a quotient in (-1, 0) truncates to 0, as the reference's cast does
            assert cell[1] == (0 * 3 + 1 if axis == 0 else 5 * 3 + 0), (axis, v)
        if accepted and v > 0:
            assert cell[1] == (9 * 3 + 1 if axis == 0 else 5 * 3 + 2), (axis, v)
        if not accepted:
            assert cell[1] == 0


# (n, ncell): pw_cells_build launches max(n, ncell + 1) threads
CSR_TABLE = [(40, 100), (300, 7), (256, 255), (1, 1)]
_need(CSR_TABLE, lambda r: r[0] < r[1] + 1, "pw_cells_build, fewer points than cells + 1")
_need(CSR_TABLE, lambda r: r[0] > r[1] + 1 and launch(cells_build_threads(*r))[0] > 1, "pw_cells_build, more points, two blocks")
_need(CSR_TABLE, lambda r: r[0] == r[1] + 1 and launch(cells_build_threads(*r))[1] == 0, "pw_cells_build, n = ncell + 1 = one full block")


def check_cells_build(ops):
    for n, ncell in CSR_TABLE:
        cell = np.random.default_rng((71, n)).integers(0, ncell, n).astype(np.int32)
        good = np.argsort(cell, kind="stable").astype(np.int32)
        start, order, st = ops.cells_build(mid(cell, 4, 4, 0), ncell, good)
        exp_start, exp_order = R.csr(cell, ncell)
        assert st == 0 and np.array_equal(start, exp_start) and np.array_equal(order, exp_order), (n, ncell)
        if n < 3:
            continue
        j = n // 2
        bad = {}
        for what, value in (("an entry of -1", -1), ("an entry of n", n), ("a repeated entry", good[j - 1])):
            o = good.copy()
            o[j] = value
            bad[what] = (cell, o)
        for what, value in (("a cell of ncell", ncell), ("a cell of -1", -1)):
            c = cell.copy()
            c[good[j]] = value
            bad[what] = (c, np.argsort(c, kind="stable").astype(np.int32))
        for what, (c, o) in bad.items():
            start, _, st = ops.cells_build(mid(c, 4, 4, 0), ncell, o)
            assert st == R.STATUS_ORDER, (n, ncell, what)
            assert start.shape == (ncell + 1,) and (start >= 0).all() and (start <= n).all(), (n, ncell, what)


# ---- float kernels ------------------------------------------------------------------------------------------------------------------
CHANNELS = (4, 8, 260, 6)
FLAT_N, FLAT_H, FLAT_W = 70, 10, 3
CONV_H, CONV_W = 5, 3
_float_table = [(C, aligned) for C in CHANNELS for aligned in ((True, False) if C % 4 == 0 else (True,))]
_need(_float_table, lambda r: width(*r) == 4 and launch(FLAT_H * FLAT_W * r[0] // 4)[0] > 1, "four channels per thread, several blocks")
_need(_float_table, lambda r: width(*r) == 4 and launch(FLAT_H * FLAT_W * r[0] // 4)[0] == 1, "four channels per thread, one partial block")
_need(_float_table, lambda r: width(*r) == 1 and r[0] % 4 == 0, "one channel per thread because a pointer is not 16-byte aligned")
_need(_float_table, lambda r: width(*r) == 1 and r[0] % 4 != 0, "one channel per thread because C % 4 != 0")
assert all(launch(FLAT_N * C // width(C))[1] != 0 for C in CHANNELS), "pw_inflate: a last block that is partly filled"


def within_bound(kernel, got, ref, what):
    e = WC.err(got, ref)
    WORST[kernel] = max(WORST.get(kernel, 0.0), e)
    print(f"{what}: error {e:.3e} (bound {BOUND:.3e})")
    assert e <= BOUND, f"{what}: error {e:.3e} > bound {BOUND:.3e}"


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


def _each_misaligned(ops, C, args, floats, call, aligned, what):
    """Every pointer argument in turn (then the output) 4 bytes past a 16-byte boundary: the same bits as the aligned call.
    A limit: the kernel is handed the offset address, so the one-channel path does run, but nothing here observes which path
    ran - a `wide` test that lost an `aligned16` term is caught only where the four-channel path then gives other bits."""
    if C % 4:
        return
    for i in floats:
        moved = list(args)
        moved[i] = off16(args[i])
        assert same_bits(call(*moved), aligned), f"{what}: argument {i} not 16-byte aligned"
    with ops.output_off16():
        assert same_bits(call(*args), aligned), f"{what}: output not 16-byte aligned"


def check_float_kernels(ops, restatement=None):
    """pw_flatten, pw_dwconv3x3 and pw_inflate at C in CHANNELS against float64 within BOUND, with every pointer in turn off
    its 16-byte boundary (the same bits), and - `restatement` given - every bit equal to the restatement's."""
    for C in CHANNELS:
        tok, sc, sh = WC.tokens_case(FLAT_N, C, 81)
        ncell = FLAT_H * FLAT_W
        cell = np.random.default_rng((82, C)).integers(0, ncell - 2, FLAT_N).astype(np.int32)      # the last two cells stay empty
        cell[:3] = ncell - 1                                                                       # but for three points in the last
        start, order = R.csr(cell, ncell)

        def flat(*a):
            grid, st = ops.flatten(*a, ncell)
            assert st == 0
            return grid
        args = [tok, sc, sh, start, order]
        grid = flat(*args)
        ref, _ = R.flatten64(tok, sc, sh, start, order, ncell)
        within_bound("pw_flatten", grid, ref, f"{ops.name} flatten C={C}")
        assert not grid[ncell - 2].any() and grid[ncell - 1].any()
        _each_misaligned(ops, C, args, (0, 1, 2), flat, grid, f"flatten C={C}")
        if restatement is not None:
            assert same_bits(grid, restatement.flatten(*args, ncell)[0]), C

        def infl(*a):
            out, st = ops.inflate(*a)
            assert st == 0
            return out
        args = [tok, sc, grid, cell]
        out = infl(*args)
        within_bound("pw_inflate", out, R.inflate64(tok, sc, grid, cell)[0], f"{ops.name} inflate C={C}")
        _each_misaligned(ops, C, args, (0, 1, 2), infl, out, f"inflate C={C}")
        if restatement is not None:
            assert same_bits(out, restatement.inflate(*args)[0]), C

        rng = np.random.default_rng((83, C))
        g = rng.standard_normal((CONV_H * CONV_W, C)).astype(np.float32)
        w = (rng.standard_normal((9, C)) / 3).astype(np.float32)
        b = rng.standard_normal(C).astype(np.float32)
        for relu in (False, True):
            def conv(gg, ww, bb):
                return ops.dwconv3x3(gg, CONV_H, CONV_W, ww, bb, relu)
            out = conv(g, w, b)
            within_bound("pw_dwconv3x3", out, R.dwconv64(g, CONV_H, CONV_W, w, b, relu), f"{ops.name} dwconv C={C} relu={relu}")
            _each_misaligned(ops, C, [g, w, b], (0, 1, 2), conv, out, f"dwconv C={C} relu={relu}")
            if restatement is not None:
                assert same_bits(out, restatement.dwconv3x3(g, CONV_H, CONV_W, w, b, relu)), (C, relu)


# (F, k, C) of pw_neigh_rows on 40 points, rows of the points 17 .. 39: the chunk ends at the last point
NEIGH_N, NEIGH_P0 = 40, 17
NEIGH_TABLE = [(F, k, C) for F in (1, R.MAX_FEAT) for k in (1, R.MAX_K) for C in (1, 65)]
_need(NEIGH_TABLE, lambda r: launch((NEIGH_N - NEIGH_P0) * r[1] * r[2]) == (1, 23), "pw_neigh_rows, F, k and C at their minimum: 23 threads")
_need(NEIGH_TABLE, lambda r: r == (R.MAX_FEAT, R.MAX_K, 65) and launch((NEIGH_N - NEIGH_P0) * r[1] * r[2])[0] > 100,
      "pw_neigh_rows, F and k at their maximum, C above a wave")


def check_neigh_rows(ops, restatement=None):
    np_ = NEIGH_N - NEIGH_P0
    for F, k, C in NEIGH_TABLE:
        rng = np.random.default_rng((91, F, k, C))
        feat = rng.standard_normal((NEIGH_N, F)).astype(np.float32)
        knn = rng.integers(0, NEIGH_N, (NEIGH_N, k)).astype(np.int32)
        knn[NEIGH_N - 1, k - 1] = NEIGH_N - 1                        # the last neighbour of the last point: itself
        A = rng.standard_normal((F, C)).astype(np.float32)
        b = rng.standard_normal(C).astype(np.float32)
        rows = ops.neigh_rows(feat, knn, NEIGH_P0, np_, A, b)
        ref, st = R.neigh_rows64(feat, knn, NEIGH_P0, np_, A, b)
        assert st == 0 and rows.shape == (np_ * k, C)
        within_bound("pw_neigh_rows", rows, ref, f"{ops.name} neigh_rows F={F} k={k} C={C}")
        assert same_bits(rows[-1], np.where(b > 0, b, np.float32(0.0)))
        if restatement is not None:
            assert same_bits(rows, restatement.neigh_rows(feat, knn, NEIGH_P0, np_, A, b)), (F, k, C)
        for ld in (C, C + 3):
            mx = ops.group_max(rows, np_, k, ld)
            exp = np.stack([rows[p * k:(p + 1) * k].max(0) for p in range(np_)])
            assert same_bits(np.ascontiguousarray(mx), exp), (F, k, C, ld)
            if k == 1:
                assert same_bits(np.ascontiguousarray(mx), rows)


# ---- status paths -----------------------------------------------------------------------------------------------------------------
SENTINEL = 1000.0             # what a read outside an array would fetch: far from every value of the case


def check_status_flatten(ops):
    n, ncell = 50, 12
    for C in (8, 6):
        tok, sc, sh = WC.tokens_case(n, C, 101)
        cell = np.random.default_rng((102, C)).permutation(np.arange(n) % ncell).astype(np.int32)     # four or five points per cell
        start, order = R.csr(cell, ncell)
        assert (np.diff(start) >= 4).all()
        # a row read before or behind `tokens` is SENTINEL; an entry read before or behind `order` lists point 0 again
        run = lambda s, o: ops.flatten(mid(tok, 2 * C, 2 * C, SENTINEL), sc, sh, s, mid(o, 8, 8, 0), ncell)
        clean, st = run(start, order)
        assert st == 0
        hit = 5                                                        # the cell whose list is damaged
        cases = {}
        for what, value in (("order -1", -1), ("order n", n)):
            o = order.copy()
            o[start[hit] + 1] = value
            cases[what] = (start, o, (hit,))
        s = start.copy()
        s[hit + 1] = s[hit] - 1                                        # cell `hit`: a > b (empty); the next cell starts one early
        cases["start a > b"] = (s, order, (hit, hit + 1))
        s = start.copy()
        s[ncell] = n + 3                                               # the last cell runs 3 entries past n: clipped
        cases["start b > n"] = (s, order, ())
        for what, (s, o, touched) in cases.items():
            grid, st = run(s, o)
            ref, ref_st = R.flatten64(tok, sc, sh, s, o, ncell)
            assert st == ref_st == R.STATUS_INDEX, (C, what)
            within_bound("pw_flatten", grid, ref, f"{ops.name} flatten C={C} {what}")
            keep = np.setdiff1d(np.arange(ncell), touched)
            assert same_bits(grid[keep], clean[keep]), (C, what)
            for c in touched:
                assert not same_bits(grid[c], clean[c]), (C, what)
        skipped, _ = run(*cases["order -1"][:2])                       # the skipped term is neither added nor counted
        members = order[start[hit]:start[hit + 1]]
        rest = np.delete(members, 1)
        t64 = tok[rest].astype(np.float64) * sc + sh
        assert WC.err(skipped[hit], t64.sum(0) / (rest.shape[0] + 1e-6)) <= BOUND


def check_status_inflate(ops):
    n, ncell = 50, 12
    for C in (8, 6):
        tok, sc, _ = WC.tokens_case(n, C, 111)
        grid = np.random.default_rng((112, C)).standard_normal((ncell, C)).astype(np.float32)
        cell = np.random.default_rng((113, C)).integers(0, ncell, n).astype(np.int32)
        run = lambda c: ops.inflate(tok, sc, mid(grid, 2 * C, 2 * C, SENTINEL), c)
        clean, st = run(cell)
        assert st == 0
        for p, value in ((7, -1), (n - 1, ncell)):
            c = cell.copy()
            c[p] = value
            out, st = run(c)
            ref, ref_st = R.inflate64(tok, sc, grid, c)
            assert st == ref_st == R.STATUS_INDEX, (C, value)
            within_bound("pw_inflate", out, ref, f"{ops.name} inflate C={C} cell {value}")
            assert same_bits(out[p], tok[p]) and not same_bits(clean[p], tok[p]), (C, value)      # the row is left as it was
            keep = np.arange(n) != p
            assert same_bits(out[keep], clean[keep]), (C, value)


def check_status_neigh_rows(ops):
    n, F, k, C, p0 = 40, 5, 4, 9, 10
    np_ = n - p0
    rng = np.random.default_rng(121)
    feat = rng.standard_normal((n, F)).astype(np.float32)
    knn = rng.integers(0, n, (n, k)).astype(np.int32)
    A, b = rng.standard_normal((F, C)).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    run = lambda kk: ops.neigh_rows_status(mid(feat, 2 * F, 2 * F, SENTINEL), kk, p0, np_, A, b)
    clean, st = run(knn)
    assert st == 0
    for (p, j), value in (((p0, 0), -1), ((n - 1, k - 1), n)):
        kk = knn.copy()
        kk[p, j] = value
        rows, st = run(kk)
        ref, ref_st = R.neigh_rows64(feat, kk, p0, np_, A, b)
        assert st == ref_st == R.STATUS_INDEX, value
        within_bound("pw_neigh_rows", rows, ref, f"{ops.name} neigh_rows neighbour {value}")
        r = (p - p0) * k + j
        assert same_bits(rows[r], np.where(b > 0, b, np.float32(0.0))), value                    # every difference is 0
        keep = np.arange(np_ * k) != r
        assert same_bits(rows[keep], clean[keep]), value
    kk = knn.copy()
    kk[0, 0] = -1                                                     # a point outside the chunk p0 .. n - 1 is not read
    rows, st = run(kk)
    assert st == 0 and same_bits(rows, clean)


def check_status_search(ops):
    """A CSR whose `order` holds -1 and n lists two points fewer: the search is the all-pairs search over the points still
    listed.  A `start` that runs past n is clipped: the result is the clean call's."""
    n = 40
    xyz = WC.cloud(n, 131, (4.0, 4.0, 2.0))
    xyz[0] = xyz.max(0)                                               # a point in the last cell, whose range will run past n
    g = host.SearchGrid.around(xyz.min(0), xyz.max(0), 1.0)
    cell = R.search_cell(xyz, g.lo, g.h, g.G)
    start, order = R.csr(cell, g.ncell)
    assert cell[0] == g.ncell - 1
    q = _queries(xyz, 20, 132)
    points = mid(xyz, 6, 6, float(np.float32(xyz.mean())))            # a row read before or behind xyz would be a near point
    listed = lambda o: mid(o, 8, 8, 0)                                # an entry read before or behind `order` lists point 0 again
    for k in (5, R.MAX_K):
        clean = ops.knn(points, start, listed(order), g, k)
        assert np.array_equal(clean, R.all_pairs(xyz, xyz, k, True)), k
        near_clean = ops.nearest(points, start, listed(order), g, q)
        gone = (int(order[3]), int(order[n - 2]))
        o = order.copy()
        o[3], o[n - 2] = -1, n
        present = np.ones(n, bool)
        present[list(gone)] = False
        got = ops.knn(points, start, listed(o), g, k)
        assert np.array_equal(got, R.all_pairs(xyz, xyz, k, True, present)), k
        assert not np.isin(got, gone).any() and (got >= 0).all()
        same = ~np.isin(clean, gone).any(1)
        assert np.array_equal(got[same], clean[same]) and (same.any() or k == R.MAX_K), k
        near = ops.nearest(points, start, listed(o), g, q)
        assert np.array_equal(near, R.all_pairs(xyz, q, 1, False, present)[:, 0]), k
        untouched = ~np.isin(near_clean, gone)
        assert np.array_equal(near[untouched], near_clean[untouched])
        s = start.copy()
        s[g.ncell] = n + 5
        assert np.array_equal(ops.knn(points, s, listed(order), g, k), clean), k
        assert np.array_equal(ops.nearest(points, s, listed(order), g, q), near_clean), k
