"""Edge cases of the view kernels (include/pasco_view.h, csrc/view.hip), numpy only, for both legs:
tests/test_view_edges_cpu.py hands `HostOps` (the restatement pasco_amd/viz/host.py) to the `check_*` functions below,
tests/test_hip_view_edges.py an object with the same methods over the pv_* kernels.  Expected values come from the literal
references of tests/view_cases.py (`pool_reference`, `filter_reference`, `brute_force`), from the two written here
(`compose_reference`, `bricks_reference`) or are stated by hand; `restatement` given, every result is also held to the
restatement in every bit."""
import itertools

import numpy as np

import view_cases as VC
from pasco_amd import viz
from pasco_amd.viz import host

F32 = np.float32
FACTORS, BG = (200, 228, 256), (9, 8, 7)
VIEWS = ("semantic", "panoptic", "mask", "vox_conf", "ins_conf")
# include/pasco_view.h, restated as numbers
STATUS_LABEL_RANGE, STATUS_STEP_CAP = 1, 2
INSTANCE_BASE, RAMP_BASE, STUFF_FIRST, STUFF_LAST, MAX_SEGMENTS, BRICK = 32, 1, 9, 19, 128, 8


class HostOps:
    name = "host"
    pool = staticmethod(host.majority_pool)
    filter = staticmethod(host.window_filter)
    bricks = staticmethod(host.bricks)

    @staticmethod
    def compose(view, shape, vmin, vmax, **inputs):
        return host.compose(view, shape, vmin=vmin, vmax=vmax, **inputs)

    @staticmethod
    def render(colour, cam, W, H, palette, step_cap=0):
        return host.render(colour, host.bricks(colour), cam, W, H, palette, FACTORS, BG, step_cap)


# !! The functions of this section restate the launch arithmetic of csrc/view.hip.  They are used to CHOOSE shapes and to assert,
# !! at import, that the cases below reach every launch class - never to form an expected value.  If a kernel's launch changes,
# !! the assertions say which class the cases lost.
BLOCK, TILE = 256, 16


def launch(threads):
    """(blocks, threads of the last block that have work; 0 = the last block is full)."""
    return -(-threads // BLOCK), threads % BLOCK


def tiles(W, H):
    """(tiles along x, along y, pixels of the last tile's row, of its column; 0 = full)."""
    return -(-W // TILE), -(-H // TILE), W % TILE, H % TILE


def brick_words(shape):
    """(bricks, words, bits of the last word that name a brick; 0 = all 32)."""
    n = int(np.prod([-(-s // BRICK) for s in shape]))
    return n, -(-n // 32), n % 32


def _need(ok, what):
    assert ok, f"the cases lost a launch class: {what}"


COMPOSE_SHAPES = ((5, 7, 3), (7, 37, 1))
SEGMENTS = (0, 1, 127, 128)
POOL_ODD, POOL_COUNT, POOL_LABELS = (10, 7, 5), (16, 8, 8), (8, 8, 8)
FILTER_SHAPE = (5, 6, 4)
RENDER_GRID, RENDER_W, RENDER_H = (16, 16, 8), 17, 9
CAP_GRID = (64, 8, 8)
BRICK_SHAPES = (RENDER_GRID, CAP_GRID, (41, 17, 9))

_need(launch(int(np.prod(COMPOSE_SHAPES[0]))) == (1, 105), "pv_compose, one partial block (the tail guard after the barriers)")
_need(launch(int(np.prod(COMPOSE_SHAPES[1]))) == (2, 3), "pv_compose, a second block of three sites")
_need(max(SEGMENTS) == MAX_SEGMENTS and MAX_SEGMENTS - 1 in SEGMENTS and 0 in SEGMENTS, "pv_compose, the table empty, full and one short")
_need([launch(int(np.prod([s // k for s in POOL_ODD]))) for k in (2, 4, 8)] == [(1, 30), (1, 2), (0, 0)],
      "pv_majority_pool, a remainder on every axis and an axis below k")
_need(all(sum(1 for s in POOL_ODD if s % k) >= 2 for k in (2, 4)), "pv_majority_pool, two axes that k does not divide")
_need(launch(int(np.prod(FILTER_SHAPE))) == (1, 120), "pv_window_filter, one partial block")
_need(tiles(RENDER_W, RENDER_H) == (2, 1, 1, 9), "pv_render, tiles partial on both axes")
_need(brick_words(RENDER_GRID) == (4, 1, 4) and brick_words(CAP_GRID) == (8, 1, 8), "pv_bricks, one word partly filled")
_need(brick_words(BRICK_SHAPES[2]) == (36, 2, 4) and all(s % BRICK for s in BRICK_SHAPES[2]),
      "pv_bricks, a second word partly filled and bricks clipped on every axis")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---- pv_majority_pool -----------------------------------------------------------------------------------------------------
def pool_cases():
    """name -> (grid, k, expected status, hand-stated cells {index: label})."""
    out = {}
    odd = VC.noise_labels(21, POOL_ODD, p=0.7, classes=8, unknown=0.15)
    odd[8:, :, :], odd[:, 6:, :], odd[:, :, 4:] = 7, 7, 7               # layers that k = 2 or k = 4 leaves over at the far faces
    odd[8:10, 0:2, 0:2] = 3                                             # x = 8, 9 is left over by k = 4 and the last cell of k = 2
    for k in (2, 4, 8):
        out[f"10x7x5 k={k}"] = (odd, k, 0, {(4, 0, 0): 3} if k == 2 else {})
    count = np.zeros(POOL_COUNT, np.uint8)
    count[:8] = 31                                                      # 512 times the top label: past a byte-wide counter
    count[8:] = 1
    count[15, 7, 7] = 2                                                 # 511 times label 1 and one label 2
    out["16x8x8 k=8, counts of 512 and 511"] = (count, 8, 0, {(0, 0, 0): 31, (1, 0, 0): 1})
    labels = VC.noise_labels(22, POOL_LABELS, p=0.8, classes=20, unknown=0.0)
    labels[0:2, 0:2, 0:2], labels[2:4, 0:2, 0:2], labels[4:6, 0:2, 0:2], labels[6:8, 0:2, 0:2] = 31, 32, 254, 255
    labels[0:2, 2:4, 0:2] = 32
    labels[0, 2, 0] = 0                                                 # 32 counts as 255: with a 0 beside it the cell is 0
    labels[2:4, 2:4, 0:2] = 254
    labels[2, 2, 0] = 31                                                # and one real label beside 254 wins
    out["8x8x8 k=2, labels 31 32 254 255"] = (labels, 2, STATUS_LABEL_RANGE,
                                              {(0, 0, 0): 31, (1, 0, 0): 255, (2, 0, 0): 255, (3, 0, 0): 255, (0, 1, 0): 0, (1, 1, 0): 31})
    only255 = labels.copy()
    only255[labels == 32], only255[labels == 254] = 255, 255
    out["8x8x8 k=2, 255 alone raises nothing"] = (only255, 2, 0, {(1, 0, 0): 255, (3, 0, 0): 255})
    return out


def check_pool(ops, restatement=None):
    for name, (grid, k, status, cells) in pool_cases().items():
        exp, exp_st = VC.pool_reference(grid, k)
        got, st = ops.pool(grid, k)
        assert got.shape == tuple(s // k for s in grid.shape) and got.dtype == np.uint8, name
        assert np.array_equal(got, exp) and st == exp_st == status, name
        for index, label in cells.items():
            assert got[index] == label, (name, index)
        if restatement is not None:
            r, r_st = restatement.pool(grid, k)
            assert same_bits(got, r) and st == r_st, name


# ---- pv_window_filter -----------------------------------------------------------------------------------------------------
def filter_cases():
    """name -> (grid, mask or None, compared in every bit)."""
    rng = np.random.default_rng(31)
    neg = (rng.random(FILTER_SHAPE, dtype=np.float32) - F32(1.5)).astype(np.float32)
    neg[rng.random(FILTER_SHAPE) < 0.3] = 255.0
    assert (neg[neg != 255.0] < -0.5).all() and (neg[neg != 255.0] >= -1.5).all()
    mask = (rng.random(FILTER_SHAPE) < 0.6).astype(np.uint8)
    same = np.full(FILTER_SHAPE, 0.3, np.float32)
    same[rng.random(FILTER_SHAPE) < 0.3] = 255.0
    zeros = np.where(rng.random(FILTER_SHAPE) < 0.5, F32(0.0), F32(-0.0)).astype(np.float32)
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    return {"all negative": (neg, None, True), "all negative, masked": (neg, mask, True), "one repeated value": (same, None, True),
            "one repeated value, masked": (same, mask, True), "+0.0 and -0.0": (zeros, None, False),
            "+0.0 and -0.0, masked": (zeros, mask, False), "a mask of zeros": (neg, np.zeros(FILTER_SHAPE, np.uint8), True)}


def check_filter(ops, restatement=None):
    for name, (grid, mask, bits) in filter_cases().items():
        for op in ("median", "max", "avg"):
            exp = VC.filter_reference(grid, op, mask)
            got = ops.filter(grid, op, mask)
            assert got.dtype == np.float32 and got.shape == grid.shape
            # the sign of a zero median or maximum is not defined by the reference: those two grids are compared by value
            assert same_bits(got, exp) if bits else np.array_equal(got, exp), (name, op)
            if name.startswith("all negative") and op != "avg":
                valid = got != 255.0
                assert valid.any() and (got[valid] < -0.5).all(), (name, op)      # a maximum that started at 0 would be 0
            if name.startswith("one repeated"):
                assert np.isin(got, F32([0.3, 255.0])).all() or op == "avg", (name, op)
            if name == "a mask of zeros":
                assert (got == 255.0).all(), op
            if restatement is not None:
                r = restatement.filter(grid, op, mask)
                assert same_bits(got, r) if bits else np.array_equal(got, r), (name, op)


# ---- pv_compose -----------------------------------------------------------------------------------------------------------
def _q(c, vmin, vmax):
    """The header's q(c), one rounded fp32 operation at a time."""
    c, vmin, vmax = F32(c), F32(vmin), F32(vmax)
    if not vmax > vmin:
        return 0
    t = F32(F32(c - vmin) / F32(vmax - vmin))
    t = t if t > 0 else F32(0.0)
    t = t if t < 1 else F32(1.0)
    return int(F32(F32(t * F32(255.0)) + F32(0.5)))


def compose_reference(view, shape, vmin, vmax, panoptic=None, seg=None, sem=None, conf=None):
    """A loop over the sites and, per site, over the segment table, from the table of views in include/pasco_view.h."""
    out = np.zeros(shape, np.uint32)
    n_seg = 0 if seg is None else seg.shape[1]
    ids = [] if seg is None else seg[0].tolist()
    thing = [] if seg is None else [v != 0 for v in seg[1].tolist()]
    level = [] if seg is None else [_q(c, vmin, vmax) for c in seg[3].view(np.float32)]
    for site in itertools.product(*(range(s) for s in shape)):
        if view == "semantic":
            c = int(sem[site])
            out[site] = c if c not in (0, 255) else 0
        elif view == "vox_conf":
            out[site] = RAMP_BASE + _q(conf[site], vmin, vmax) if sem[site] != 0 else 0
        else:
            ident, s = int(panoptic[site]), None
            if ident != 0:
                for i in range(n_seg):                       # the first segment with that id
                    if ids[i] == ident:
                        s = i
                        break
            if s is not None and thing[s]:
                rank = sum(thing[:s + 1])
                out[site] = RAMP_BASE + level[s] if view == "ins_conf" else INSTANCE_BASE + rank - 1
            elif view == "panoptic" and STUFF_FIRST <= int(sem[site]) <= STUFF_LAST:
                out[site] = int(sem[site])
    return out


def compose_inputs(shape, n_seg, twice):
    """Ids 0, 1 .. n_seg, one id no segment has and a negative one in the grid; `twice` = "thing first" or "stuff first": the
    last entry of the table repeats the id of entry 0 with the other kind (n_seg >= 2)."""
    rng = np.random.default_rng((41, n_seg) + tuple(shape))
    sem = rng.integers(0, 21, shape).astype(np.uint8)
    sem.reshape(-1)[:4] = (0, 255, 9, 19)
    pan = rng.integers(0, max(n_seg, 1) + 1, shape).astype(np.int32)
    flat = pan.reshape(-1)
    flat[5:9] = (0, n_seg + 5, -3, 1)
    flat[-1], flat[-2] = 1, -3                                # the last site of the last block belongs to the repeated id
    conf = rng.random(shape, dtype=np.float32)
    seg = None
    if n_seg:
        seg = np.zeros((4, n_seg), np.int32)
        seg[0] = np.arange(1, n_seg + 1)
        seg[1] = np.arange(n_seg) % 3 != 1
        seg[2] = 1 + np.arange(n_seg) % 8
        seg[3] = (0.25 + 0.5 * ((np.arange(n_seg) * 37) % 128) / 127.0).astype(np.float32).view(np.int32)
        if n_seg >= 2:
            seg[0, -1] = seg[0, 0]
            seg[1, 0], seg[1, -1] = (1, 0) if twice == "thing first" else (0, 1)
    return dict(panoptic=pan, seg=seg, sem=sem, conf=conf)


USES = {"semantic": ("sem",), "panoptic": ("panoptic", "seg", "sem"), "mask": ("panoptic", "seg"), "vox_conf": ("sem", "conf"),
        "ins_conf": ("panoptic", "seg")}


def check_compose(ops, shape, n_seg, restatement=None):
    for twice in ("thing first", "stuff first") if n_seg >= 2 else ("none",):
        inputs = compose_inputs(shape, n_seg, twice)
        assert {0, 1, -3, n_seg + 5} <= set(inputs["panoptic"].reshape(-1).tolist())
        for view in VIEWS:
            for vmin, vmax in ((0.25, 0.75), (0.5, 0.5)) if view.endswith("conf") else ((0.0, 1.0),):
                use = {k: inputs[k] for k in USES[view] if inputs[k] is not None}
                exp = compose_reference(view, shape, vmin, vmax, **use)
                got = ops.compose(view, shape, vmin, vmax, **use)
                assert got.dtype == np.uint32 and np.array_equal(got, exp), (shape, n_seg, twice, view, vmin)
                if restatement is not None:
                    assert same_bits(got, restatement.compose(view, shape, vmin, vmax, **use)), (shape, n_seg, twice, view)
        if n_seg >= 2:                                       # the first entry with the id decides: a thing, or stuff (no instance)
            mask = ops.compose("mask", shape, 0.0, 1.0, panoptic=inputs["panoptic"], seg=inputs["seg"])
            own = mask[inputs["panoptic"] == 1]
            assert own.size >= 2 and (own == (INSTANCE_BASE if twice == "thing first" else 0)).all(), (n_seg, twice)
            assert (mask[inputs["panoptic"] == -3] == 0).all() and (mask[inputs["panoptic"] == n_seg + 5] == 0).all()


# ---- pv_bricks ------------------------------------------------------------------------------------------------------------
def bricks_reference(colour):
    nb = [-(-s // BRICK) for s in colour.shape]
    n = nb[0] * nb[1] * nb[2]
    words = [0] * (-(-n // 32))
    for bx, by, bz in itertools.product(range(nb[0]), range(nb[1]), range(nb[2])):
        box = colour[bx * BRICK:(bx + 1) * BRICK, by * BRICK:(by + 1) * BRICK, bz * BRICK:(bz + 1) * BRICK]
        if (box != 0).any():
            b = (bx * nb[1] + by) * nb[2] + bz
            words[b >> 5] |= 1 << (b & 31)
    return np.array(words, np.uint32)


def check_bricks(ops, restatement=None):
    for shape in BRICK_SHAPES:
        grids = {"empty": np.zeros(shape, np.uint32), "sparse": VC.sparse_colour(51, shape, 0.004),
                 "far corner": np.zeros(shape, np.uint32)}
        grids["far corner"][-1, -1, -1] = 1                   # the last voxel, in the last (clipped) brick
        for name, colour in grids.items():
            got = ops.bricks(colour)
            assert same_bits(got, bricks_reference(colour)), (shape, name)
            if name == "far corner":
                n = brick_words(shape)[0]
                assert got[-1] == np.uint32(1 << ((n - 1) & 31)) and not got[:-1].any(), shape
            if name == "sparse":
                assert got.any(), shape
            if restatement is not None:
                assert same_bits(got, restatement.bricks(colour)), (shape, name)


# ---- pv_render ------------------------------------------------------------------------------------------------------------
def fixed_ray(origin, direction, negative_zeros=False):
    """A camera whose every pixel casts the same ray: du = dv = 0 (or -0.0 throughout, so that a -0.0 component stays -0.0)."""
    z = F32(-0.0) if negative_zeros else F32(0.0)
    cam = np.array(list(origin) + list(direction) + [z] * 6, np.float32)
    return cam


def site_of(x, y, z, shape=RENDER_GRID):
    return (x * shape[1] + y) * shape[2] + z


def tie_directions():
    two = [d for d in itertools.product((1, 0, -1), repeat=3) if sum(abs(v) for v in d) == 2]
    return two + list(itertools.product((1, -1), repeat=3))


def tie_camera(direction, shape=RENDER_GRID):
    """From integer coordinates two voxels outside the grid (3 on an axis the ray does not move along): every plane crossing of
    two or three axes happens at the same t."""
    origin = [(-2.0 if d > 0 else n + 2.0) if d else 3.0 for d, n in zip(direction, shape)]
    return fixed_ray(origin, [float(d) for d in direction])


def hand_cases():
    """(name, colour, camera, expected site, expected face), each worked out from "the smallest t wins, ties x, then y, then z"."""
    out = []
    diag = tie_camera((1, 1, 0))                              # o = (-2, -2, 3): x and y planes are both entered at t = 2
    g = np.zeros(RENDER_GRID, np.uint32)
    g[0, 0, 3] = 5
    out.append(("entry tie: the x face", g, diag, site_of(0, 0, 3), 0))
    g = np.zeros(RENDER_GRID, np.uint32)
    g[4, 5, 3], g[5, 4, 3], g[6, 6, 3] = 6, 7, 8            # the walk is (0,0) (1,0) (1,1) (2,1) ...: it never visits (4,5)
    out.append(("x steps before y", g, diag, site_of(5, 4, 3), 0))
    g = np.zeros(RENDER_GRID, np.uint32)
    g[3, 2, 2], g[2, 3, 2], g[2, 2, 3], g[3, 3, 3] = 9, 4, 4, 4      # from (-1,-1,-1) along (1,1,1): x, y, z, x, y, z, x
    out.append(("x before y before z", g, fixed_ray([-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]), site_of(3, 2, 2), 0))
    g = np.zeros(RENDER_GRID, np.uint32)
    g[14, 15, 3], g[15, 14, 3] = 6, 7                         # from (18, 18, 3) along (-1,-1,0): enters (15,15), then x first
    out.append(("x before y, moving down", g, tie_camera((-1, -1, 0)), site_of(14, 15, 3), 1))
    return out


def face_cases():
    """(name, camera, expected site or -1, face): an origin exactly on a face of the grid on an axis the ray does not move
    along - 0.0 is inside, the extent is outside - and -0.0 as a direction component.  The grid is full."""
    X, Y, Z = RENDER_GRID
    minus = fixed_ray([-2.0, 3.5, 3.5], [1.0, -0.0, -0.0], negative_zeros=True)
    d = (minus[3:6] + F32(3.0) * minus[6:9]) + F32(5.0) * minus[9:12]
    assert np.signbit(d[1]) and np.signbit(d[2]) and d[1] == 0          # the kernel's own sum keeps the -0.0
    return [("y = 0.0", fixed_ray([-2.0, 0.0, 3.5], [1.0, 0.0, 0.0]), site_of(0, 0, 3), 0),
            ("y = Y", fixed_ray([-2.0, float(Y), 3.5], [1.0, 0.0, 0.0]), -1, 255),
            ("z = 0.0", fixed_ray([-2.0, 3.5, 0.0], [1.0, 0.0, 0.0]), site_of(0, 3, 0), 0),
            ("z = Z", fixed_ray([-2.0, 3.5, float(Z)], [1.0, 0.0, 0.0]), -1, 255),
            ("x = 0.0", fixed_ray([0.0, -2.0, 3.5], [0.0, 1.0, 0.0]), site_of(0, 0, 3), 2),
            ("x = X", fixed_ray([float(X), -2.0, 3.5], [0.0, 1.0, 0.0]), -1, 255),
            ("x = 0.0 and z = 0.0, moving down y", fixed_ray([0.0, Y + 2.0, 0.0], [0.0, -1.0, 0.0]), site_of(0, Y - 1, 0), 3),
            ("-0.0 components", minus, site_of(0, 3, 3), 0)]


def tie_grids():
    a = VC.sparse_colour(61, RENDER_GRID, 0.1)
    b = a.copy()
    b[:, :8, :] = 0                                           # two empty bricks: brick steps tie as voxel steps do
    return {"sparse": a, "two empty bricks": b}


def _uniform(img, value, what):
    assert (np.asarray(img) == value).all(), what


def check_render(ops, restatement=None):
    pal = viz.ramp_palette()
    W, H = RENDER_W, RENDER_H

    def run(colour, cam, step_cap=0):
        got = ops.render(colour, cam, W, H, pal, step_cap)
        assert got[0].shape == (H, W) and got[1].shape == (H, W) and got[2].shape == (H, W, 3)
        if restatement is not None:
            r = restatement.render(colour, cam, W, H, pal, step_cap)
            assert all(same_bits(a, b) for a, b in zip(got[:3], r[:3])) and got[3] == r[3]
        return got

    for name, colour, cam, site, face in hand_cases():
        hit, f, rgb, status = run(colour, cam)
        _uniform(hit, site, name)
        _uniform(f, face, name)
        _uniform(rgb, ((pal[colour.reshape(-1)[site]].astype(np.int32) * FACTORS[face >> 1]) >> 8).astype(np.uint8), name)
        assert status == 0, name
    full = np.full(RENDER_GRID, 3, np.uint32)
    for name, cam, site, face in face_cases():
        hit, f, rgb, status = run(full, cam)
        _uniform(hit, site, name)
        _uniform(f, face, name)
        assert status == 0, name
        if site < 0:
            _uniform(rgb, np.array(BG, np.uint8), name)
    hits = 0
    for gname, colour in tie_grids().items():                # every tie ray, held to what no tie rule can change (`_slabs`)
        for d in tie_directions():
            cam = tie_camera(d)
            hit, f, _, status = run(colour, cam)
            assert status == 0 and (hit == hit[0, 0]).all() and (f == f[0, 0]).all(), (gname, d)
            sites, near, far = _slabs(colour, cam)
            through = far > near                              # the ray runs through the voxel, not only along an edge or a corner
            first = near[through].min() if through.any() else np.inf
            if hit[0, 0] < 0:
                assert not through.any(), (gname, d)
            else:
                hits += 1
                mine = int(np.flatnonzero(sites == hit[0, 0])[0])                 # the voxel hit is occupied,
                assert near[mine] <= far[mine] and near[mine] <= first, (gname, d)     # touched, and no later than the first one run through
                assert f[0, 0] >> 1 in [a for a in range(3) if d[a]] and (f[0, 0] & 1) == (d[f[0, 0] >> 1] < 0), (gname, d)
    assert hits >= 20
    colour = tie_grids()["sparse"]
    cams = {"behind": viz.preset("behind", RENDER_GRID, W, H),
            "from a corner": viz.camera([-6.3, -3.1, 14.2], [8.4, 7.7, 1.2], [0, 0, 1], 40.0, W, H),
            "inside": viz.camera([8.3, 7.1, 3.6], [16.0, 9.3, 0.7], [0, 0, 1], 40.0, W, H)}
    for cname, cam in cams.items():                           # the cameras without ties: the fp64 brute force on every pixel
        b_hit, b_face, tie = VC.brute_force(colour, cam, W, H)
        assert tie.sum() <= 0.01 * W * H, (cname, int(tie.sum()))
        hit, f, _, status = run(colour, cam)
        keep = ~tie
        assert status == 0 and np.array_equal(hit[keep], b_hit[keep]) and np.array_equal(f[keep].astype(np.int32), b_face[keep])
        assert (b_hit >= 0).sum() >= 0.1 * W * H


def _slabs(colour, cam):
    """fp64 slab intersection of a fixed-ray camera's ray with every occupied voxel -> (site, entry t, exit t) of the voxels it
    touches.  The tie rays have small integer data, so every t is exact."""
    o, d = cam[0:3].astype(np.float64), cam[3:6].astype(np.float64)
    vox = np.argwhere(colour != 0).astype(np.float64)
    near, far = np.full(vox.shape[0], -np.inf), np.full(vox.shape[0], np.inf)
    ok = np.ones(vox.shape[0], bool)
    for a in range(3):
        if d[a] == 0:
            ok &= (o[a] >= vox[:, a]) & (o[a] < vox[:, a] + 1)
        else:
            t_lo, t_hi = (vox[:, a] - o[a]) / d[a], (vox[:, a] + 1 - o[a]) / d[a]
            near, far = np.maximum(near, np.minimum(t_lo, t_hi)), np.minimum(far, np.maximum(t_lo, t_hi))
    ok &= (near <= far) & (far >= 0)
    return np.flatnonzero(colour.reshape(-1) != 0)[ok], near[ok], far[ok]


def check_coarse_cap(ops, restatement=None):
    """An empty 64 x 8 x 8 grid, a ray along +x through its eight bricks: a cap of three brick steps is reached (the status
    word says so, the pixel is a miss); without a cap the ray leaves the grid, status 0."""
    colour = np.zeros(CAP_GRID, np.uint32)
    cam = fixed_ray([-2.0, 3.5, 3.5], [1.0, 0.0, 0.0])
    pal = viz.ramp_palette()
    for cap, status in ((3, STATUS_STEP_CAP), (0, 0)):
        hit, face, rgb, st = ops.render(colour, cam, RENDER_W, RENDER_H, pal, cap)
        assert st == status, cap
        _uniform(hit, -1, cap)
        _uniform(face, 255, cap)
        _uniform(rgb, np.array(BG, np.uint8), cap)
        if restatement is not None:
            r = restatement.render(colour, cam, RENDER_W, RENDER_H, pal, cap)
            assert all(same_bits(a, b) for a, b in zip((hit, face, rgb), r[:3])) and st == r[3]
