"""The view kernels on the MI355X (include/pasco_view.h, csrc/view.hip) against the host restatement (pasco_amd/viz/host.py,
itself pinned to independent references in test_view_cpu.py): every integer, every byte and every fp32 bit equal, inputs
never written, and nothing written past the end of an output (guard entries behind each one)."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CONFIG = os.path.join(HERE, "golden", "semantic-kitti.yaml")

import view_cases as VC  # noqa: E402
from pasco_amd import viz  # noqa: E402
from pasco_amd.viz import host  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FULL = VC.FULL
GUARD = 64
FACTORS, BG = (200, 228, 256), (9, 8, 7)


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.viz.lib import view_lib
    return view_lib()


def guarded(numel, dtype, fill):
    """An output buffer of `numel` entries with GUARD more behind it, all set to `fill`."""
    return torch.full((numel + GUARD,), fill, dtype=dtype, device=DEV)


def untouched(buf, numel, fill):
    return bool((buf[numel:] == fill).all())


def dev(a):
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(t, a):
    """Device tensor == host array, bit for bit."""
    a = np.ascontiguousarray(a)
    h = t.cpu().numpy().reshape(-1)
    return np.array_equal(h.view(np.uint8), a.reshape(-1).view(np.uint8))


# ---- pool ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8, 8), (24, 16, 8)])
@pytest.mark.parametrize("k", [2, 4, 8])
def test_pool_small(lib, shape, k):
    g = VC.noise_labels(1, shape, p=0.7, classes=8, unknown=0.2)
    g[0:2, 0:2, 0:2] = 255
    g[2:4, 0:2, 0:2] = [[[3, 3], [5, 5]], [[5, 3], [0, 255]]]
    for bad in (False, True):
        if bad:
            g[5, 5, 5] = 40
        exp, st = host.majority_pool(g, k)
        d = dev(g)
        out = guarded(exp.size, torch.uint8, 77)
        _, status = lib.majority_pool(d, k, out=out)
        torch.cuda.synchronize(DEV)
        assert same(out[:exp.size], exp) and untouched(out, exp.size, 77) and int(status.item()) == st == int(bad)
        assert same(d, g), "the input was written"


def test_pool_full_noise_grid(lib):
    g = VC.noise_labels(2, FULL, p=0.6, classes=20, unknown=0.1)
    d = dev(g)
    for k in (2, 4, 8):
        exp, _ = host.majority_pool(g, k)
        out, status = lib.majority_pool(d, k)
        assert same(out, exp) and int(status.item()) == 0 and tuple(out.shape) == exp.shape


# ---- filter -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 3, 3), (5, 6, 4), (33, 9, 32)])
def test_filter_small(lib, shape):
    for seed, sentinel in ((0, 0.4), (1, 0.0), (2, 1.0), (3, 0.9)):
        g = VC.conf_grid(seed, shape, sentinel)
        mask = (VC.noise_labels(seed, shape, p=0.7, classes=3, unknown=0.0) != 0).astype(np.uint8)
        d, dm = dev(g), dev(mask)
        for op in ("median", "max", "avg"):
            for m, hm in ((None, None), (dm, mask)):
                exp = host.window_filter(g, op, hm)
                out = guarded(g.size, torch.float32, -3.0)
                lib.window_filter(d, op, m, out=out)
                torch.cuda.synchronize(DEV)
                assert same(out[:g.size], exp), (shape, seed, op, m is not None)
                assert untouched(out, g.size, -3.0)
        assert same(d, g) and same(dm, mask)


def test_filter_full_grid(lib):
    g = VC.conf_grid(5, FULL, 0.6)
    sem = VC.blob_labels(5)
    d, dm = dev(g), dev(sem)
    for op in ("median", "max", "avg"):
        assert same(lib.window_filter(d, op, dm), host.window_filter(g, op, sem)), op
    assert same(lib.window_filter(d, "median"), host.window_filter(g, "median"))


# ---- compose ------------------------------------------------------------------------------------------------------------
def compose_inputs(n_seg):
    """A full-size frame with `n_seg` segments: every third one a stuff segment, one id that no voxel has, one voxel id (n_seg
    + 5) that no segment has; thing confidences spread over [0.25, 0.75] with both ends present."""
    rng = np.random.default_rng(n_seg)
    sem = VC.blob_labels(7)
    pan = (rng.integers(0, n_seg + 1, FULL) * (sem != 0)).astype(np.int32)
    pan[pan == 2] = 0                                        # id 2 is in the table and in no voxel
    pan[10:12, 10:12, 4:6] = n_seg + 5                       # in the grid and in no segment
    conf = rng.random(FULL, dtype=np.float32)
    infos = []
    for s in range(n_seg):
        c = 0.25 + 0.5 * ((s * 37) % 128) / 127.0
        infos.append({"id": (s * 5) % n_seg + 1 if n_seg % 5 else s + 1, "isthing": s % 3 != 1, "category_id": 1 + s % 8,
                      "confidence": float(np.float32(c))})
    return sem, pan, conf, viz.frames.segment_table(infos)


@pytest.mark.parametrize("n_seg", [0, 1, 128])
def test_compose_full_grid(lib, n_seg):
    sem, pan, conf, seg = compose_inputs(n_seg)
    things = seg[3, seg[1] != 0].view(np.float32)
    lo, hi = (float(things.min()), float(things.max())) if things.size else (0.0, 0.0)
    if n_seg == 128:
        assert lo == 0.25 and hi == 0.75 and len(set(seg[0].tolist())) == 128
    d_sem, d_pan, d_conf = dev(sem), dev(pan), dev(conf)
    d_seg = dev(seg) if n_seg else None
    h_seg = seg if n_seg else None
    S = sem.size
    cases = [("semantic", dict(sem=True), 0.0, 1.0), ("panoptic", dict(panoptic=True, seg=True, sem=True), 0.0, 1.0),
             ("mask", dict(panoptic=True, seg=True), 0.0, 1.0), ("vox_conf", dict(sem=True, conf=True), 0.125, 0.875),
             ("vox_conf", dict(sem=True, conf=True), 0.5, 0.5), ("ins_conf", dict(panoptic=True, seg=True), lo, hi),
             ("ins_conf", dict(panoptic=True, seg=True), 0.5, 0.5)]            # vmin == vmax: level 0, nothing divided
    for view, use, vmin, vmax in cases:
        kw_d = {k: {"sem": d_sem, "panoptic": d_pan, "conf": d_conf, "seg": d_seg}[k] for k in use}
        kw_h = {k: {"sem": sem, "panoptic": pan, "conf": conf, "seg": h_seg}[k] for k in use}
        exp = host.compose(view, FULL, vmin=vmin, vmax=vmax, **kw_h)
        out = guarded(S, torch.int32, -5)
        lib.compose(view, FULL, vmin=vmin, vmax=vmax, out=out, **kw_d)
        torch.cuda.synchronize(DEV)
        assert same(out[:S], exp), (view, n_seg, vmin, vmax)
        assert untouched(out, S, -5)
        if view == "ins_conf" and n_seg == 128 and vmin < vmax:
            assert {1, 256} <= set(np.unique(exp).tolist())                    # a thing exactly at vmin and one at vmax
    assert same(d_sem, sem) and same(d_pan, pan) and same(d_conf, conf) and (d_seg is None or same(d_seg, seg))


# ---- bricks and render --------------------------------------------------------------------------------------------------
def corner_grid(shape, corner):
    g = np.zeros(shape, np.uint32)
    g[tuple((s - 1) * c for s, c in zip(shape, corner))] = 7
    return g


def render_grids():
    grids = {"empty": np.zeros((16, 16, 8), np.uint32), "full": np.full((16, 16, 8), 3, np.uint32),
             "32x32x4": VC.sparse_colour(1, (32, 32, 4), 0.1), "10x7x3": VC.sparse_colour(2, (10, 7, 3), 0.2)}
    for c in range(8):
        grids[f"corner{c}"] = corner_grid((10, 7, 3), (c & 1, (c >> 1) & 1, c >> 2))
    return grids


def cameras(shape, W, H):
    X, Y, Z = shape
    cams = {"behind": viz.preset("behind", shape, W, H), "top": viz.preset("top", shape, W, H),
            "oblique": viz.preset("oblique", shape, W, H),
            "inside": viz.camera([X / 2 + 0.3, Y / 2 + 0.4, Z / 2 + 0.2], [X, Y / 2, 0.5], [0, 0, 1], 70.0, W, H),
            "inside corner voxel": viz.camera([X - 0.5, Y - 0.5, Z - 0.5], [0, 0, 0], [0, 0, 1], 60.0, W, H),
            "away": viz.camera([-5.0, Y / 2, Z + 4.0], [-20.0, Y / 2, Z + 9.0], [0, 0, 1], 40.0, W, H)}
    for a in range(3):                        # exactly along each axis, both ways: two direction components are exactly 0
        for sign in (1, -1):
            c = np.zeros(12, np.float32)
            c[0:3] = [X / 2 + 0.25, Y / 2 + 0.25, Z / 2 + 0.25]
            c[a] = -3.0 if sign > 0 else shape[a] + 3.0
            c[3 + a] = sign
            cams[f"axis{a}{'+' if sign > 0 else '-'}"] = c
    return cams


def render_both(lib, colour, cam, W, H, pal, step_cap=0):
    bits_h = host.bricks(colour)
    d_col = dev(colour)
    words = bits_h.size
    bits = guarded(words, torch.int32, 0x5A5A5A5A)
    lib.bricks(d_col, out=bits)
    hit, face, rgb = guarded(W * H, torch.int32, -9), guarded(W * H, torch.uint8, 99), guarded(3 * W * H, torch.uint8, 99)
    status = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
    lib.render(d_col, bits, dev(cam), W, H, dev(pal), FACTORS, BG, step_cap, hit=hit, face=face, rgb=rgb, status=status)
    torch.cuda.synchronize(DEV)
    e_hit, e_face, e_rgb, e_status = host.render(colour, bits_h, cam, W, H, pal, FACTORS, BG, step_cap)
    assert same(bits[:words], bits_h) and untouched(bits, words, 0x5A5A5A5A)
    assert same(hit[:W * H], e_hit) and untouched(hit, W * H, -9)
    assert same(face[:W * H], e_face) and untouched(face, W * H, 99)
    assert same(rgb[:3 * W * H], e_rgb) and untouched(rgb, 3 * W * H, 99)
    assert int(status[0].item()) == e_status and not status[1:].any()
    assert same(d_col, colour), "the colour grid was written"
    return e_hit, e_face, e_status


@pytest.mark.parametrize("size", [(1, 1), (37, 23)])
def test_render_small_grids_and_cameras(lib, size):
    W, H = size
    pal = viz.ramp_palette()
    for name, colour in render_grids().items():
        for cname, cam in cameras(colour.shape, W, H).items():
            if name.startswith("corner") and cname not in ("behind", "inside corner voxel", "axis0+", "axis2-"):
                continue
            hit, face, status = render_both(lib, colour, cam, W, H, pal)
            assert status == 0, (name, cname)
            if name == "empty" or cname == "away":
                assert (hit < 0).all(), (name, cname)
            if name == "full" and cname in ("inside", "inside corner voxel"):
                assert (face == host.FACE_INSIDE).all() and (hit == hit[0, 0]).all()      # no face was crossed
            if name == "full" and cname.startswith("axis"):
                a, plus = int(cname[4]), cname[5] == "+"
                assert (face == 2 * a + (0 if plus else 1)).all() and (hit >= 0).all()
    # the corner voxels are seen from the cameras that look at them
    corner = corner_grid((10, 7, 3), (1, 1, 1))
    hit, face, _ = render_both(lib, corner, cameras((10, 7, 3), 37, 23)["inside corner voxel"], 37, 23, pal)
    assert (hit == 10 * 7 * 3 - 1).all() and (face == host.FACE_INSIDE).all()


def test_render_step_cap_is_reported_not_a_fault(lib):
    """A ray that needs nine voxel steps under a cap of four: the status word says so and the pixel is a miss."""
    colour = np.zeros((10, 7, 3), np.uint32)
    colour[9, 3, 1], colour[0, 0, 0] = 5, 3
    cam = np.array([-2.0, 3.5, 1.5, 1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    hit, _, status = render_both(lib, colour, cam, 1, 1, viz.ramp_palette(), step_cap=4)
    assert status == host.STATUS_STEP_CAP and hit[0, 0] == -1
    hit, face, status = render_both(lib, colour, cam, 1, 1, viz.ramp_palette())
    assert status == 0 and hit[0, 0] == (9 * 7 + 3) * 3 + 1 and face[0, 0] == 0
    hit, _, status = render_both(lib, colour, cam, 1, 1, viz.ramp_palette()[:4])          # colour 5 is past this palette
    assert status == host.STATUS_PALETTE and hit[0, 0] >= 0


def test_render_full_blob_scene(lib):
    sem = VC.blob_labels(11, unknown=0.0)
    colour = host.compose("semantic", FULL, sem=sem)
    pal = viz.label_palette(CONFIG)
    for cname in ("behind", "top"):
        hit, _, status = render_both(lib, colour, viz.preset(cname, FULL, 128, 96), 128, 96, pal)
        assert status == 0 and (hit >= 0).mean() > 0.2, cname


# ---- downsample ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 2, 3])
@pytest.mark.parametrize("size", [(6, 6), (37, 23)])
def test_downsample(lib, s, size):
    W, H = size
    img = np.random.default_rng(s).integers(0, 256, (H * s, W * s, 3)).astype(np.uint8)
    img[0:s, 0:s] = 255                                      # a block of 255: the sum does not wrap
    d = dev(img)
    out = guarded(3 * W * H, torch.uint8, 99)
    lib.downsample(d, s, out=out)
    torch.cuda.synchronize(DEV)
    assert same(out[:3 * W * H], host.downsample(img, s)) and untouched(out, 3 * W * H, 99) and same(d, img)


# ---- the command --------------------------------------------------------------------------------------------------------
def test_command_on_the_device_and_on_the_host_write_the_same_bytes(hip, tmp_path, capsys):
    from pasco_amd.viz.__main__ import main
    src = os.path.join(tmp_path, "out")
    viz.write_record(src, "000005", 1, VC.synthetic_record())
    common = ["--outputs", src, "--config", CONFIG, "--size", "40", "--supersample", "2"]
    main(common + ["--save-folder", os.path.join(tmp_path, "gpu"), "--device", "cuda"])
    main(common + ["--save-folder", os.path.join(tmp_path, "cpu"), "--device", "cpu"])
    capsys.readouterr()
    names = sorted(os.listdir(os.path.join(tmp_path, "cpu")))
    assert len(names) == 10 and names == sorted(os.listdir(os.path.join(tmp_path, "gpu")))
    for n in names:
        with open(os.path.join(tmp_path, "cpu", n), "rb") as a, open(os.path.join(tmp_path, "gpu", n), "rb") as b:
            assert a.read() == b.read(), n


def test_argument_checks(lib):
    g = torch.zeros((8, 8, 8), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="pv_majority_pool"):
        lib.majority_pool(g, 3)
    c = torch.zeros((8, 8, 8), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="pv_compose"):
        lib.compose("mask", (8, 8, 8), panoptic=c, seg=torch.zeros((4, 129), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="pv_compose"):
        lib.compose("vox_conf", (8, 8, 8), sem=g)
    f = torch.zeros((8, 8, 8), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="pv_window_filter"):
        lib.window_filter(f, "max", out=f)


def test_scoring_saves_frames_that_the_command_draws(hip, tmp_path, capsys):
    """`eval.kitti --save-outputs` on the mini tree: the tables are the ones printed without the flag, every output of the
    frame is saved, and `python -m pasco_amd.viz` draws them."""
    import pickle
    import shutil
    from pasco_amd.eval import kitti as E
    from pasco_amd.viz.__main__ import main
    gold = os.path.join(HERE, "golden")
    root = os.path.join(tmp_path, "mini")
    shutil.copytree(os.path.join(gold, "kitti_mini"), root)
    pre, ckpt, out = os.path.join(root, "preprocess"), os.path.join(gold, "net_mini.ckpt"), os.path.join(tmp_path, "saved")
    plain, _ = E.evaluate(root, pre, ckpt, "08", frames=1)
    assert not os.path.exists(out)
    saved, _ = E.evaluate(root, pre, ckpt, "08", frames=1, save_outputs=out)
    assert plain.tables(step_time=0.0) == saved.tables(step_time=0.0)
    names = sorted(os.listdir(out))
    assert len(names) >= 2 and all(n.endswith(".pkl") for n in names)
    with open(os.path.join(out, names[-1]), "rb") as f:
        rec = pickle.load(f)
    assert tuple(rec) == viz.KEYS and rec["ssc_pred"].shape == (1, 64, 64, 16) == rec["vox_confidence_denses"].shape
    main(["--outputs", out, "--config", CONFIG, "--save-folder", os.path.join(tmp_path, "img"), "--size", "32", "--views",
          "semantic,panoptic,vox_conf", "--scales", "1,2"])
    capsys.readouterr()
    assert len(os.listdir(os.path.join(tmp_path, "img"))) == len(names) * 6
