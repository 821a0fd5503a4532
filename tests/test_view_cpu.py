"""The numpy restatement of the view kernels (pasco_amd/viz/host.py) against independent references written one cell, one
window and one ray-voxel pair at a time (tests/view_cases.py), and the files the two commands write.  No GPU."""
import os
import pickle
import struct
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
CONFIG = os.path.join(HERE, "golden", "semantic-kitti.yaml")

import view_cases as VC  # noqa: E402
from pasco_amd import viz  # noqa: E402
from pasco_amd.viz import host  # noqa: E402


# ---- pooling ------------------------------------------------------------------------------------------------------------
def pool_grid(shape):
    g = VC.noise_labels(3, shape, p=0.6, classes=6, unknown=0.15)
    g[0:2, 0:2, 0:2] = 255                                   # a cell of 255 only
    g[2:4, 0:2, 0:2] = 255
    g[2, 0, 0] = 0                                           # 0 and 255 only
    g[4:6, 0:2, 0:2] = [[[3, 3], [5, 5]], [[5, 3], [0, 255]]]          # 3 and 5 three times each: 3
    g[6:8, 0:2, 0:2] = [[[7, 7], [4, 4]], [[2, 2], [0, 255]]]          # 2, 4 and 7 twice each: 2
    return g


@pytest.mark.parametrize("shape", [(8, 8, 8), (16, 24, 8)])
@pytest.mark.parametrize("k", [2, 4, 8])
def test_pooling_against_a_unique_per_cell_loop(shape, k):
    g = pool_grid(shape)
    exp, st = VC.pool_reference(g, k)
    got, status = host.majority_pool(g, k)
    assert got.dtype == np.uint8 and got.shape == tuple(s // k for s in shape)
    assert status == 0 and st == 0 and np.array_equal(got, exp)
    if k == 2:
        assert got[0, 0, 0] == 255 and got[1, 0, 0] == 0 and got[2, 0, 0] == 3 and got[3, 0, 0] == 2
    g[5, 5, 5] = 40                                          # outside 0 .. 31 and 255: reported, counted as 255
    exp, st = VC.pool_reference(g, k)
    got, status = host.majority_pool(g, k)
    assert st == 1 and status == host.STATUS_LABEL_RANGE and np.array_equal(got, exp)


# ---- filter -------------------------------------------------------------------------------------------------------------
def filter_grids():
    shape = (5, 6, 4)
    g = VC.conf_grid(1, shape, sentinel=0.45)
    g[0:3, 0:3, 0:3] = 255.0                                 # the window of the corner (0, 0, 0) .. (1, 1, 1): nothing valid
    g[4, 5, 3], g[3, 5, 3], g[4, 4, 3], g[4, 5, 2] = 0.25, 0.5, 255.0, 255.0
    g[3, 4, 3], g[3, 4, 2], g[3, 5, 2], g[4, 4, 2] = 255.0, 255.0, 255.0, 255.0       # corner (4, 5, 3): two valid (even)
    g[0, 5, 0], g[1, 5, 0], g[0, 4, 0], g[1, 4, 0] = 0.75, 255.0, 0.125, 255.0
    g[0, 5, 1], g[1, 5, 1], g[0, 4, 1], g[1, 4, 1] = 0.5, 255.0, 255.0, 255.0          # corner (0, 5, 0): three valid (odd)
    return {"mixed": g, "all valid": VC.conf_grid(2, shape, sentinel=0.0), "none valid": np.full(shape, 255.0, np.float32)}


@pytest.mark.parametrize("op", ["median", "max", "avg"])
def test_filter_against_a_window_loop(op):
    for name, g in filter_grids().items():
        got = host.window_filter(g, op)
        exp = VC.filter_reference(g, op)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), exp.view(np.int32)), (name, op)
    g = filter_grids()["mixed"]
    out = host.window_filter(g, op)
    assert out[0, 0, 0] == 255.0 and out[1, 1, 1] == 255.0
    assert out[4, 5, 3] == {"median": 0.375, "max": 0.5, "avg": 0.375}[op]
    assert out[0, 5, 0] == {"median": 0.5, "max": 0.75}.get(op, out[0, 5, 0])
    assert (host.window_filter(filter_grids()["none valid"], op) == 255.0).all()
    mask = (VC.noise_labels(5, g.shape, p=0.5, classes=3, unknown=0.0) != 0).astype(np.uint8)
    assert np.array_equal(host.window_filter(g, op, mask).view(np.int32), VC.filter_reference(g, op, mask).view(np.int32))


# ---- compose ------------------------------------------------------------------------------------------------------------
def test_compose_views_against_per_segment_painting():
    shape = (6, 5, 4)
    rng = np.random.default_rng(0)
    pan = rng.integers(0, 6, shape).astype(np.int32)          # ids 1 .. 5 in the grid; 5 is in no segment, 9 in no voxel
    sem = rng.integers(0, 21, shape).astype(np.uint8)
    conf = rng.random(shape, dtype=np.float32)
    infos = [{"id": 2, "isthing": True, "category_id": 1, "confidence": 0.25},
             {"id": 1, "isthing": False, "category_id": 9, "confidence": 0.5},
             {"id": 9, "isthing": True, "category_id": 2, "confidence": 0.75},
             {"id": 4, "isthing": True, "category_id": 3, "confidence": 1.0},
             {"id": 3, "isthing": True, "category_id": 3, "confidence": 0.625}]
    seg = viz.frames.segment_table(infos)
    exp = np.zeros(shape, np.uint32)
    for rank, i in ((1, 2), (3, 4), (4, 3)):                  # things in table order: ids 2, 9, 4, 3 -> ranks 1 .. 4
        exp[pan == i] = host.INSTANCE_BASE + rank - 1
    assert np.array_equal(host.compose("mask", shape, panoptic=pan, seg=seg), exp)
    stuff = (exp == 0) & (sem >= 9) & (sem <= 19)
    exp_p = exp.copy()
    exp_p[stuff] = sem[stuff]
    assert np.array_equal(host.compose("panoptic", shape, panoptic=pan, seg=seg, sem=sem), exp_p)
    q = lambda c: int(np.float32(np.float32(np.float32(c) - np.float32(0.25)) / np.float32(0.75)) * np.float32(255.0)
                      + np.float32(0.5))
    exp_i = np.zeros(shape, np.uint32)
    for i, c in ((2, 0.25), (4, 1.0), (3, 0.625)):
        exp_i[pan == i] = 1 + q(c)
    got = host.compose("ins_conf", shape, panoptic=pan, seg=seg, vmin=0.25, vmax=1.0)
    assert np.array_equal(got, exp_i) and got[pan == 2].tolist() == [1] * int((pan == 2).sum()) and (got[pan == 4] == 256).all()
    assert set(np.unique(host.compose("ins_conf", shape, panoptic=pan, seg=seg, vmin=0.5, vmax=0.5))) <= {0, 1}   # vmin == vmax
    sem_g = sem.copy()
    sem_g[0, 0, 0], sem_g[0, 0, 1] = 255, 0
    got = host.compose("semantic", shape, sem=sem_g)
    assert got[0, 0, 0] == 0 and got[0, 0, 1] == 0 and np.array_equal(got[1:], sem_g[1:])
    got = host.compose("vox_conf", shape, sem=sem, conf=conf, vmin=0.0, vmax=1.0)
    assert ((got == 0) == (sem == 0)).all() and got.max() <= 256
    assert got[sem != 0].tolist() == [1 + int(np.float32(c * np.float32(255.0)) + np.float32(0.5)) for c in conf[sem != 0]]


# ---- renderer -----------------------------------------------------------------------------------------------------------
RENDER_CASES = [
    # (grid seed, shape, density, camera, W, H)
    (0, (16, 16, 8), 0.06, "behind", 48, 40),
    (1, (16, 16, 8), 0.25, "oblique", 48, 40),
    (2, (16, 16, 8), 0.06, "down", 37, 23),
    (3, (10, 7, 3), 0.3, "oblique", 37, 23),
    (4, (16, 16, 8), 0.1, "inside", 48, 40),
]


def render_case(seed, shape, p, cam, W, H):
    colour = VC.sparse_colour(seed, shape, p)
    if cam == "inside":                      # in the middle of the grid, looking along +x and slightly down, in an empty voxel
        colour[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 0
        c = viz.camera([shape[0] / 2 + 0.37, shape[1] / 2 + 0.41, shape[2] / 2 + 0.53],
                       [shape[0], shape[1] / 2 - 1.3, 0.7], [0, 0, 1], 70.0, W, H)
    elif cam == "down":                      # the top-down preset moved off the grid's planes: straight down, x up in the image
        c = viz.camera([shape[0] / 2 + 0.31, shape[1] / 2 + 0.23, shape[2] + 30.0], [shape[0] / 2 + 0.31, shape[1] / 2 + 0.23, 0],
                       [1, 0, 0], 40.0, W, H)
    else:
        c = viz.preset(cam, shape, W, H)
    return colour, c


@pytest.mark.parametrize("case", RENDER_CASES, ids=lambda c: f"{c[3]}-{c[1][0]}x{c[1][1]}x{c[1][2]}")
def test_renderer_against_brute_force(case):
    """Hit index and face equal the fp64 brute force on every pixel that is not a near-tie; at most 1 % of the pixels may be
    near-ties (a condition on the case, which the brute force alone decides).  Counted on the CPU, near-ties / pixels / hits:
    behind 16x16x8: 0 / 1920 / 1047; oblique 16x16x8: 2 / 1920 / 1394; down 16x16x8: 0 / 851 / 98;
    oblique 10x7x3: 1 / 851 / 316; inside 16x16x8: 0 / 1920 / 1414."""
    seed, shape, p, cam_name, W, H = case
    colour, cam = render_case(*case)
    hit, face, tie = VC.brute_force(colour, cam, W, H)
    print(f"[{cam_name} {shape}] near-ties {int(tie.sum())} / {W * H}, hits {int((hit >= 0).sum())}")
    assert tie.sum() <= 0.01 * W * H
    assert (hit >= 0).sum() >= 0.1 * W * H and (hit < 0).sum() > 0
    pal = viz.ramp_palette()
    g_hit, g_face, g_rgb, status = host.render(colour, host.bricks(colour), cam, W, H, pal, (200, 228, 256), (9, 8, 7))
    assert status == 0 and g_hit.dtype == np.int32 and g_face.dtype == np.uint8 and g_rgb.dtype == np.uint8
    keep = ~tie
    assert np.array_equal(g_hit[keep], hit[keep])
    assert np.array_equal(g_face[keep].astype(np.int32), face[keep])
    # the pixel is the palette entry of the voxel hit, scaled by the factor of the face's axis; the background on a miss
    f = np.array([200, 228, 256, 256])[np.minimum(g_face >> 1, 3)]
    exp = (pal[colour.reshape(-1)[np.maximum(g_hit, 0)]].astype(np.int32) * f[..., None]) >> 8
    exp[g_hit < 0] = (9, 8, 7)
    assert np.array_equal(g_rgb, exp.astype(np.uint8))


def test_bricks_and_downsample_against_loops():
    for shape in ((16, 16, 8), (10, 7, 3), (32, 32, 4), (1, 1, 1)):
        colour = VC.sparse_colour(7, shape, 0.01)
        nb = host.brick_dims(shape)
        exp = np.zeros(host.brick_words(shape), np.uint32)
        for x, y, z in np.argwhere(colour != 0):
            b = ((x // 8) * nb[1] + y // 8) * nb[2] + z // 8
            exp[b >> 5] |= np.uint32(1 << (b & 31))
        assert np.array_equal(host.bricks(colour), exp)
    rng = np.random.default_rng(0)
    for s in (1, 2, 3):
        img = rng.integers(0, 256, (4 * s, 5 * s, 3)).astype(np.uint8)
        exp = np.zeros((4, 5, 3), np.uint8)
        for j in range(4):
            for i in range(5):
                for c in range(3):
                    exp[j, i, c] = (int(img[j * s:(j + 1) * s, i * s:(i + 1) * s, c].astype(np.int64).sum()) + s * s // 2) // (s * s)
        assert np.array_equal(host.downsample(img, s), exp)


def test_zero_direction_components_and_step_cap():
    """A camera whose rays run exactly along an axis: no step on the other two, a miss when the origin is outside their
    range.  `step_cap` lowers the cap: the ray that needs more steps reports STATUS_STEP_CAP and is a miss."""
    colour = np.zeros((10, 7, 3), np.uint32)
    colour[9, 3, 1] = 5
    colour[0, 0, 0] = 3                                    # off the ray, but its brick is occupied: the ray walks it voxel by voxel
    pal = viz.ramp_palette()
    bits = host.bricks(colour)
    along_x = np.array([-2.0, 3.5, 1.5, 1, 0, 0, 0, 0, 0, 0, 0, 0], np.float32)
    hit, face, rgb, status = host.render(colour, bits, along_x, 1, 1, pal)
    assert status == 0 and hit[0, 0] == (9 * 7 + 3) * 3 + 1 and face[0, 0] == 0
    back = along_x.copy()
    back[0], back[3] = 12.0, -1.0
    hit, face, _, status = host.render(colour, bits, back, 1, 1, pal)
    assert status == 0 and hit[0, 0] == (9 * 7 + 3) * 3 + 1 and face[0, 0] == 1
    outside = along_x.copy()
    outside[1] = 7.0                                       # y == Y: outside [0, Y)
    hit, face, rgb, status = host.render(colour, bits, outside, 1, 1, pal, background=(1, 2, 3))
    assert status == 0 and hit[0, 0] == -1 and face[0, 0] == 255 and rgb[0, 0].tolist() == [1, 2, 3]
    hit, _, _, status = host.render(colour, bits, along_x, 1, 1, pal, step_cap=4)
    assert status == host.STATUS_STEP_CAP and hit[0, 0] == -1
    inside = along_x.copy()
    inside[0] = 9.25                                       # starts inside the occupied voxel: no face was crossed
    hit, face, _, status = host.render(colour, bits, inside, 1, 1, pal)
    assert status == 0 and hit[0, 0] == (9 * 7 + 3) * 3 + 1 and face[0, 0] == host.FACE_INSIDE


# ---- files --------------------------------------------------------------------------------------------------------------
def test_pickle_keys_shapes_and_dtypes(tmp_path):
    rec = VC.synthetic_record()
    path = viz.write_record(str(tmp_path), "000005", 1, rec)
    assert os.path.basename(path) == "000005_1.pkl"
    with open(path, "rb") as f:
        got = pickle.load(f)
    assert tuple(got) == ("ssc_pred", "pred_panoptic_seg", "pred_segments_info", "vox_confidence_denses",
                          "instance_confidence_denses", "xyz", "gt_panoptic_seg", "gt_segments_info", "semantic_label_origin",
                          "instance_label_origin")
    for k, shape, dt in (("ssc_pred", (1, 32, 32, 8), np.int64), ("pred_panoptic_seg", (1, 32, 32, 8), np.int32),
                         ("vox_confidence_denses", (1, 32, 32, 8), np.float32),
                         ("instance_confidence_denses", (1, 32, 32, 8), np.float32), ("xyz", (50, 3), np.float32),
                         ("gt_panoptic_seg", (32, 32, 8), np.int32), ("semantic_label_origin", (32, 32, 8), np.uint8),
                         ("instance_label_origin", (32, 32, 8), np.uint8)):
        assert got[k].shape == shape and got[k].dtype == dt, k
    assert len(got["pred_segments_info"]) == 1 and got["pred_segments_info"][0][3] == \
        {"id": 4, "isthing": False, "category_id": 9, "confidence": float(np.float32(0.7))}
    assert isinstance(got["gt_segments_info"], list)


def test_png_decoded_by_hand(tmp_path):
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (23, 37, 3)).astype(np.uint8)
    path = os.path.join(tmp_path, "a.png")
    viz.write_png(path, img)
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, head = 8, b"", None
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        if kind == b"IDAT":
            idat += body
        pos += 12 + n
    assert head == (37, 23, 8, 2, 0, 0, 0) and kind == b"IEND"
    rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(23, 1 + 37 * 3)
    assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(23, 37, 3), img)
    assert np.array_equal(viz.decode_png(data), img)


def test_palettes():
    pal = viz.label_palette(CONFIG)
    assert pal.shape == (host.INSTANCE_BASE + host.MAX_SEGMENTS, 3) and pal.dtype == np.uint8
    assert pal[1].tolist() == [100, 150, 245] and pal[9].tolist() == [255, 0, 255]      # car, road: the yaml's BGR reversed
    assert len({tuple(c) for c in pal[host.INSTANCE_BASE:]}) == host.MAX_SEGMENTS
    ramp = viz.ramp_palette()
    assert ramp.shape == (257, 3) and ramp[1].tolist() == [24, 32, 120] and ramp[256].tolist() == [200, 24, 24]


def test_command_on_the_host_writes_the_reference_file_names(tmp_path, capsys):
    from pasco_amd.viz.__main__ import main
    src, dst = os.path.join(tmp_path, "out"), os.path.join(tmp_path, "img")
    viz.write_record(src, "000005", 1, VC.synthetic_record())
    main(["--outputs", src, "--config", CONFIG, "--save-folder", dst, "--device", "cpu", "--size", "24", "--supersample", "2",
          "--method", "pasco_single"])
    capsys.readouterr()
    exp = [f"pasco_single_{tag}_000005_{k}_1.png" for k in (1, 2, 4) for tag in ("sem", "sem_gt")]
    exp += [f"pasco_single_{tag}_000005_4_1.png" for tag in ("panop_pred", "mask_pred", "vox_conf", "ins_conf")]
    assert sorted(os.listdir(dst)) == sorted(exp)
    for name in exp:
        img = viz.decode_png(open(os.path.join(dst, name), "rb").read())
        assert img.shape == (24, 24, 3)
        assert (img != 255).any(), name                   # something was drawn
    main(["--outputs", src, "--config", CONFIG, "--save-folder", dst + "2", "--device", "cpu", "--size", "16", "--supersample",
          "1", "--views", "mask", "--scales", "1", "--camera", "top", "--filter", "raw"])
    assert os.listdir(dst + "2") == ["pasco_single_mask_pred_000005_1_1.png"]


def test_step_outputs_are_saved_with_the_ten_keys(tmp_path):
    """`save_step_outputs` on what a step returns (tensors, one entry per output): one pickle per output."""
    import torch
    from pasco_amd.eval.gt import GroundTruth
    shape = (8, 8, 4)
    sem = VC.blob_labels(0, shape, n=6)
    ins = ((sem > 0) & (sem < 9)).astype(np.uint8)
    gt = GroundTruth.from_labels(sem, ins, range(1, 9))
    out = {"panoptic_seg_denses": torch.ones((1,) + shape, dtype=torch.int64),
           "segments_infos": [[{"id": 1, "isthing": True, "category_id": 1, "confidence": 0.5, "all_class_probs": torch.zeros(20)}]],
           "ins_uncertainty_denses": torch.zeros((1,) + shape), "ssc_confidence": torch.rand(shape)}
    probs = torch.rand((20,) + shape)
    paths = viz.save_step_outputs(str(tmp_path), "000010", [out, out], [probs, probs], gt, sem, torch.from_numpy(ins))
    assert [os.path.basename(p) for p in paths] == ["000010_0.pkl", "000010_1.pkl"]
    with open(paths[1], "rb") as f:
        rec = pickle.load(f)
    assert tuple(rec) == viz.KEYS and rec["ssc_pred"].shape == (1,) + shape and rec["pred_panoptic_seg"].dtype == np.int32
    assert np.array_equal(rec["ssc_pred"][0], probs.argmax(0).numpy()) and rec["xyz"].shape == (0, 3)
    assert isinstance(rec["pred_segments_info"][0][0]["all_class_probs"], np.ndarray)
    assert np.array_equal(rec["gt_panoptic_seg"], gt.panoptic.reshape(shape).numpy())
    assert [s["id"] for s in rec["gt_segments_info"]] == gt.seg_id.tolist()
    assert np.array_equal(rec["semantic_label_origin"], sem) and np.array_equal(rec["instance_label_origin"], ins)
    list(viz.frame_images(rec, viz.HostOps(viz.label_palette(CONFIG), viz.ramp_palette()), "m", "000010", 1, size=8,
                          supersample=1, scales=(1, 2)))
