"""Instance-label generation on the MI355X (include/pasco_label.h, csrc/label.hip) against the host restatement
(data/instances.py, itself pinned to the reference's generator in test_instances_cpu.py): every integer equal."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden")
CONFIG = os.path.join(GOLD, "semantic-kitti.yaml")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FULL = (256, 256, 32)


def run_device(grid, things, min_size=8, extra=3):
    """-> (instance, semantic, record, sizes) as host tensors; `sizes` has `extra` entries past the host's count."""
    from pasco_amd.data.instances import instance_labels_host
    from pasco_amd.data.label_lib import label_lib
    exp = instance_labels_host(grid, things, min_size)
    sem = torch.from_numpy(np.ascontiguousarray(grid)).to(DEV)
    ins, out, rec, sizes = label_lib().instances(sem, things, min_size, sizes_cap=exp[2]["n_instances"] + extra)
    torch.cuda.synchronize(DEV)
    assert torch.equal(sem.cpu(), torch.from_numpy(grid)), "the input grid was written"
    return (ins.cpu(), out.cpu(), rec.cpu(), sizes.cpu()), exp


def check(grid, things, min_size=8, what=""):
    """Device == host restatement on both grids, the record and the sizes; returns the host's info."""
    (ins, out, rec, sizes), (e_ins, e_sem, info) = run_device(grid, things, min_size)
    n = info["n_instances"]
    assert rec.tolist() == [n, info["n_dropped"], info["n_unknown"], 0], (what, rec.tolist(), info)
    assert ins.dtype == torch.int32 and out.dtype == torch.uint8
    assert torch.equal(ins, torch.from_numpy(e_ins)), what
    assert torch.equal(out, torch.from_numpy(e_sem)), what
    assert torch.equal(sizes[:n], torch.from_numpy(info["sizes"])), what
    assert not sizes[n:].any(), (what, "entries past the last instance were written")
    return info


def blob_scene(seed, shape=FULL, n=700, classes=20):
    """Seeded boxes ("cars") of classes 0..classes-1 and 255 on a ground sheet: a few hundred thing instances."""
    rng = np.random.default_rng(seed)
    g = np.zeros(shape, np.uint8)
    g[:, :, : max(1, shape[2] // 8)] = 9
    for _ in range(n):
        e = [int(rng.integers(1, 12)), int(rng.integers(1, 8)), int(rng.integers(1, 7))]
        o = [int(rng.integers(0, max(1, s - d + 1))) for s, d in zip(shape, e)]
        g[o[0]:o[0] + e[0], o[1]:o[1] + e[1], o[2]:o[2] + e[2]] = 255 if rng.random() < 0.05 else rng.integers(0, classes)
    return g


def noise_scene(seed, shape=FULL, p=0.3, classes=9):
    rng = np.random.default_rng(seed)
    g = (rng.integers(0, classes, shape) * (rng.random(shape) < p)).astype(np.uint8)
    g[rng.random(shape) < 0.02] = 255
    return g


def snake(shape=FULL, cls=1):
    """A one-voxel-wide path through every tile: along x on every second y row of the bottom layer, joined at alternating
    ends, then (where the grid is taller than one tile) up a column and back across the top layer."""
    g = np.zeros(shape, np.uint8)
    X, Y, Z = shape
    for k, y in enumerate(range(0, Y, 2)):
        g[:, y, 0] = cls
        if y + 2 < Y:
            g[X - 1 if k % 2 == 0 else 0, y + 1, 0] = cls
    if Z > 32:
        g[0, 0, :] = cls
        for k, y in enumerate(range(0, Y, 2)):
            g[:, y, Z - 1] = cls
            if y + 2 < Y:
                g[0 if k % 2 == 0 else X - 1, y + 1, Z - 1] = cls
    return g


def test_every_fixture_grid(hip):
    g = np.load(os.path.join(GOLD, "instances_ref.npz"))
    for n in g["names"]:
        things = [int(t) for t in g[f"{n}_things"]]
        (ins, out, rec, _), _ = run_device(g[f"{n}_grid"], things)
        assert torch.equal(ins, torch.from_numpy(g[f"{n}_instance"])), n        # the reference's own output
        assert torch.equal(out, torch.from_numpy(g[f"{n}_semantic"])), n
        check(g[f"{n}_grid"], things, what=str(n))


@pytest.mark.parametrize("things", [list(range(1, 9)), list(range(1, 7)), [5, 2, 8, 1]])
def test_full_size_blob_scenes(hip, things):
    info = check(blob_scene(11), things, what="blobs")
    assert 100 <= info["n_instances"] <= 2000
    print(f"[blobs {things}] {info['n_instances']} instances, {info['n_dropped']} dropped")


def test_full_size_dense_noise(hip):
    info = check(noise_scene(3), list(range(1, 9)), what="noise")
    assert info["n_dropped"] >= 20000 and info["n_instances"] > 255
    print(f"[noise] {info['n_instances']} instances, {info['n_dropped']} dropped, {info['n_unknown']} voxels unknown")
    check(noise_scene(4, p=0.6, classes=3), [1, 2], what="noise, two big classes")


@pytest.mark.parametrize("shape", [(13, 9, 35), (17, 8, 33), (9, 17, 7), (1, 40, 40), (40, 1, 40), (40, 40, 1), (1, 1, 64),
                                   (1, 1, 1), (3, 5, 2), (64, 64, 16)])
def test_shapes_off_the_tile_and_flat_axes(hip, shape):
    for seed, p, classes in ((0, 0.5, 4), (1, 0.9, 3), (2, 0.2, 9)):
        check(noise_scene(seed, shape, p, classes), [1, 2, 3], min_size=3, what=f"{shape} seed {seed}")


def test_uniform_grids(hip):
    things = list(range(1, 9))
    assert check(np.zeros(FULL, np.uint8), things)["n_instances"] == 0
    assert check(np.full(FULL, 255, np.uint8), things)["n_instances"] == 0
    info = check(np.full(FULL, 3, np.uint8), things, what="one class everywhere")
    assert info["n_instances"] == 1 and info["sizes"].tolist() == [FULL[0] * FULL[1] * FULL[2]]
    assert check(np.full(FULL, 3, np.uint8), [1, 2], what="no thing voxel")["n_instances"] == 0
    assert check(np.full((8, 8, 32), 2, np.uint8), [], what="no thing ids")["n_instances"] == 0


@pytest.mark.parametrize("shape", [FULL, (40, 24, 80)])
def test_snake_through_every_tile_finishes_clean(hip, shape):
    """The worst case of any propagation scheme: one component whose only path visits every tile.  The status word stays
    clean (`check` asserts record[3] == 0) and the whole path is one instance."""
    g = snake(shape)
    info = check(g, [1], what="snake")
    assert info["n_instances"] == 1 and info["sizes"].tolist() == [int((g == 1).sum())]
    g2 = g.copy()
    g2[shape[0] // 2, :, :] = 0                     # cut every row once: many pieces, still exact
    assert check(g2, [1], what="cut snake")["n_instances"] > 1


def test_contacts_across_tile_faces_edges_and_corners(hip):
    """Tiles are 8 x 8 x 32: pairs of voxels that touch only diagonally, across a face, an edge and a corner of a tile."""
    g = np.zeros((24, 24, 96), np.uint8)
    pairs = [((7, 3, 5), (8, 4, 6)), ((3, 7, 40), (4, 8, 41)), ((2, 2, 31), (3, 3, 32)),          # faces
             ((7, 7, 10), (8, 8, 10)), ((7, 12, 31), (8, 12, 32)), ((12, 15, 63), (12, 16, 64)),    # edges
             ((7, 7, 31), (8, 8, 32)), ((15, 15, 63), (16, 16, 64)), ((15, 8, 32), (16, 7, 31)),    # corners
             ((16, 23, 95), (15, 22, 94))]
    for k, (a, b) in enumerate(pairs):
        g[a] = g[b] = 1 + k % 3
    g[20, 20, 20] = 1                                # alone: dropped at min_size 2
    g[7, 20, 50], g[8, 20, 50] = 1, 2                # two classes across a face: never joined
    info = check(g, [1, 2, 3], min_size=2, what="diagonal contacts")
    assert info["n_instances"] == len(pairs) and info["n_dropped"] == 3 and set(info["sizes"].tolist()) == {2}


def test_corners_of_the_grid_and_sizes_around_the_threshold(hip):
    g = np.zeros((20, 20, 40), np.uint8)
    for x in (0, 18):
        for y in (0, 18):
            for z in (0, 38):
                g[x:x + 2, y:y + 2, z:z + 2] = 4
    g[4:11, 10, 30] = 5          # 7 voxels across x = 8: dropped
    g[4:12, 13, 30] = 5          # 8 voxels across x = 8: kept
    g[10, 4:11, 33] = 6          # 7 across y = 8
    g[12, 4:12, 33] = 6          # 8 across y = 8
    g[14, 10, 28:35] = 7         # 7 across z = 32
    g[16, 10, 28:36] = 7         # 8 across z = 32
    info = check(g, [4, 5, 6, 7], what="corners and thresholds")
    assert info["n_instances"] == 8 + 3 and info["n_dropped"] == 3 and info["n_unknown"] == 21
    assert check(g, [4, 5, 6, 7], min_size=7)["n_instances"] == 8 + 6
    assert check(g, [7, 4], min_size=0)["n_instances"] == 10


def test_two_runs_are_bit_equal(hip):
    from pasco_amd.data.label_lib import label_lib
    for g in (noise_scene(8), blob_scene(9)):
        sem = torch.from_numpy(g).to(DEV)
        a = label_lib().instances(sem, list(range(1, 9)), 8, sizes_cap=4096)
        b = label_lib().instances(sem, list(range(1, 9)), 8, sizes_cap=4096)
        torch.cuda.synchronize(DEV)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


def test_api_on_the_device_and_argument_checks(hip):
    from pasco_amd.data import instances as I
    from pasco_amd.data.label_lib import label_lib
    g = blob_scene(5, (40, 40, 16), 60)
    ins, sem, info = I.instance_labels(g, range(1, 9), device=DEV)
    e_ins, e_sem, e_info = I.instance_labels(g, range(1, 9))
    assert ins.is_cuda and torch.equal(ins.cpu(), torch.from_numpy(e_ins)) and torch.equal(sem.cpu(), torch.from_numpy(e_sem))
    assert torch.equal(info["sizes"].cpu(), torch.from_numpy(e_info["sizes"]))
    assert {k: info[k] for k in ("n_instances", "n_dropped", "n_unknown", "over_uint8")} == \
           {k: e_info[k] for k in ("n_instances", "n_dropped", "n_unknown", "over_uint8")}
    d = torch.from_numpy(g).to(DEV)
    for bad in ([0], [255], [2, 2], list(range(1, 34))):
        with pytest.raises((RuntimeError, ValueError), match="pl_instances"):
            label_lib().instances(d, bad)
    with pytest.raises(RuntimeError, match="workspace"):
        label_lib().instances(d, [1], ws=torch.empty(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="min_size"):
        label_lib().instances(d, [1], min_size=-1)


def test_semantic_grid_against_numpy(hip):
    from pasco_amd.data import instances as I
    from pasco_amd.data.label_lib import STATUS_RAW_RANGE, label_lib
    lut = I.remap_lut(CONFIG)
    rng = np.random.default_rng(2)
    for S in (16, 64, 2048 + 8, 64 * 64 * 16):
        raw = rng.integers(0, lut.size, S).astype(np.uint16)
        bits = (rng.random(S) < 0.3).astype(np.uint8)
        bits[[0, 7, S - 8, S - 1]] = [1, 0, 0, 1]               # first and last byte: their outer bits set, inner clear
        raw[[0, 7, S - 8, S - 1]] = 10
        inv = np.packbits(bits)
        exp = I.semantic_grid_from_raw(raw, inv, lut, (S // 8, 4, 2))
        assert exp.ravel()[[0, 7, S - 8, S - 1]].tolist() == [255, 1, 1, 255]
        got = I.semantic_grid_from_raw(raw, inv, lut, (S // 8, 4, 2), device=DEV)
        assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), torch.from_numpy(exp))
        # an unaligned view takes the narrow path
        pad = torch.from_numpy(np.concatenate([np.zeros(1, np.uint16), raw])).to(DEV)
        sem, st = label_lib().semantic_grid(pad[1:], torch.from_numpy(inv).to(DEV), torch.from_numpy(lut).to(DEV))
        assert int(st.item()) == 0 and torch.equal(sem.cpu(), torch.from_numpy(exp.ravel()))
    # a raw value outside the table: reported through the status word, 255 written, nothing read out of bounds
    raw = np.zeros(64, np.uint16)
    raw[13], raw[40], raw[41] = lut.size, 65535, 10
    sem, st = label_lib().semantic_grid(torch.from_numpy(raw).to(DEV), torch.zeros(8, dtype=torch.uint8, device=DEV),
                                        torch.from_numpy(lut).to(DEV))
    assert int(st.item()) == STATUS_RAW_RANGE
    exp = np.zeros(64, np.uint8)
    exp[13], exp[40], exp[41] = 255, 255, 1
    assert torch.equal(sem.cpu(), torch.from_numpy(exp))
    with pytest.raises(ValueError, match="outside the lookup table"):
        I.semantic_grid_from_raw(raw, np.zeros(8, np.uint8), lut, (4, 4, 4), device=DEV)


def test_scoring_from_cli_pickles_and_from_the_device_is_identical(hip, tmp_path, capsys):
    """The mini SemanticKITTI tree (with cars and people drawn into its voxel labels): pickles written by the CLI on the
    device and on the host are the same files, and `eval.kitti` prints the same tables from them and with
    `instances="device"`, which needs no pickle directory at all."""
    from pasco_amd.data import gen_instances as G
    from pasco_amd.data import read_instance_label_pickle
    from pasco_amd.eval import kitti as E
    root = os.path.join(tmp_path, "mini")
    shutil.copytree(os.path.join(GOLD, "kitti_mini"), root)
    pre = os.path.join(root, "preprocess")
    shutil.rmtree(os.path.join(pre, "instance_labels_v2"))
    label = os.path.join(root, "dataset", "sequences", "08", "voxels", "000005.label")
    raw = np.fromfile(label, np.uint16).reshape(64, 64, 16)
    raw[4:60, 6:58, 0:2] = 40                       # road
    raw[20:28, 20:30, 5:10] = 10                    # a car
    raw[40:44, 30:33, 5:8] = 30                     # a person
    raw[40:44, 33:36, 5:8] = 31                     # a bicyclist touching the person: another class, another instance
    raw[50, 50, 5:9] = 10                           # a car of 4 voxels: dropped
    raw.tofile(label)
    common = ["--root", root, "--config", CONFIG, "--sequences", "08", "--grid", "64,64,16"]
    G.main(common + ["--preprocess-root", pre])
    host_pre = os.path.join(tmp_path, "host_pre")
    G.main(common + ["--preprocess-root", host_pre, "--device", "cpu"])
    capsys.readouterr()
    rel = os.path.join("instance_labels_v2", "08", "000005_1_1.pkl")
    with open(os.path.join(pre, rel), "rb") as a, open(os.path.join(host_pre, rel), "rb") as b:
        assert a.read() == b.read()
    sem, ins = read_instance_label_pickle(os.path.join(pre, rel))
    assert ins.max() >= 3 and (sem[50, 50, 5:9] == 255).all() and sem[22, 22, 6] == 1
    ckpt = os.path.join(GOLD, "net_mini.ckpt")
    ev_file, _ = E.evaluate(root, pre, ckpt, "08")
    bare = os.path.join(tmp_path, "no_pickles")         # the point features only
    shutil.copytree(os.path.join(pre, "waffleiron_v2"), os.path.join(bare, "waffleiron_v2"))
    ev_dev, _ = E.evaluate(root, bare, ckpt, "08", instances="device", config=CONFIG, grid=(64, 64, 16))
    assert ev_file.tables(step_time=0.0) == ev_dev.tables(step_time=0.0)
    with pytest.raises(FileNotFoundError):
        E.evaluate(root, bare, ckpt, "08")              # the default still wants the pickles
    E.main(["--root", root, "--preprocess-root", bare, "--ckpt", ckpt, "--instances-on-device", "--config", CONFIG,
            "--grid", "64,64,16", "--frames", "1"])
    assert "car" in capsys.readouterr().out
