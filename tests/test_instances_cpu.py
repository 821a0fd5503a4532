"""Instance-label generation on the host (pasco_amd/data/instances.py, data/gen_instances.py) against the grids the
reference's own generator produced (tests/golden/instances_ref.npz, written by make_golden_instances.py), exactly."""
import os
import pickle
import re
import subprocess

import numpy as np
import pytest
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
CONFIG = os.path.join(GOLD, "semantic-kitti.yaml")

from pasco_amd.data import instances as I  # noqa: E402


def fixture_cases():
    g = np.load(os.path.join(GOLD, "instances_ref.npz"))
    return [(str(n), g[f"{n}_grid"], [int(t) for t in g[f"{n}_things"]], g[f"{n}_instance"], g[f"{n}_semantic"])
            for n in g["names"]]


@pytest.mark.parametrize("use_scipy", [None, False])
def test_host_restatement_equals_the_reference_generator(use_scipy):
    cases = fixture_cases()
    assert len(cases) >= 8 and any(e.max() >= 17 for _, _, _, e, _ in cases)
    for name, grid, things, exp_ins, exp_sem in cases:
        ins, sem, info = I.instance_labels_host(grid, things, 8, use_scipy=use_scipy)
        assert ins.dtype == np.int32 and sem.dtype == np.uint8 and ins.shape == grid.shape == sem.shape
        assert np.array_equal(ins, exp_ins), name
        assert np.array_equal(sem, exp_sem), name
        n = int(exp_ins.max())
        assert info["n_instances"] == n and not info["over_uint8"]
        assert np.array_equal(info["sizes"], np.bincount(exp_ins.ravel(), minlength=n + 1)[1:]), name
        assert info["n_unknown"] == int((exp_sem == 255).sum() - (grid == 255).sum()), name


def test_thing_ids_in_another_order_renumber_by_list_position():
    """`cars_order` was generated with thing ids [5, 2, 8, 1]; the same grid under ascending ids holds the same components
    in another numbering, and instance ids follow the position in the list, not the class value."""
    name, grid, things, exp_ins, _ = next(c for c in fixture_cases() if c[0] == "cars_order")
    assert things == [5, 2, 8, 1]
    ins, _, info = I.instance_labels(grid, things)
    assert np.array_equal(ins, exp_ins)
    first_class = [int(grid[ins == i][0]) for i in range(1, info["n_instances"] + 1)]
    assert [things.index(c) for c in first_class] == sorted(things.index(c) for c in first_class)
    asc, _, info2 = I.instance_labels(grid, sorted(things))
    assert info2["n_instances"] == info["n_instances"] and np.array_equal(asc > 0, ins > 0) and not np.array_equal(asc, ins)
    for bad in ([0, 1], [255], [3, 3], list(range(1, 34))):
        with pytest.raises(ValueError):
            I.instance_labels(grid, bad)


def test_corner_rules_of_the_definition():
    """Diagonal contact joins, two classes never join, 7 is dropped and 8 kept, min_size is a parameter."""
    g = np.zeros((4, 4, 4), np.uint8)
    for k in range(4):
        g[k, k, k] = 1                       # a body diagonal: one component of 4
    g[0, 3, 0:4] = 2
    g[1, 3, 0:4] = 3                         # face to face with the 2s
    ins, sem, info = I.instance_labels(g, [1, 2, 3], min_size=4)
    assert info["n_instances"] == 3 and info["sizes"].tolist() == [4, 4, 4] and info["n_dropped"] == 0
    assert np.array_equal(sem, g) and set(ins[g == 1]) == {1} and set(ins[g == 2]) == {2} and set(ins[g == 3]) == {3}
    ins, sem, info = I.instance_labels(g, [1, 2, 3], min_size=5)
    assert info["n_instances"] == 0 and info["n_dropped"] == 3 and info["n_unknown"] == 12
    assert not ins.any() and (sem[g > 0] == 255).all() and (sem[g == 0] == 0).all()
    for shape in ((1, 1, 1), (5, 1, 1), (1, 7, 1), (1, 1, 9)):
        e = np.zeros(shape, np.uint8)
        ins, sem, info = I.instance_labels(e, [1, 2])
        assert not ins.any() and info["n_instances"] == 0 and info["sizes"].size == 0


def test_remap_lut_follows_the_three_rules():
    lut = I.remap_lut(CONFIG)
    lm = yaml.safe_load(open(CONFIG))["learning_map"]
    assert lut.dtype == np.uint8 and lut.size == max(lm) + 100
    assert lut[0] == 0 and lm[0] == 0
    for k in range(1, lut.size):
        v = lm.get(k, 0)
        assert lut[k] == (255 if v == 0 else v), k
    assert lut[10] == 1 and lut[252] == 1 and lut[1] == 255 and lut[40] == 9


def test_semantic_grid_from_raw_voxel_files():
    """The mini tree's voxel files: lookup, then the invalid mask (most significant bit first), then the reshape."""
    vox = os.path.join(GOLD, "kitti_mini", "dataset", "sequences", "08", "voxels")
    lut = I.remap_lut(CONFIG)
    sem = I.semantic_grid(os.path.join(vox, "000005.label"), os.path.join(vox, "000005.invalid"), lut, grid=(64, 64, 16))
    raw = np.fromfile(os.path.join(vox, "000005.label"), np.uint16)
    inv = np.fromfile(os.path.join(vox, "000005.invalid"), np.uint8)
    exp = np.array([255 if (inv[i >> 3] >> (7 - (i & 7))) & 1 else lut[raw[i]] for i in range(0, raw.size, 37)], np.uint8)
    assert sem.shape == (64, 64, 16) and sem.dtype == np.uint8 and np.array_equal(sem.ravel()[::37], exp)
    with pytest.raises(ValueError, match="outside the lookup table"):
        I.semantic_grid_from_raw(np.full(8, lut.size, np.uint16), np.zeros(1, np.uint8), lut, (2, 2, 2))
    with pytest.raises(ValueError, match="voxels"):
        I.semantic_grid_from_raw(raw, inv, lut, (64, 64, 32))


def test_pickle_round_trip_through_the_reader(tmp_path):
    from pasco_amd.data import read_instance_label_pickle
    _, grid, things, exp_ins, exp_sem = next(c for c in fixture_cases() if c[0] == "cars")
    ins, sem, _ = I.instance_labels(grid, things)
    path = os.path.join(tmp_path, "000000_1_1.pkl")
    I.write_instance_pickle(path, ins, sem)
    with open(path, "rb") as f:
        d = pickle.load(f)
    assert sorted(d) == ["instance_labels", "semantic_labels"]
    assert d["instance_labels"].dtype == np.float64 and d["semantic_labels"].dtype == np.float32
    assert d["instance_labels"].shape == grid.shape == d["semantic_labels"].shape
    s, i = read_instance_label_pickle(path)
    assert np.array_equal(s, exp_sem) and np.array_equal(i, exp_ins.astype(np.uint8))
    assert all(np.array_equal(a, b) for a, b in zip(I.as_label_pair(ins, sem), (s, i)))
    I.write_instance_pickle(path, ins, sem, np.uint16)       # KITTI-360: the dtype of the source .npy
    assert pickle.load(open(path, "rb"))["semantic_labels"].dtype == np.uint16
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def _kitti_tree(root, rng, frames=("000000", "000003", "000005", "000010"), grid=(16, 16, 8)):
    """A synthetic SemanticKITTI tree: raw labels drawn from the yaml's keys, blobs of cars, a random invalid mask."""
    lm = yaml.safe_load(open(CONFIG))["learning_map"]
    keys = np.array(sorted(lm), np.uint16)
    vox = os.path.join(root, "dataset", "sequences", "08", "voxels")
    os.makedirs(vox)
    for f in frames:
        raw = keys[rng.integers(0, keys.size, grid)] * (rng.random(grid) < 0.3)
        raw[2:5, 3:6, 1:4] = 10
        raw[9:12, 9:11, 2:4] = 30
        raw.astype(np.uint16).tofile(os.path.join(vox, f + ".label"))
        np.packbits((rng.random(raw.size) < 0.1).astype(np.uint8)).tofile(os.path.join(vox, f + ".invalid"))
    return vox


def test_cli_on_a_synthetic_tree_with_the_host_path(tmp_path, capsys):
    from pasco_amd.data import gen_instances as G
    from pasco_amd.data import read_instance_label_pickle
    rng = np.random.default_rng(5)
    root, out = os.path.join(tmp_path, "kitti"), os.path.join(tmp_path, "pre")
    vox = _kitti_tree(root, rng)
    argv = ["--root", root, "--preprocess-root", out, "--config", CONFIG, "--sequences", "08", "--grid", "16,16,8",
            "--device", "cpu"]
    G.main(argv)
    assert "3 frames in" in capsys.readouterr().out
    d = os.path.join(out, "instance_labels_v2", "08")
    assert sorted(os.listdir(d)) == ["000000_1_1.pkl", "000005_1_1.pkl", "000010_1_1.pkl"]      # 000003 % 5 != 0
    lut = I.remap_lut(CONFIG)
    for f in ("000000", "000005", "000010"):
        sem0 = I.semantic_grid(os.path.join(vox, f + ".label"), os.path.join(vox, f + ".invalid"), lut, grid=(16, 16, 8))
        ins, sem, info = I.instance_labels(sem0, G.KITTI_THING_IDS)
        s, i = read_instance_label_pickle(os.path.join(d, f + "_1_1.pkl"))
        assert np.array_equal(s, sem) and np.array_equal(i, ins.astype(np.uint8)) and info["n_instances"] >= 1
    from pasco_amd.eval.kitti import frames_of
    assert frames_of(out, "08") == frames_of(out, "08", root=root) == ["000000", "000005", "000010"]
    stamp = {f: os.path.getmtime(os.path.join(d, f)) for f in os.listdir(d)}
    G.main(argv)                                           # existing files are skipped
    assert "0 frames in" in capsys.readouterr().out
    assert stamp == {f: os.path.getmtime(os.path.join(d, f)) for f in os.listdir(d)}
    # KITTI-360: the grid as stored, thing ids 1..6, the semantic grid keeps the dtype of the .npy
    lroot = os.path.join(tmp_path, "ssc")
    seq = "2013_05_28_drive_0009_sync"
    os.makedirs(os.path.join(lroot, "labels", seq))
    grid = (rng.integers(0, 19, (16, 16, 8)) * (rng.random((16, 16, 8)) < 0.2)).astype(np.uint16)
    grid[1:4, 1:4, 1:4] = 7          # class 7 is a thing on SemanticKITTI, not here
    grid[8:11, 8:11, 2:5] = 1
    np.save(os.path.join(lroot, "labels", seq, "000042_1_1.npy"), grid)
    G.main(["--kitti360", "--label-root", lroot, "--preprocess-root", out, "--sequences", seq, "--device", "cpu"])
    with open(os.path.join(out, "instance_labels_v2", seq, "000042_1_1.pkl"), "rb") as f:
        d360 = pickle.load(f)
    ins, sem, _ = I.instance_labels(grid.astype(np.uint8), (1, 2, 3, 4, 5, 6))
    assert d360["semantic_labels"].dtype == np.uint16 and d360["instance_labels"].dtype == np.float64
    assert np.array_equal(d360["instance_labels"], ins) and np.array_equal(d360["semantic_labels"], sem)
    assert not ins[1:4, 1:4, 1:4].any() and ins[8:11, 8:11, 2:5].all()


def test_readers_keep_the_file_path_by_default_and_check_the_mode(tmp_path):
    from pasco_amd.data import FrameReader, Kitti360FrameReader
    mini = os.path.join(GOLD, "kitti_mini")
    r = FrameReader(mini, os.path.join(mini, "preprocess"))
    assert r.instances == "file" and r.labels("08", "000005")[0].shape == (64, 64, 16)
    with pytest.raises(ValueError, match="config"):
        FrameReader(mini, os.path.join(mini, "preprocess"), instances="device")
    with pytest.raises(ValueError, match="'file' or 'device'"):
        FrameReader(mini, os.path.join(mini, "preprocess"), instances="gpu")
    m = os.path.join(GOLD, "kitti360_mini")
    with pytest.raises(ValueError, match="'file' or 'device'"):
        Kitti360FrameReader(m, os.path.join(m, "preprocess"), os.path.join(m, "sscbench"), os.path.join(m, "match.txt"),
                            instances="gpu")


def test_library_exports_exactly_the_label_header():
    """As tests/test_abi.py does for ph_*: the pl_* symbols of libpascohip.so are the entry points pasco_label.h declares,
    and the ctypes binding names the same set."""
    from pasco_amd.build import build_hip
    from pasco_amd.data import label_lib as L
    header = open(os.path.join(ROOT, "include", "pasco_label.h")).read()
    declared = set(re.findall(r"PL_FN\((\w+)\)\s*\(", header))
    assert {"abi_version", "last_error", "semantic_grid", "instances", "instances_workspace_bytes"} <= declared
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip(verbose=False)], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TW"}
    assert {s for s in exported if s.startswith("pl_")} == {"pl_" + n for n in declared}
    assert set(L._SIGNATURES) == declared
    assert int(re.search(r"#define PL_ABI_VERSION (\d+)", header).group(1)) == L.PL_ABI_VERSION
    assert int(re.search(r"#define PL_MAX_THINGS (\d+)", header).group(1)) == L.MAX_THINGS
    assert int(re.search(r"#define PL_RECORD (\d+)", header).group(1)) == L.RECORD
