"""The restatement of the point-feature stage (pasco_amd/waffle/host.py, prep.py, net.py's parameter tree) against references
that share no code with it: the reference's own formulas written out in numpy, all-pairs searches, scipy's cKDTree, fp64, and
the reference's recorded results (tests/golden/waffle*.npz).  No GPU; tests/test_hip_waffle.py holds the kernels to this."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import waffle_cases as WC  # noqa: E402
import waffle_ref64 as R  # noqa: E402
from pasco_amd.waffle import Extractor, WaffleNet, host, prep  # noqa: E402

OPS = WC.HostOps()


# ---- the surface ------------------------------------------------------------------------------------------------------------
def test_library_exports_exactly_the_header_s_pw_entries():
    import re
    import subprocess
    from pasco_amd.build import CSRC, build_hip
    from pasco_amd.waffle import lib as WL
    root = os.path.dirname(HERE)
    header = open(os.path.join(root, "include", "pasco_waffle.h")).read()
    declared = set(re.findall(r"PW_FN\((\w+)\)\s*\(", header))
    assert declared == set(WL._SIGNATURES) and int(re.search(r"#define PW_ABI_VERSION (\d+)", header).group(1)) == WL.PW_ABI_VERSION == 1
    out = subprocess.check_output(["nm", "-D", "--defined-only", build_hip(verbose=False)], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-1].startswith("pw_")}
    assert exported == {"pw_" + n for n in declared}
    assert "getenv(" not in open(os.path.join(CSRC, "waffle.hip")).read()
    for name, value in (("MAX_K", host.MAX_K), ("MAX_FEAT", host.MAX_FEAT), ("STATUS_OFF_GRID", host.STATUS_OFF_GRID),
                        ("STATUS_ORDER", host.STATUS_ORDER), ("STATUS_INDEX", host.STATUS_INDEX),
                        ("STATUS_KEY_RANGE", host.STATUS_KEY_RANGE)):
        assert int(re.search(rf"#define PW_{name} (\d+)", header).group(1)) == value, name


# ---- decisions ------------------------------------------------------------------------------------------------------------
def test_voxel_first_equals_unique():
    WC.check_voxel(OPS)


def test_crop_is_strict_at_eps():
    WC.check_crop(lambda pc: host.crop_mask(pc, WC.FOV, prep.EPS))


def test_cells_and_csr():
    WC.check_cells(OPS)


@pytest.mark.parametrize("name", list(WC.search_cases()))
def test_search_equals_all_pairs(name):
    WC.check_search(OPS, names=(name,))


def test_search_against_ckdtree_as_sets():
    """cKDTree orders by fp64 distances: a point whose k-th and (k+1)-th fp64 distances differ by less than 1e-6 relative may
    be left out, at most 1 % of the points, and the chosen inputs stay within that."""
    from scipy.spatial import cKDTree
    for name in ("n700", "n5000", "cluster denser than a cell", "flat sheet"):
        xyz, h = WC.search_cases()[name]
        g, start, order = WC.build_search(OPS, xyz, h)
        got = host.knn(xyz, start, order, g, WC.K)
        tree = cKDTree(xyz.astype(np.float64))
        dist, idx = tree.query(xyz.astype(np.float64), k=WC.K + 2)
        close = (dist[:, WC.K + 1] - dist[:, WC.K]) < 1e-6 * dist[:, WC.K + 1]
        assert close.mean() <= 0.01, name
        for p in np.nonzero(~close)[0]:
            assert set(got[p].tolist()) == set(idx[p, 1:WC.K + 1].tolist()), (name, p)
        span = xyz.max(0) - xyz.min(0) + np.float32(1.0)                  # queries up to one extent outside on every side
        q = (xyz.min(0) - span + np.random.default_rng(3).random((500, 3)) * 3 * span).astype(np.float32)
        d2, i2 = tree.query(q.astype(np.float64), k=2)
        near = host.nearest(xyz, start, order, g, q)
        ok = (d2[:, 1] - d2[:, 0]) >= 1e-6 * d2[:, 1]
        assert ok.mean() >= 0.99 and np.array_equal(near[ok], i2[ok, 0]), name


@pytest.mark.parametrize("scan", WC.SCANS)
def test_preparation_equals_the_reference(scan):
    g = WC.gold()
    cfg = WC.settings("c32")
    pc = prep.input_features(WC.scan(scan), cfg["input_feat"])
    assert pc.dtype == np.float32
    it = prep.prepare_host(pc, cfg)
    assert np.array_equal(pc[it["kept"]], g[f"{scan}_pc"])                           # content and order of Voxelize + Crop
    assert np.array_equal(np.stack([c[0] for c in it["cells"]]), g[f"{scan}_c32_cell_ind"])
    ref_n, ref_up = g[f"{scan}_neigh"][1:].T, g[f"{scan}_upsample"]
    same = [set(a.tolist()) == set(b.tolist()) for a, b in zip(it["knn"], ref_n)]
    assert np.mean(same) >= 0.99 and (it["upsample"] == ref_up).mean() >= 0.99
    wide = [host.cell_index(pc[it["kept"]], *geo)[0] for geo in prep._grid_geometry(WC.settings("c256"))]   # the published grids
    assert np.array_equal(np.stack(wide), g[f"{scan}_c256_cell_ind"])


def test_augmentation_is_explicit_and_only_for_several_votes():
    p = prep.tta_params(0, 5, 1)
    assert p == prep.tta_params(0, 5, 1) != prep.tta_params(0, 5, 2) and 0.9 <= p["scale"] <= 1.1 and abs(p["theta"]) <= np.pi
    pc = prep.input_features(WC.mini_scan(), ["intensity", "xyz", "radius"])
    assert np.array_equal(prep.augment(pc, None), pc)
    q = prep.augment(pc, {"theta": 0.3, "flip": True, "axis": 1, "scale": 1.05})
    assert np.array_equal(q[:, 3:], pc[:, 3:]) and not np.array_equal(q[:, :3], pc[:, :3])      # features keep the scan's xyz
    r = np.hypot(q[:, 0], q[:, 1]) / np.hypot(pc[:, 0], pc[:, 1])
    assert np.allclose(r, 1.05, rtol=1e-5) and np.allclose(q[:, 2], pc[:, 2] * 1.05, rtol=1e-6)


# ---- floats ---------------------------------------------------------------------------------------------------------------
def test_flatten_inflate():
    WC.check_flatten_inflate(OPS)


def test_dwconv3x3():
    WC.check_dwconv(OPS)


def test_neigh_rows_and_group_max():
    WC.check_neigh(OPS)


def _twin32(net, scan):
    g = WC.gold()
    return [t.numpy() for t in R.forward(WC.state(net), WC.settings(net)["grids"], g[f"{scan}_pc"][:, 3:],
                                         g[f"{scan}_{net}_cell_ind"], g[f"{scan}_neigh"][1:].T, torch.float32)]


@pytest.mark.parametrize("net", WC.NETS)
def test_fp32_twin_of_ref64_equals_the_recorded_reference(net):
    for scan in WC.SCANS:
        rec, step = WC.recorded(net, scan)
        for got, ref in zip(_twin32(net, scan), rec):
            assert np.abs(got[::step] - ref).max() <= 1e-4 * np.abs(ref).max(), (net, scan)


def test_bound_is_twice_the_reference_error():
    worst = 0.0
    for net in WC.NETS:
        for scan in WC.SCANS:
            rec, step = WC.recorded(net, scan)
            worst = max(worst, max(WC.err(a, b[::step]) for a, b in zip(rec, WC.ref64(net, scan))))
    print(f"reference fp32 against ref64: {worst:.4e}")
    assert worst <= WC.REF_ERROR <= 1.01 * worst and WC.BOUND == 2 * WC.REF_ERROR


def _golden_inputs(net, scan, device="cpu"):
    g = WC.gold()
    grids = WC.settings(net)["grids"]
    cells = [(torch.from_numpy(c.astype(np.int64)).to(device), tuple(s)) for c, s in zip(g[f"{scan}_{net}_cell_ind"], grids)]
    return (torch.from_numpy(np.ascontiguousarray(g[f"{scan}_pc"][:, 3:])).to(device), cells,
            torch.from_numpy(g[f"{scan}_neigh"][1:].T.astype(np.int64)).to(device))


@pytest.mark.parametrize("net", WC.NETS)
def test_host_network_within_the_bound(net):
    model = WaffleNet(WC.state(net), WC.settings(net)["grids"], "cpu")
    assert (model.C, model.depth, model.cin, model.classes) == ({"c256": 256, "c32": 32}[net], {"c256": 3, "c32": 7}[net], 5, 19)
    for scan in WC.SCANS:
        feat, cells, knn = _golden_inputs(net, scan)
        with torch.no_grad():
            out = host.forward(model, feat, cells, knn)
        for name, got, ref in zip(("embedding", "tokens", "logits"), out, WC.ref64(net, scan)):
            WC.within_bound(got.numpy(), ref, f"host {net} {scan} {name}")


def test_checkpoint_keys_are_the_reference_s(tmp_path):
    path = WC.write_ckpt(os.path.join(tmp_path, "m.pth"), "c32", module_prefix=True)
    model = WaffleNet.load(path, WC.settings("c32")["grids"], "cpu")
    st = WC.state("c32")
    assert set(model.modules_.state_dict()) == set(st)
    assert tuple(st["embed.conv1.weight"].shape) == (32, 5, 1) and tuple(st["waffleiron.spatial_mix.0.ffn.0.weight"].shape) == (32, 1, 3, 3)
    assert tuple(st["waffleiron.channel_mix.6.scale.weight"].shape) == (32, 1, 1)
    extra = dict(st)
    extra["classif.extra"] = torch.zeros(1)
    with pytest.raises(KeyError, match="unexpected"):
        WaffleNet(extra, WC.settings("c32")["grids"], "cpu")
    less = {k: v for k, v in st.items() if k != "embed.final.bias"}
    with pytest.raises(KeyError, match="missing"):
        WaffleNet(less, WC.settings("c32")["grids"], "cpu")


# ---- the command on the host --------------------------------------------------------------------------------------------------
def test_command_on_the_host_writes_the_reference_s_pickle(tmp_path, capsys):
    from pasco_amd.data.semantic_kitti import read_waffleiron_features
    from pasco_amd.waffle.__main__ import main
    ckpt = WC.write_ckpt(os.path.join(tmp_path, "c32.pth"), "c32")
    out = os.path.join(tmp_path, "waffleiron_v2")
    main(["--root", os.path.join(WC.GOLD, "kitti_mini"), "--ckpt", ckpt, "--config", WC.config_path("c32"), "--result-folder", out,
          "--num-votes", "2", "--device", "cpu", "--half"])
    assert "saved to" in capsys.readouterr().out
    path = os.path.join(out, "sequences", "08", "seg_feats_tta", "000005.pkl")
    with open(path, "rb") as f:
        item = pickle.load(f)
    scan = WC.mini_scan()
    assert tuple(item) == ("embedding", "coords", "vote") and item["embedding"].dtype == np.float16
    assert item["embedding"].shape == (2, 32, scan.shape[0]) and item["vote"].shape == (scan.shape[0], 19)
    assert np.array_equal(item["coords"], scan) and np.allclose(item["vote"].sum(1), 1.0, atol=1e-5)
    xyz, vote, intensity, emb = read_waffleiron_features(path, embedding_index=1)
    assert xyz.shape == (scan.shape[0], 3) and intensity.shape == (scan.shape[0], 1) and emb.shape == (scan.shape[0], 32)


def test_one_vote_is_the_reference_s_result_gathered_through_upsample(tmp_path):
    """One vote means no augmentation: the embedding of the pickle is the recorded reference embedding at upsample."""
    ckpt = WC.write_ckpt(os.path.join(tmp_path, "c32.pth"), "c32")
    item = Extractor(ckpt, WC.config_path("c32"), "cpu", num_votes=1).frame(WC.mini_scan(), 5)
    g = WC.gold()
    ref = WC.ref64("c32", "mini")
    up = g["mini_upsample"]
    WC.within_bound(item["embedding"][0].T, ref[0][up], "pickle embedding")
    prob = torch.softmax(torch.from_numpy(ref[2][up]), dim=1).numpy()
    WC.within_bound(item["vote"], prob, "pickle vote")
