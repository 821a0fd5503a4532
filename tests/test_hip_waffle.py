"""The point-feature kernels on the MI355X (include/pasco_waffle.h, csrc/waffle.hip) against the restatement
(pasco_amd/waffle/host.py, itself pinned to independent references in test_waffle_cpu.py): every integer equal, every float
the same fp32 bits where the kernel's operation order is the restatement's, every float tensor within the bound of
tests/waffle_cases.py against fp64, inputs never written, nothing written past the end of an output (guard entries behind
each one).  Then both golden nets end to end on the torch fallback and on the split-precision product route, the extraction
command, and scoring with the features computed on the device."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import waffle_cases as WC  # noqa: E402
from pasco_amd.waffle import WaffleNet, host, prep  # noqa: E402
from waffle_device import DEV, DeviceOps, dev  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.waffle.lib import waffle_lib
    return waffle_lib()


@pytest.fixture(scope="module")
def ops(lib):
    return DeviceOps(lib)


# ---- decisions: bit-exact ---------------------------------------------------------------------------------------------------
def test_voxel_keys(ops):
    WC.check_voxel(ops)


def test_crop_on_the_device(hip):
    def mask(pc):
        d = dev(pc)
        keep = torch.ones(pc.shape[0], dtype=torch.bool, device=DEV)
        for a in range(3):
            keep &= (d[:, a] > torch.tensor(np.float32(WC.FOV[0][a] + prep.EPS), device=DEV)) & \
                    (d[:, a] < torch.tensor(np.float32(WC.FOV[1][a] - prep.EPS), device=DEV))
        return keep.cpu().numpy()
    WC.check_crop(mask)


def test_cells_and_csr(ops):
    WC.check_cells(ops)


@pytest.mark.parametrize("name", list(WC.search_cases()))
def test_search_equals_all_pairs_and_the_restatement(ops, name):
    WC.check_search(ops, names=(name,))
    xyz, h = WC.search_cases()[name]
    if xyz.shape[0] <= 700:                                  # and the restatement's own walk gives the same lists
        g, start, order = WC.build_search(WC.HostOps(), xyz, h)
        assert np.array_equal(ops.knn(xyz, start, order, g, 5), host.knn(xyz, start, order, g, 5))


@pytest.mark.parametrize("net,scan", [("c256", "synth"), ("c256", "mini"), ("c32", "mini")])
def test_preparation_equals_the_restatement(lib, net, scan):
    cfg = WC.settings(net)
    pc = prep.input_features(WC.scan(scan), cfg["input_feat"])
    pc = prep.augment(pc, prep.tta_params(0, 5, 1) if net == "c32" else None)
    h = prep.prepare_host(pc, cfg)
    d = prep.prepare_device(pc, cfg, DEV)
    assert np.array_equal(d["kept"].cpu().numpy(), h["kept"]) and np.array_equal(d["feat"].cpu().numpy(), h["feat"])
    for (c, s, o, shape), (hc, hs, ho, hshape) in zip(d["cells"], h["cells"]):
        assert tuple(shape) == tuple(hshape)
        assert np.array_equal(c.cpu().numpy(), hc) and np.array_equal(s.cpu().numpy(), hs) and np.array_equal(o.cpu().numpy(), ho)
    assert np.array_equal(d["knn"].cpu().numpy(), h["knn"]) and np.array_equal(d["upsample"].cpu().numpy(), h["upsample"])
    if net == "c256":                                        # no augmentation: the reference's recorded preparation
        g = WC.gold()
        assert np.array_equal(pc[h["kept"]], g[f"{scan}_pc"])
        assert np.array_equal(np.stack([c[0].cpu().numpy() for c in d["cells"]]), g[f"{scan}_c256_cell_ind"])


# ---- float kernels ------------------------------------------------------------------------------------------------------------
def test_flatten_inflate(ops):
    WC.check_flatten_inflate(ops, bitwise_to_host=True)


def test_dwconv3x3(ops):
    WC.check_dwconv(ops, bitwise_to_host=True)


def test_neigh_rows_and_group_max(ops):
    WC.check_neigh(ops, bitwise_to_host=True)


def test_argument_checks(lib):
    f = torch.zeros((8, 8), dtype=torch.float32, device=DEV)
    w, b = torch.zeros((9, 8), dtype=torch.float32, device=DEV), torch.zeros(8, dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="pw_dwconv3x3"):
        lib.dwconv3x3(f, 2, 4, w, b, False, out=f)
    xyz = torch.zeros((10, 3), dtype=torch.float32, device=DEV)
    g = host.SearchGrid((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
    start = torch.tensor([0, 10], dtype=torch.int32, device=DEV)
    order = torch.arange(10, dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError, match="pw_knn"):
        lib.knn(xyz, start, order, g, 10)                    # k must be below n
    with pytest.raises(RuntimeError, match="pw_knn"):
        lib.knn(xyz, start, order, g, 33)
    with pytest.raises(RuntimeError, match="pw_grid_cells"):
        lib.grid_cells(xyz, host.SearchGrid((0.0, 0.0, 0.0), 1.0, (1 << 12, 1 << 12, 2)), lib.new_status(DEV))


# ---- the nets end to end ------------------------------------------------------------------------------------------------------
def golden_inputs(lib, net, scan):
    g = WC.gold()
    grids = WC.settings(net)["grids"]
    status = lib.new_status(DEV)
    cells = []
    for c, shape in zip(g[f"{scan}_{net}_cell_ind"], grids):
        cell = dev(c.astype(np.int32))
        start, order = lib.cells_build(cell, shape[0] * shape[1], status)
        cells.append((cell, start, order, tuple(shape)))
    assert int(status.item()) == 0
    return dev(g[f"{scan}_pc"][:, 3:]), cells, dev(g[f"{scan}_neigh"][1:].T.astype(np.int32))


@pytest.mark.parametrize("route", ["torch below MIN_ROWS_LINEAR", "product route"])
@pytest.mark.parametrize("scan", WC.SCANS)
@pytest.mark.parametrize("net", WC.NETS)
def test_golden_nets_within_the_bound(lib, net, scan, route):
    """N is 1103 and 500: below `fused.MIN_ROWS_LINEAR`, so the default call takes the torch fallback for every product;
    `min_rows=1` sends the same products through ph_conv_fwd's split-precision route (the 5-input and 19-output products, whose
    shapes that route does not take, through its exact fp32 kernel)."""
    from pasco_amd.graph import fused
    model = WaffleNet(WC.state(net), WC.settings(net)["grids"], DEV)
    feat, cells, knn = golden_inputs(lib, net, scan)
    assert feat.shape[0] < fused.MIN_ROWS_LINEAR
    out = model.forward(feat, cells, knn, min_rows=None if route.startswith("torch") else 1)
    torch.cuda.synchronize(DEV)
    worst = []
    for name, got, ref in zip(("embedding", "tokens", "logits"), out, WC.ref64(net, scan)):
        e = WC.err(got.cpu().numpy(), ref)
        print(f"{net} {scan} {route} {name}: error {e:.3e} (bound {WC.BOUND:.3e})")
        worst.append(e)
    assert max(worst) <= WC.BOUND, worst


def test_above_the_row_threshold_the_default_call_takes_the_product_route(lib):
    """17 000 points of the synthetic scan's kind: N >= MIN_ROWS_LINEAR, the default call.  fp64 comes from ref64 directly."""
    import waffle_ref64 as R
    from pasco_amd.graph import fused
    rng = np.random.default_rng(77)
    n = fused.MIN_ROWS_LINEAR + 616
    xyz = np.stack([rng.uniform(-49, 49, n), rng.uniform(-49, 49, n), rng.uniform(-2.9, 1.9, n)], 1).astype(np.float32)
    scan = np.concatenate([xyz, rng.random((n, 1), dtype=np.float32)], 1)
    cfg = WC.settings("c32")
    it = prep.prepare_device(prep.input_features(scan, cfg["input_feat"]), cfg, DEV)
    assert it["feat"].shape[0] >= fused.MIN_ROWS_LINEAR
    model = WaffleNet(WC.state("c32"), cfg["grids"], DEV)
    out = model.forward(it["feat"], it["cells"], it["knn"])
    ref = R.forward(WC.state("c32"), cfg["grids"], it["feat"].cpu().numpy(), np.stack([c[0].cpu().numpy() for c in it["cells"]]),
                    it["knn"].cpu().numpy(), torch.float64)
    for name, got, r in zip(("embedding", "tokens", "logits"), out, ref):
        WC.within_bound(got.cpu().numpy(), r.numpy(), f"c32 n={it['feat'].shape[0]} {name}")


# ---- the commands ---------------------------------------------------------------------------------------------------------------
def test_command_on_the_device_and_on_the_host(hip, tmp_path, capsys):
    from pasco_amd.data.semantic_kitti import read_waffleiron_features
    from pasco_amd.waffle.__main__ import main
    ckpt = WC.write_ckpt(os.path.join(tmp_path, "c32.pth"), "c32")
    items = {}
    for device in ("cuda", "cpu"):
        out = os.path.join(tmp_path, device)
        main(["--root", os.path.join(WC.GOLD, "kitti_mini"), "--ckpt", ckpt, "--config", WC.config_path("c32"),
              "--result-folder", out, "--num-votes", "3", "--device", device])
        path = os.path.join(out, "sequences", "08", "seg_feats_tta", "000005.pkl")
        with open(path, "rb") as f:
            items[device] = pickle.load(f)
        xyz, vote, intensity, emb = read_waffleiron_features(path, embedding_index=2)
        assert emb.shape == (500, 32) and vote.shape == (500, 19)
    capsys.readouterr()
    g, c = items["cuda"], items["cpu"]
    scan = WC.mini_scan()
    assert g["embedding"].shape == (3, 32, 500) and np.array_equal(g["coords"], scan) and np.array_equal(c["coords"], scan)
    assert np.allclose(g["vote"].sum(1), 1.0, atol=1e-5)
    WC.within_bound(g["embedding"], c["embedding"], "embedding, device against host")
    WC.within_bound(g["vote"], c["vote"], "vote, device against host")


def test_scoring_with_features_computed_on_the_device(hip, tmp_path):
    """`eval.kitti --features-on-device` on the mini tree with no waffleiron_v2 folder: the C = 256 golden net gives the 19
    votes and the 256 embedding channels net_mini.ckpt takes."""
    import shutil
    from pasco_amd.eval import kitti as E
    root = os.path.join(tmp_path, "mini")
    shutil.copytree(os.path.join(WC.GOLD, "kitti_mini"), root)
    pre = os.path.join(root, "preprocess")
    shutil.rmtree(os.path.join(pre, "waffleiron_v2"))
    wck = WC.write_ckpt(os.path.join(tmp_path, "c256.pth"), "c256")
    ckpt = os.path.join(WC.GOLD, "net_mini.ckpt")
    for device_prep in (False, True):
        ev, _ = E.evaluate(root, pre, ckpt, "08", frames=1, device_prep=device_prep, features="device", waffle_ckpt=wck,
                           waffle_config=WC.config_path("c256"), num_votes=2)
        assert len(ev.tables(step_time=0.0)) > 0
