"""The training-target kernels on libpascohip.so (csrc/target.hip, include/pasco_target.h) against the host restatement
`build_train_item`, on the cases of tests/target_cases.py; the three fixture frames also against what the reference returned.
Every output is uint8, int32 or bool: every comparison is `torch.equal`.  The CPU side is tests/test_targets_cpu.py."""
import os
import pickle

import numpy as np
import pytest
import torch

from pasco_amd.data import semantic_kitti as SK
from tests import target_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


def device_targets(c: tc.Case, dev, origin_masks=False):
    from pasco_amd.data.targets import prepare_targets
    sem, ins = torch.from_numpy(c.sem).to(dev), torch.from_numpy(c.ins).to(dev)
    return prepare_targets(sem, ins, c.Ts, thing_ids=c.thing_ids, n_classes=c.n_classes, crop_u=c.crop_u, origin_masks=origin_masks)


def assert_same(got, want, what):
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)}, the host has {want.dtype} {tuple(want.shape)}"
    assert torch.equal(got, want), f"{what}: {int((got != want).sum())} of {want.numel()} values differ"


@pytest.mark.parametrize("name", tc.case_names() + tc.long_case_names())
def test_device_targets_equal_the_host_restatement(dev, name):
    c = tc.case(name)
    host = tc.host_targets(c)
    got = device_targets(c, dev, origin_masks=True)
    assert len(got) == len(host) == len(c.Ts)
    for m, (g, h) in enumerate(zip(got, host)):
        for k in ("min_C", "max_C", "semantic_label", "instance_label"):
            assert_same(g[k], h[k], f"{name}[{m}] {k}")
        for s in (1, 2, 4):
            assert_same(g["geo_labels"][f"1_{s}"], h["geo_labels"][f"1_{s}"], f"{name}[{m}] geo 1_{s}")
            assert_same(g["sem_labels"][f"1_{s}"], h["sem_labels"][f"1_{s}"], f"{name}[{m}] sem 1_{s}")
        assert g["sem_labels"]["1_1"] is g["semantic_label"]
        ml = g["mask_label"]
        assert_same(ml["labels"], h["mask_label"]["labels"], f"{name}[{m}] labels")
        assert not dict.__contains__(ml, "masks") and "masks" in ml and ml.keys() == ["labels", "masks"] and len(ml) == 2
        assert_same(ml["masks"], h["mask_label"]["masks"], f"{name}[{m}] masks")
        assert dict.__contains__(ml, "masks") and ml.get("masks") is ml["masks"] and [k for k, _ in ml.items()] == ["labels", "masks"]
    mo = got[0]["mask_label_origin"]
    assert_same(mo["labels"], host[0]["mask_label_origin"]["labels"], f"{name} origin labels")
    assert_same(mo["masks"], host[0]["mask_label_origin"]["masks"], f"{name} origin masks")


def test_the_cases_cover_what_they_are_named_for():
    """Properties of the host's targets that make the cases discriminating (no kernel involved)."""
    assert len(tc.case("m3").Ts) == 3
    h = tc.host_targets(tc.case("no_instances"))[0]
    assert not bool(h["instance_label"].any()) and h["mask_label"]["labels"].numel() > 0
    assert tc.case("instance_ids_zero_only").ins.max() == 255 and set(np.unique(tc.case("instance_ids_zero_only").ins)) == {0, 255}
    h = tc.host_targets(tc.case("single_known_voxel"))[0]
    assert int((h["semantic_label"] != 255).sum()) >= 1 and h["mask_label"]["labels"].tolist() == [12]
    assert bool((tc.host_targets(tc.case("negative_box"))[0]["min_C"] < 0).any())
    assert 8 in tuple(tc.host_targets(tc.case("scene_size_8"))[0]["semantic_label"].shape)
    assert tc.case("kitti360_classes").n_classes == 19 and tc.case("kitti360_classes").thing_ids == tc.KITTI360_THING_IDS
    assert tc.case("m3_crop").crop_u[1, :2].tolist() == [0.0, 0.0] and tc.case("m3_crop").crop_u[2, :2].tolist() == [0.999, 0.999]
    assert tc.host_targets(tc.case("many_targets"))[0]["mask_label"]["labels"].numel() > 128
    for name in ("m3_crop", "fixture_c"):                   # the crop changes the targets
        c = tc.case(name)
        un = SK.build_train_item(np.array([[1.0, -20.0, 0.0]], np.float32), np.zeros((1, 1), np.float32), np.zeros((1, 1), np.float32),
                                 np.zeros((1, 1), np.float32), c.sem, c.ins, c.Ts[0], 8, None, thing_ids=c.thing_ids)
        assert un["semantic_label"].shape != tc.host_targets(c)[0]["semantic_label"].shape or \
            not torch.equal(un["semantic_label"], tc.host_targets(c)[0]["semantic_label"])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_device_targets_equal_the_reference_fixture(dev, tag):
    fx = tc.fixture(tag)
    g = device_targets(tc.case("fixture_" + tag), dev, origin_masks=True)[0]
    item = dict(g, semantic_label_origin=torch.from_numpy(fx["in_sem"]), instance_label_origin=torch.from_numpy(fx["in_ins"]))
    tc.assert_item_equals_fixture(item, fx, points=False)


@pytest.mark.parametrize("name", ["fixture_b", "fixture_c", "m3", "instance_ids_zero_only", "single_known_voxel", "negative_box",
                                  "second_trip"])
def test_resample_bounds_equal_pf_label_bounds(dev, name):
    """(e) The box and the union of the semantic-only and instance-only bounds of pt_resample are pf_label_bounds' words."""
    from pasco_amd.data.frame_lib import box_upper_bound, frame_lib
    from pasco_amd.data.target_lib import BOUNDS, target_lib
    c = tc.case(name)
    sem, ins = torch.from_numpy(c.sem).to(dev), torch.from_numpy(c.ins).to(dev)
    Ts = [T.float() for T in c.Ts]
    Tinv = [torch.inverse(T) for T in Ts]
    ub = box_upper_bound(tuple(sem.shape), Ts)
    want = frame_lib().label_bounds(sem, ins, Ts, Tinv, ub).cpu()
    stride = int((ub[:, 3:] - ub[:, :3] + 1).long().prod(dim=1).max())
    sb = torch.empty((len(Ts), stride), dtype=torch.uint8, device=dev)
    ib = torch.empty_like(sb)
    bounds = torch.empty((len(Ts), BOUNDS), dtype=torch.int32, device=dev)
    target_lib().resample(sem, ins, Ts, Tinv, ub, sb, ib, bounds)
    b = bounds.cpu()
    assert torch.equal(b[:, :6], want[:, :6])
    assert torch.equal(torch.minimum(b[:, 6:9], b[:, 12:15]), want[:, 6:9])
    assert torch.equal(torch.maximum(b[:, 9:12], b[:, 15:18]), want[:, 9:12])
    assert bool((b[:, :3] >= ub[:, :3]).all()) and bool((b[:, 3:6] <= ub[:, 3:]).all())


def _rows(g, dev, seed=0):
    """Voxel rows over a subnet's scene, a few of them outside the grid; an unknown grid."""
    gen = torch.Generator().manual_seed(seed)
    shape = torch.tensor(g["semantic_label"].shape)
    n = 700
    xyz = (torch.rand((n, 3), generator=gen) * shape).long() + g["min_C"].long()
    xyz[:5] = g["min_C"].long() - 1
    xyz[5:9] = g["min_C"].long() + shape
    xyz[9] = g["min_C"].long() + shape - 1
    coords = torch.cat([torch.zeros((n, 1), dtype=torch.long), xyz], 1).to(torch.int32).to(dev)
    return coords, 9


@pytest.mark.parametrize("name", ["fixture_a", "fixture_c", "m3_crop", "kitti360_classes", "no_instances", "second_trip",
                                  "second_trip_crop"])
@pytest.mark.parametrize("with_unknown", [False, True])
def test_pack_equals_pack_targets_of_the_materialised_masks(dev, name, with_unknown):
    """(f) words, flags and oob, bit for bit; rows outside the grid included."""
    from pasco_amd.grad.criterion import pack_targets
    for g in device_targets(tc.case(name), dev):
        coords, n_out = _rows(g, dev)
        unknown = (g["geo_labels"]["1_1"] == 255) if with_unknown else None
        origin = g["min_C"].tolist()
        got = g["mask_label"].pack(coords, unknown, origin)
        assert not dict.__contains__(g["mask_label"], "masks"), "pack must not build the masks"
        want = pack_targets(g["mask_label"]["masks"], unknown, coords, origin)
        assert got.t == want.t == g["mask_label"]["labels"].numel() > 0
        assert torch.equal(got.tbits, want.tbits) and torch.equal(got.flags, want.flags) and torch.equal(got.oob, want.oob)
        assert int(got.oob) == n_out
        words = got.tbits.cpu().long() & 0xFFFFFFFF
        bits = sum(((words[:, j:j + 1] >> torch.arange(32)) & 1).sum(1) for j in range(4))
        if name in ("fixture_a", "fixture_c", "m3_crop"):
            assert int(bits.max()) <= 2
    stuff_and_instance = device_targets(tc.case("fixture_a"), dev)[0]
    sem, ins = stuff_and_instance["semantic_label"], stuff_and_instance["instance_label"]
    both = torch.nonzero((sem == 9) & (ins == 3))
    assert both.shape[0] > 0
    c = torch.cat([torch.zeros((both.shape[0], 1), dtype=torch.long, device=dev), both + stuff_and_instance["min_C"].to(dev)], 1)
    p = stuff_and_instance["mask_label"].pack(c.to(torch.int32), None, stuff_and_instance["min_C"].tolist())
    w = p.tbits.cpu().long() & 0xFFFFFFFF
    assert all(bin(int(w[r, 0])).count("1") == 2 for r in range(w.shape[0])), "a stuff voxel with an instance id carries two bits"


def test_more_than_128_targets_masks_are_correct_and_pack_raises(dev):
    c = tc.case("many_targets")
    g = device_targets(c, dev)[0]
    h = tc.host_targets(c)[0]
    assert g["mask_label"]["labels"].numel() > 128
    assert_same(g["mask_label"]["masks"], h["mask_label"]["masks"], "masks")
    coords, _ = _rows(g, dev)
    with pytest.raises(ValueError, match="at most"):
        g["mask_label"].pack(coords, None, g["min_C"].tolist())


def _flat_labels(seed=11):
    """Synthetic uint8 label arrays of tc.LONG_FLAT voxels (host): classes and instance ids whose first voxel lies in every trip
    of a capped grid, one class and one id in the last, partial wave alone."""
    n = tc.LONG_FLAT
    rng = np.random.default_rng(seed)
    sem = rng.choice(np.array([0, 255, 3, 9, 14], np.uint8), n, p=[0.4, 0.1, 0.2, 0.2, 0.1])
    ins = rng.choice(np.array([0, 1, 7], np.uint8), n, p=[0.9, 0.05, 0.05])
    trip = tc.MAX_BLOCKS * tc.BLOCK
    for k in range(1, -(-n // trip)):                 # a class and an id that appear first in trip k
        at = k * trip + 100 * k + 3
        sem[at:] = np.where(sem[at:] == (3 if k == 1 else 19 + k), 20 + k, sem[at:])
        ins[at + 5::97] = 100 + k
    sem[n - 2], ins[n - 1] = 77, 200                  # the last wave of the last trip: 4 voxels
    assert n % 64 == 4 and n % 4 == 0 and tc.trips(n) == 5 and tc.trips(n // 4) == 2
    return sem, ins


def test_masks_on_a_second_trip_equal_numpy(dev):
    """pt_masks strides over n / 4 words under the grid cap: its second trip needs more than 4 x 2048 x 256 voxels."""
    from pasco_amd.data.target_lib import target_lib
    sem, ins = _flat_labels()
    t = 3
    cls_slot, ins_slot = np.full(256, -1, np.int32), np.full(256, -1, np.int32)
    cls_slot[9], cls_slot[24], ins_slot[7] = 0, 1, 2       # class 24 exists in the second trip alone, 9 and id 7 everywhere
    got = target_lib().masks(torch.from_numpy(sem).to(dev), torch.from_numpy(ins).to(dev), torch.from_numpy(cls_slot).to(dev),
                             torch.from_numpy(ins_slot).to(dev), t)
    assert got.dtype == torch.bool and tuple(got.shape) == (t, tc.LONG_FLAT)
    cs, is_ = cls_slot[sem], ins_slot[ins]
    want = np.stack([(cs == k) | (is_ == k) for k in range(t)])
    assert all(want[k].any() and not want[k].all() for k in range(t))
    assert want[:, 4 * tc.MAX_BLOCKS * tc.BLOCK:].any(axis=1).all(), "every target has voxels in the second trip"
    assert np.array_equal(got.cpu().numpy(), want), f"{int((got.cpu().numpy() != want).sum())} of {want.size} mask voxels differ"


def test_presence_on_later_trips_equals_numpy(dev):
    """pt_presence over five trips of its capped grid, the last of one partial wave: the class flags, the first index of every
    instance id and the class found there."""
    from pasco_amd.data.target_lib import TABLE, target_lib
    sem, ins = _flat_labels()
    table = torch.full((TABLE,), -5, dtype=torch.int32, device=dev)
    target_lib().presence(torch.from_numpy(sem).to(dev), torch.from_numpy(ins).to(dev), table)
    got = table.cpu().numpy()
    flags = np.zeros(256, np.int32)
    flags[np.unique(sem[(sem != 0) & (sem != 255)])] = 1
    first = np.full(256, np.iinfo(np.int32).max, np.int64)
    ids, at = np.unique(ins, return_index=True)          # the first occurrence of every value
    first[ids], first[0] = at, np.iinfo(np.int32).max
    cls = np.where(first == np.iinfo(np.int32).max, 0, sem[np.minimum(first, len(sem) - 1)])
    assert flags[77] == 1 and flags[[21, 22, 23, 24]].all() and first[200] == len(sem) - 1 and (first[[101, 102, 103, 104]] < len(sem)).all()
    assert np.array_equal(got[:256], flags), "class flags"
    assert np.array_equal(got[256:512], first.astype(np.int32)), "first index of every instance id"
    assert np.array_equal(got[512:], cls.astype(np.int32)), "class at the first index"


def _criterion_inputs(g, dev, q=12, seed=3):
    import pasco_amd.me as ME
    sem = g["semantic_label"]
    xyz = torch.nonzero(sem != 255)[::3]
    coords = torch.cat([torch.zeros((xyz.shape[0], 1), dtype=torch.long, device=dev), xyz + g["min_C"].to(dev)], 1).to(torch.int32)
    gen = torch.Generator().manual_seed(seed)
    f = (torch.randn((coords.shape[0], q), generator=gen) * 2).to(dev).requires_grad_(True)
    ql = torch.randn((1, q, 21), generator=gen).to(dev).requires_grad_(True)
    return {"voxel_logits": ME.SparseTensor(features=f, coordinates=coords), "query_logits": ql}, f, ql


@pytest.mark.parametrize("name", ["fixture_a", "fixture_c"])
def test_criterion_is_the_same_with_target_masks_and_with_a_plain_dict(dev, name):
    """(g) identical losses, matches and gradients."""
    from pasco_amd.grad import criterion as crit
    g = device_targets(tc.case(name), dev)[0]
    weights = {"loss_ce": 1.0, "loss_mask": 40.0, "loss_dice": 1.0}
    criterion = crit.SetCriterion(20, crit.HungarianMatcher(1, 1, 1), weights, 0.1, [torch.ones(21, device=dev)], torch.ones(20)).to(dev)
    unknown = (g["geo_labels"]["1_1"] == 255)[None]
    results = []
    for kind in ("lazy", "plain"):
        ml = device_targets(tc.case(name), dev)[0]["mask_label"]
        target = ml if kind == "lazy" else {"labels": ml["labels"], "masks": ml["masks"]}
        assert hasattr(target, "pack") == (kind == "lazy")
        outputs, f, ql = _criterion_inputs(g, dev)
        losses = criterion(None, outputs, [target], None, unknown, 0, None, g["min_C"])
        if kind == "lazy":
            assert not dict.__contains__(ml, "masks"), "the criterion must not build the masks of a TargetMasks"
        total = losses["loss_ce"] + losses["loss_mask"] + losses["loss_dice"]
        total.backward()
        results.append(([losses[k].detach().clone() for k in ("loss_ce", "loss_mask", "loss_dice")], criterion.matched[0][0],
                        f.grad.clone(), ql.grad.clone()))
    (la, ma, fa, qa), (lb, mb, fb, qb) = results
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and all(bool(torch.isfinite(a)) for a in la)
    assert torch.equal(ma[0], mb[0]) and torch.equal(ma[1], mb[1]) and ma[0].numel() > 0
    assert torch.equal(fa, fb) and torch.equal(qa, qb) and bool(fa.any())


def write_fixture_frame(fx, root, seq="08", frame="000007"):
    """The fixture's frame in the reference's on-disk layout -> (dataset root, preprocess root)."""
    pre = os.path.join(root, "preprocess")
    for d in (os.path.join(root, "dataset", "sequences", seq, "labels"), os.path.join(pre, "instance_labels_v2", seq),
              os.path.join(pre, "waffleiron_v2", "sequences", seq, "seg_feats_tta")):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(pre, "instance_labels_v2", seq, f"{frame}_1_1.pkl"), "wb") as f:
        pickle.dump({"semantic_labels": fx["in_sem"], "instance_labels": fx["in_ins"]}, f)
    with open(os.path.join(pre, "waffleiron_v2", "sequences", seq, "seg_feats_tta", frame + ".pkl"), "wb") as f:
        pickle.dump({"embedding": fx["in_emb"], "coords": fx["in_coords"], "vote": fx["in_vote"]}, f)
    fx["in_plab"].tofile(os.path.join(root, "dataset", "sequences", seq, "labels", frame + ".label"))
    return root, pre


def test_train_batch_on_the_device_equals_the_host_and_the_reference(dev, tmp_path):
    fx = tc.fixture("c")
    root, pre = write_fixture_frame(fx, str(tmp_path))
    reader = SK.FrameReader(root, pre)
    T, u, e = torch.from_numpy(fx["T"]), fx["crop_u"], int(fx["emb_index"])
    host = reader.train_batch("08", "000007", [T], crop_u=[u], embedding_index=e)
    got = reader.train_batch("08", "000007", [T], crop_u=[u], embedding_index=e, device=dev)
    assert sorted(got.keys()) == sorted(host.keys())
    assert_same(got["in_feats"][0], host["in_feats"][0], "in_feats")
    assert_same(got["in_coords"][0], host["in_coords"][0], "in_coords")
    assert got["in_feats"][0].shape[0] == int(fx["n_in"])
    for k in ("global_min_Cs", "global_max_Cs", "semantic_label_origin", "instance_label_origin"):
        assert_same(got[k], host[k], k)
    item = {k: got[k][0] for k in ("semantic_label", "instance_label", "mask_label", "mask_label_origin")}
    item.update(min_C=got["min_Cs"][0], max_C=got["max_Cs"][0], in_feat=got["in_feats"][0], in_coord=got["in_coords"][0], T=got["Ts"][0],
                xyz=got["xyz"][0], input_pcd_instance_label=got["input_pcd_instance_label"][0],
                semantic_label_origin=got["semantic_label_origin"][0], instance_label_origin=got["instance_label_origin"][0],
                geo_labels={k: v[0] for k, v in got["geo_labels"].items()}, sem_labels={k: v[0] for k, v in got["sem_labels"].items()})
    tc.assert_item_equals_fixture(item, fx)


def test_one_training_step_from_train_batch(dev, tmp_path):
    """(h) train_batch on the train fixture -> a mini net of pasco_amd.me modules -> compute_sem_compl_loss + SetCriterion ->
    backward: the loss is finite and every parameter has a gradient."""
    fx = tc.fixture("c")
    root, pre = write_fixture_frame(fx, str(tmp_path))
    batch = SK.FrameReader(root, pre).train_batch("08", "000007", [torch.from_numpy(fx["T"])], crop_u=[fx["crop_u"]],
                                                  embedding_index=int(fx["emb_index"]), device=dev)
    loss, params = tc.mini_step(batch, dev)
    assert bool(torch.isfinite(loss)) and float(loss) > 0
    for name, p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name


@pytest.mark.parametrize("name", ["m3_crop", "fixture_c", "second_trip", "second_trip_crop"])
def test_two_runs_give_the_same_bytes(dev, name):
    """(i)"""
    c = tc.case(name)
    runs = []
    for _ in range(2):
        out = device_targets(c, dev, origin_masks=True)
        coords, _ = _rows(out[0], dev)
        p = out[0]["mask_label"].pack(coords, None, out[0]["min_C"].tolist())
        flat = [p.tbits, p.flags, p.oob]
        for g in out:
            flat += [g["semantic_label"], g["instance_label"], g["mask_label"]["labels"], g["mask_label"]["masks"]]
            flat += list(g["geo_labels"].values()) + list(g["sem_labels"].values())
        runs.append([t.cpu().numpy().tobytes() for t in flat])
    assert runs[0] == runs[1]
