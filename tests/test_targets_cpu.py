"""The host restatement of the training-side targets (pasco_amd/data/semantic_kitti.py `build_train_item` /
`collate_train`, pasco_amd/data/augment.py) against what the reference's `get_individual` returned
(tests/golden/targets_{a,b,c}.npz, tests/golden/make_golden_targets.py).  Everything is integer or boolean: equal means
equal.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pasco_amd.data import semantic_kitti as SK
from pasco_amd.data.augment import random_transformation
from tests import target_cases as tc


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_build_train_item_equals_the_reference(tag):
    fx = tc.fixture(tag)
    item = tc.host_item(fx)
    tc.assert_item_equals_fixture(item, fx)
    batch = SK.collate_train([item], 8)
    assert torch.equal(batch["global_min_Cs"], torch.from_numpy(fx["global_min_Cs"]))
    assert torch.equal(batch["global_max_Cs"], torch.from_numpy(fx["global_max_Cs"]))
    assert list(batch["semantic_label_origin"].shape) == fx["batch_semantic_label_origin_shape"].tolist()
    assert batch["instance_label_origin"].shape == batch["semantic_label_origin"].shape
    for key in ("semantic_label", "instance_label", "mask_label", "mask_label_origin", "in_feats", "in_coords", "Ts", "min_Cs",
                "max_Cs", "xyz", "input_pcd_instance_label", "frame_id", "sequence"):
        assert isinstance(batch[key], list) and len(batch[key]) == 1, key
    for s in (1, 2, 4):
        assert batch["geo_labels"][f"1_{s}"][0] is item["geo_labels"][f"1_{s}"]
        assert batch["sem_labels"][f"1_{s}"][0] is item["sem_labels"][f"1_{s}"]


def test_the_train_fixture_crops_some_rows_and_keeps_some():
    fx = tc.fixture("c")
    uncropped = tc.host_item(fx, crop=False)
    n_all, n_kept = uncropped["in_feat"].shape[0], int(fx["n_in"])
    assert 0 < n_kept < n_all and fx["in_feat"].shape[0] == n_kept
    assert (fx["min_C"] < 0).any()


def test_random_transformation_equals_the_stored_draw():
    fx = tc.fixture("c")
    rng = np.random.RandomState(int(fx["seed"]))
    assert int(rng.randint(0, int(fx["emb_count"]))) == int(fx["emb_index"])       # the reference draws the embedding first
    T = random_transformation(rng, max_angle=float(fx["aug_max_angle"]), flip=True, scale_range=float(fx["aug_scale_range"]),
                              max_translation=fx["aug_max_translation"])
    assert T.dtype == torch.float32 and torch.equal(T, torch.from_numpy(fx["T"]))
    assert np.array_equal(rng.rand(3), fx["crop_u"])
    scale = torch.linalg.norm(T[:3, :3], dim=1)
    assert float(scale.max() - scale.min()) > 0.05                                   # anisotropic


def pooled_labels(sem: torch.Tensor, n_classes: int):
    """The multi-scale labels through one-hot tensors and pooling passes, for the comparison with the integer rules."""
    geo, lab = {}, {}
    occ = torch.where(sem == 255, torch.tensor(255.0), (sem > 0).float())
    occ_known = torch.where(sem == 255, torch.tensor(0.0), occ)
    idx = sem.long()
    idx[sem == 255] = n_classes
    oh = F.one_hot(idx, n_classes + 1).permute(3, 0, 1, 2).float()
    for s in (2, 4):
        g = F.max_pool3d(occ_known[None, None], s, s)[0, 0]
        g[F.avg_pool3d(occ[None, None], s, s)[0, 0] == 255] = 255
        geo[s] = g.to(torch.uint8)
        frac = F.avg_pool3d(oh[None], s, s)[0]
        classes = frac.clone()
        classes[0] = 0
        classes[n_classes] = 0
        best = classes.argmax(0)
        rest = torch.where(frac[n_classes] == 1, 0, 255)
        lab[s] = torch.where(best == 0, rest, best).to(torch.uint8)
    return geo, lab


@pytest.mark.parametrize("n_classes", [20, 19])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_integer_rules_equal_the_pooling_restatement(seed, n_classes):
    g = torch.Generator().manual_seed(seed)
    shape = (16, 8, 24)
    sem = torch.randint(0, n_classes, shape, generator=g).to(torch.uint8)
    r = torch.rand(shape, generator=g)
    sem[r < 0.35] = 0
    sem[r > 0.7] = 255
    sem[:4, :4, :8] = 255                      # whole blocks of unknowns, of empties, and of both
    sem[4:8, :4, :8] = 0
    sem[8:12, :4, :4] = 0
    sem[8:12, :4, 4:8] = 255
    sem[12:16, 4:8, :2] = 3                    # exact ties: two classes with equal counts in the same block
    sem[12:16, 4:8, 2:4] = 2
    geo, lab = SK.multiscale_labels(sem, n_classes)
    pgeo, plab = pooled_labels(sem, n_classes)
    for s in (2, 4):
        assert torch.equal(geo[f"1_{s}"], pgeo[s]) and torch.equal(lab[f"1_{s}"], plab[s])
        assert (lab[f"1_{s}"] == 0).any() and (lab[f"1_{s}"] == 255).any()
    assert lab["1_1"] is sem
    assert torch.equal(geo["1_1"], torch.where(sem == 255, sem, (sem > 0).to(torch.uint8)))


def test_a_frame_without_targets_gives_t_zero():
    sem = torch.full((8, 8, 8), 255, dtype=torch.uint8)
    sem[2:6, 2:6, 2:6] = 0
    ml = SK.mask_targets(sem, torch.zeros_like(sem))
    assert ml["labels"].shape == (0,) and ml["masks"].shape == (0, 8, 8, 8) and ml["masks"].dtype == torch.bool


def test_mask_targets_order_and_first_voxel_class():
    sem = torch.zeros((4, 4, 8), dtype=torch.uint8)
    sem[0] = 12
    sem[1] = 9
    sem[2, :, :4] = 3            # a thing class without an instance id: no entry
    ins = torch.zeros_like(sem)
    ins[3, 2:, :] = 7
    sem[3, 2, 0] = 5             # the class at the first voxel of instance 7, row-major
    sem[3, 3, :] = 6
    ins[1, 0, 0] = 2             # an instance id on a stuff voxel
    ml = SK.mask_targets(sem, ins)
    assert ml["labels"].tolist() == [9, 12, 9, 5]
    assert torch.equal(ml["masks"][0], sem == 9) and torch.equal(ml["masks"][2], ins == 2) and torch.equal(ml["masks"][3], ins == 7)
    assert bool((ml["masks"][0] & ml["masks"][2]).any())


def test_the_long_cases_are_tie_free_and_reach_a_second_trip():
    """tests/target_cases.py `long_cases`: built on the host, held to `assert_tie_free` and to the launch classes they are there
    for (the assertions are in the builder; tests/test_hip_targets.py runs the kernels on them)."""
    cases = tc.long_cases()
    assert [c.name for c in cases] == tc.long_case_names()
    assert all(c.sem.size > tc.MAX_BLOCKS * tc.BLOCK for c in cases) and tc.trips(tc.LONG_FLAT // 4) == 2
    assert cases[1].crop_u is not None and cases[0].crop_u is None and len(cases[0].Ts) == 2
