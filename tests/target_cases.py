"""Cases and checks for the training targets, shared by tests/test_targets_cpu.py (host restatement against the reference's
fixtures) and tests/test_hip_targets.py (pt_* kernels against the host restatement).  Every comparison is exact.

A case is a pair of label grids, one transform per subnet and, optionally, one crop draw per subnet.  The device computes
`transform_coords` by an fmaf chain, the host by torch's CPU matmul; the two may differ where a value sits on a .5 rounding
tie, and a case with such a sample would measure the host, not the kernel.  `assert_tie_free` therefore
holds every case to two conditions, checked on the CPU when the case is built:

  1. for transforms the builder chooses: in fp64, no coordinate of any sample under T or T^-1 lies within 1e-3 of a tie;
  2. for every case: the exact emulation of the chain (tests/frame_ref.py `ref_transform`) and the host's `transform_coords`
     give the same integer for every sample under T and T^-1.

Condition 1 cannot hold for the fixture frames b and c: their transforms are fixed by the fixture (a 17 degree rotation, a
random draw) and spread ~2 x 10^5 fractional parts evenly, so some hundreds lie within 1e-3 of a tie whatever the seed.
They are held to condition 2, which is the property condition 1 is a sufficient margin for."""
import os
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from pasco_amd.data import semantic_kitti as SK
from tests import frame_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KITTI360_THING_IDS = (1, 2, 3, 4, 5, 6)
_FIXTURES = {}


def fixture(tag: str):
    if tag not in _FIXTURES:
        _FIXTURES[tag] = dict(np.load(os.path.join(GOLDEN, f"targets_{tag}.npz")))
    return _FIXTURES[tag]


def host_item(fx, crop: bool = True):
    """`build_train_item` on a fixture's frame, with the fixture's transform, embedding index and crop draw."""
    coords, emb = fx["in_coords"], fx["in_emb"][int(fx["emb_index"])].T
    u = fx["crop_u"] if (crop and "crop_u" in fx) else None
    return SK.build_train_item(coords[:, :3], fx["in_vote"], coords[:, 3:], emb, fx["in_sem"], fx["in_ins"],
                               torch.from_numpy(fx["T"]), 8, fx["in_plab"].reshape(-1, 1) & 0xFFFF, crop_u=u)


def _eq(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.shape == want.shape, f"{what}: shape {got.shape}, the reference has {want.shape}"
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} values differ"


def unpack_masks(fx, key):
    shape = tuple(int(v) for v in fx[key + "_shape"])
    return np.unpackbits(fx[key + "_bits"])[:int(np.prod(shape))].reshape(shape).astype(bool)


def assert_item_equals_fixture(item, fx, points: bool = True):
    keys = ["min_C", "max_C", "semantic_label", "instance_label", "semantic_label_origin", "instance_label_origin"]
    if points:
        keys += ["in_feat", "in_coord", "T", "xyz", "input_pcd_instance_label"]
    for k in keys:
        _eq(item[k], fx[k], k)
    for s in (1, 2, 4):
        _eq(item["geo_labels"][f"1_{s}"], fx[f"geo_1_{s}"], f"geo_labels 1_{s}")
        _eq(item["sem_labels"][f"1_{s}"], fx[f"sem_1_{s}"], f"sem_labels 1_{s}")
    for k in ("mask_label", "mask_label_origin"):
        _eq(item[k]["labels"], fx[k + "_labels"], k + " labels")
        _eq(item[k]["masks"], unpack_masks(fx, k), k + " masks")
        assert item[k]["masks"].dtype == torch.bool


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    sem: np.ndarray
    ins: np.ndarray
    Ts: Sequence[torch.Tensor]
    crop_u: Optional[np.ndarray]        # [M, 3] or None
    thing_ids: tuple
    n_classes: int
    chosen: bool                        # the builder chose the transforms (condition 1 applies)


def lattice_T(flip_y=False, quarter_turns=0, scale=(1.0, 1.0, 1.0), shift_voxels=(0.0, 0.0, 0.0)) -> torch.Tensor:
    """A transform whose fractional parts stay away from ties: quarter turns about z, a y flip, scales with few binary digits
    and a translation in voxels (0.2 m)."""
    c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][quarter_turns % 4]
    R = np.identity(4)
    R[:2, :2] = [[c, -s], [s, c]]
    R[:3, 3] = np.asarray(shift_voxels, np.float64) * 0.2
    F = np.identity(4)
    if flip_y:
        F[1, 1] = -1
    S = np.diag(list(scale) + [1.0])
    return torch.from_numpy(S).float() @ torch.from_numpy(R).float() @ torch.from_numpy(F).float()


def tie_report(sem: np.ndarray, T: torch.Tensor):
    """-> (samples within 1e-3 of a tie in fp64, samples where the exact chain and the host's matmul disagree), both over
    the known voxels under T and the box samples under T^-1."""
    sites = np.argwhere(sem != 255).astype(np.int64)
    Tinv = torch.inverse(T)
    mb = np.array([0.0, -25.6, -2.0], np.float32).astype(np.float64)
    near = differ = 0
    pts, mat = sites, T
    for step in range(2):
        M64 = mat.double().numpy()
        p = pts.astype(np.float64) * 0.2 + 0.1 + mb
        q = (p @ M64[:3, :3].T + M64[:3, 3] - mb - 0.1) / 0.2
        near += int((np.abs(np.abs(q - np.floor(q)) - 0.5) < 1e-3).any(axis=1).sum())
        chain = frame_ref.ref_transform(pts, [mat.numpy()], True)[0][0]
        host = SK.transform_coords(torch.from_numpy(pts), mat).long().numpy()
        differ += int((chain != host).any(axis=1).sum())
        if step == 0:
            lo, hi = host.min(0), host.max(0)
            axes = [np.arange(lo[d], hi[d] + 1, dtype=np.int64) for d in range(3)]
            pts, mat = np.stack([g.ravel() for g in np.meshgrid(*axes, indexing="ij")], 1), Tinv
    return near, differ


def assert_tie_free(case: Case):
    for m, T in enumerate(case.Ts):
        near, differ = tie_report(case.sem, T)
        assert differ == 0, f"{case.name}[{m}]: {differ} samples where the fmaf chain and the host's matmul round differently"
        if case.chosen:
            assert near == 0, f"{case.name}[{m}]: {near} samples within 1e-3 of a .5 tie"


def _scene(shape, seed, instances=True, thing=(1, 6)):
    """A small labelled frame: unknown border, a ground sheet, mixed stuff, an unknown pocket, two things."""
    rng = np.random.default_rng(seed)
    X, Y, Z = shape
    sem = np.full(shape, 255, np.uint8)
    sem[1:X - 1, 2:Y - 1, 1:Z] = 0
    sem[1:X - 1, 2:Y - 1, 1:3] = 9
    mix = rng.random(shape) < 0.3
    mix[:, :, :3] = False
    mix[:, :, 5:] = False
    sem[mix & (sem != 255)] = rng.integers(9, 19, shape, dtype=np.uint8)[mix & (sem != 255)]
    sem[X // 2:X // 2 + 3, Y // 2:Y // 2 + 3, 2:6] = 255
    ins = np.zeros(shape, np.uint8)
    if instances:
        sem[2:5, 3:7, 3:6] = thing[0]
        ins[2:5, 3:7, 3:6] = 1
        sem[X - 6:X - 3, Y - 6:Y - 2, 3:5] = thing[1]
        ins[X - 6:X - 3, Y - 6:Y - 2, 3:5] = 2
        ins[6:8, 3:5, 1:3] = 3                      # an instance id on ground voxels
    return sem, ins


def _fixture_case(tag):
    fx = fixture(tag)
    u = fx["crop_u"].reshape(1, 3) if "crop_u" in fx else None
    return Case("fixture_" + tag, fx["in_sem"], fx["in_ins"], [torch.from_numpy(fx["T"])], u, SK.SEMANTIC_KITTI_THING_IDS, 20,
                chosen=(tag == "a"))


def _many_targets():
    """More than 128 targets: 135 instance ids and a few stuff classes."""
    sem, ins = _scene((32, 32, 8), 5, instances=False)
    k = 1
    for x in range(2, 30, 2):
        for y in range(3, 29, 2):
            if k <= 135:
                sem[x, y, 4] = 1 + k % 8
                ins[x, y, 4] = k
                k += 1
    assert k == 136
    return sem, ins


def build_cases():
    KI = SK.SEMANTIC_KITTI_THING_IDS
    eye = lattice_T()
    turn = lattice_T(flip_y=True, quarter_turns=1, shift_voxels=(3.0, -2.0, 1.0))
    stretch = lattice_T(scale=(1.25, 0.75, 1.0), shift_voxels=(0.25, 0.25, 0.0))          # drops and duplicates source voxels
    back = lattice_T(quarter_turns=2, shift_voxels=(-5.0, 4.0, -2.0))                     # the box starts at negative coordinates
    sem, ins = _scene((24, 20, 8), 1)
    cases = [_fixture_case("a"), _fixture_case("b"), _fixture_case("c")]
    cases.append(Case("m3", sem, ins, [eye, turn, stretch], None, KI, 20, True))
    cases.append(Case("m3_crop", sem, ins, [eye, turn, stretch], np.array([[0.3, 0.6, 0.1], [0.0, 0.0, 0.5], [0.999, 0.999, 0.5]]),
                      KI, 20, True))
    s2, i2 = _scene((16, 16, 8), 2, instances=False)
    cases.append(Case("no_instances", s2, i2, [stretch], None, KI, 20, True))
    cases.append(Case("no_instances_crop", s2, i2, [turn], np.array([[0.5, 0.5, 0.5]]), KI, 20, True))
    i3 = np.zeros_like(s2)
    i3[:, :, 6:] = 255                                # ids {0 only}: "no label" 255 above, so id 0 decides where samples survive
    cases.append(Case("instance_ids_zero_only", s2, i3, [eye], None, KI, 20, True))
    s4 = np.full((16, 16, 8), 255, np.uint8)
    s4[9, 3, 5] = 12
    cases.append(Case("single_known_voxel", s4, np.zeros_like(s4), [turn], None, KI, 20, True))
    cases.append(Case("negative_box", sem, ins, [back], np.array([[0.0, 0.0, 0.0]]), KI, 20, True))
    s5 = np.full((16, 16, 8), 255, np.uint8)
    s5[2:8, 1:15, 0:8] = 0
    s5[2:8, 1:15, 1] = 10
    s5[3:5, 3:6, 2:4] = 2
    i5 = np.zeros_like(s5)
    i5[3:5, 3:6, 2:4] = 9
    cases.append(Case("scene_size_8", s5, i5, [eye], None, KI, 20, True))                 # x 2..7 and z 0..7 -> scene 8
    s6, i6 = _scene((24, 20, 8), 3, thing=(2, 6))
    assert s6[s6 != 255].max() == 18                   # 19 classes: 0..18
    cases.append(Case("kitti360_classes", s6, i6, [turn, eye], None, KITTI360_THING_IDS, 19, True))
    sm, im = _many_targets()
    cases.append(Case("many_targets", sm, im, [eye], None, KI, 20, True))
    return cases


_CASES = None


def cases():
    """The case list, built and held to `assert_tie_free` once."""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
        for c in _CASES:
            assert c.sem.shape[0] <= 64 and c.sem.shape[1] <= 64 and c.sem.shape[2] <= 16
            assert_tie_free(c)
    return _CASES


# ---- past the first trip of the capped grids --------------------------------------------------------------------------------
# Every case above is at most 64 x 64 x 16 voxels = 256 workgroups, so no grid-stride loop of csrc/target.hip has taken a
# second trip.  These are kept out of `cases()` and its size assertion, in a list with its own.
MAX_BLOCKS, BLOCK, WAVES = 2048, 256, 4          # csrc/target.hip: the grid cap, the threads and the waves of a workgroup
LONG_GRID = (128, 128, 36)
LONG_FLAT = 4 * (MAX_BLOCKS * BLOCK + 257)       # voxels of the synthetic pt_masks / pt_presence arrays: a multiple of 4


# !! `trips` restates the grid arithmetic of pasco_amd/csrc/target.hip (`grid_for`, and k_labels' one wave per 4^3 block).  It
# !! is used to CHOOSE sizes and to assert that the long cases reach a second trip of every capped grid - never to form an
# !! expected value: those are the host restatement's and numpy's.
def trips(work: int, per_block: int = BLOCK) -> int:
    blocks = min(max(-(-work // per_block), 1), MAX_BLOCKS)
    return -(-work // (blocks * per_block))


def build_long_cases():
    KI = SK.SEMANTIC_KITTI_THING_IDS
    turn = lattice_T(flip_y=True, quarter_turns=1, shift_voxels=(3.0, -2.0, 1.0))          # `turn` of build_cases
    sem, ins = _scene(LONG_GRID, 7)
    # The crop keeps 0.8 of the scene in x and y, which takes k_labels back under its cap: the second trip of k_labels is the
    # uncropped case's, the second trip of k_crop_bounds (over the sample box, which no crop shrinks) the cropped one's.
    return [Case("second_trip", sem, ins, [lattice_T(), turn], None, KI, 20, True),
            Case("second_trip_crop", sem, ins, [turn], np.array([[0.3, 0.6, 0.1]]), KI, 20, True)]


_LONG_CASES = None


def long_cases():
    """The long cases, built, held to `assert_tie_free` and to their launch classes once."""
    global _LONG_CASES
    if _LONG_CASES is None:
        _LONG_CASES = build_long_cases()
        assert_tie_free(_LONG_CASES[0])             # the second case has the same grid and one of the same transforms
        for c in _LONG_CASES:
            assert c.sem.shape == LONG_GRID and trips(c.sem.size) > 1, "k_box, k_samples, k_crop_bounds: a second trip"
            assert trips(LONG_FLAT // 4) > 1 >= trips(c.sem.size // 4), "k_masks takes its second trip on the synthetic arrays alone"
        for h in host_targets(_LONG_CASES[0]):
            scene = tuple(h["semantic_label"].shape)
            assert trips(scene[0] * scene[1] * scene[2] // 64, WAVES) > 1, f"k_labels: a second trip (scene {scene})"
            assert trips(scene[0] * scene[1] * scene[2]) > 1, "k_presence: a second trip"
        h = host_targets(_LONG_CASES[1])[0]
        assert h["semantic_label"].numel() < host_targets(_LONG_CASES[0])[1]["semantic_label"].numel(), "the crop acts"
    return _LONG_CASES


def long_case_names():
    return ["second_trip", "second_trip_crop"]


def case_names():
    return ["fixture_a", "fixture_b", "fixture_c", "m3", "m3_crop", "no_instances", "no_instances_crop", "instance_ids_zero_only",
            "single_known_voxel", "negative_box", "scene_size_8", "kitti360_classes", "many_targets"]


def case(name: str) -> Case:
    if name in long_case_names():
        return {c.name: c for c in long_cases()}[name]
    return {c.name: c for c in cases()}[name]


_HOST = {}


def host_targets(c: Case):
    """The host restatement's targets of a case, one item per subnet (computed once, shared, never modified)."""
    if c.name not in _HOST:
        xyz = np.array([[1.0, -20.0, 0.0]], np.float32)
        one = np.zeros((1, 1), np.float32)
        _HOST[c.name] = [SK.build_train_item(xyz, one, one, one, c.sem, c.ins, T, 8, None,
                                             crop_u=None if c.crop_u is None else c.crop_u[m], thing_ids=c.thing_ids,
                                             n_classes=c.n_classes) for m, T in enumerate(c.Ts)]
    return _HOST[c.name]


# ---- one training step on a train_batch dict ---------------------------------------------------------------------------
def mini_step(batch, dev, q: int = 8, width: int = 16, seed: int = 0):
    """A mini net of pasco_amd.me modules on subnet 0 of a `train_batch` dict: a stem convolution on the voxelised points, two
    strided convolutions, a semantic head per scale and a mask head with `q` queries; `compute_sem_compl_loss` on the three
    scales plus `SetCriterion` on the mask targets; backward.  -> (loss, [(name, parameter)])."""
    import pasco_amd.me as ME
    from pasco_amd.grad import criterion as crit
    from pasco_amd.grad.semloss import compute_sem_compl_loss
    torch.manual_seed(seed)
    min_c, sem = batch["min_Cs"][0], batch["semantic_label"][0]
    coords, feats = batch["in_coords"][0].to(dev), batch["in_feats"][0].to(dev)
    lo = min_c.to(dev).long()
    hi = lo + torch.tensor(sem.shape, device=dev)
    inside = ((coords >= lo) & (coords < hi)).all(dim=1)           # rows the label grids cover
    coords, feats = coords[inside], feats[inside]
    uc, inv = torch.unique(coords, dim=0, return_inverse=True)      # one row per voxel: the sum of its points
    rows = torch.zeros((uc.shape[0], feats.shape[1]), device=dev).index_add_(0, inv, feats)
    c4 = torch.cat([torch.zeros((uc.shape[0], 1), dtype=uc.dtype, device=dev), uc], 1).to(torch.int32)

    class Mini(torch.nn.Module):
        def __init__(self, cin):
            super().__init__()
            self.stem = ME.MinkowskiConvolution(cin, width, kernel_size=3, bias=True, dimension=3)
            self.down2 = ME.MinkowskiConvolution(width, width, kernel_size=2, stride=2, bias=True, dimension=3)
            self.down4 = ME.MinkowskiConvolution(width, width, kernel_size=2, stride=2, bias=True, dimension=3)
            self.heads = torch.nn.ModuleDict({str(s): torch.nn.Linear(width, 20) for s in (1, 2, 4)})
            self.mask = torch.nn.Linear(width, q)
            self.query_logits = torch.nn.Parameter(torch.randn(1, q, 21) * 0.1)

        @staticmethod
        def on(x, f):
            return ME.SparseTensor(features=f, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)

        def forward(self, x):
            x1 = self.stem(x)
            x2 = self.down2(x1)
            x4 = self.down4(x2)
            sem_logits = {s: [self.on(t, self.heads[str(s)](t.F))] for s, t in ((1, x1), (2, x2), (4, x4))}
            return sem_logits, {"voxel_logits": self.on(x1, self.mask(x1.F)), "query_logits": self.query_logits}

    net = Mini(int(rows.shape[1])).to(dev).train()
    sem_logits, outputs = net(ME.SparseTensor(features=rows * 0.01, coordinates=c4))
    freq = {f"1_{s}": np.ones(20) for s in (1, 2, 4)}
    ce, lovasz = compute_sem_compl_loss(batch["sem_labels"], sem_logits, batch["min_Cs"], batch["max_Cs"], freq)
    criterion = crit.SetCriterion(20, crit.HungarianMatcher(1, 1, 1), {"loss_ce": 1.0, "loss_mask": 40.0, "loss_dice": 1.0}, 0.1,
                                  [torch.ones(21, device=dev)], torch.ones(20)).to(dev)
    unknown = (batch["geo_labels"]["1_1"][0] == 255)[None]
    losses = criterion(None, outputs, [batch["mask_label"][0]], None, unknown, 0, None, min_c)
    loss = ce + lovasz + losses["loss_ce"] + losses["loss_mask"] + losses["loss_dice"]
    loss.backward()
    return loss.detach(), list(net.named_parameters())
