"""The reference of tests/frame_ref.py tied to what the project already trusts (no GPU): the host restatements
`build_item` / `build_item_kitti360` / `transform_coords` / `transformed_labels` on the case clouds and grids of
tests/frame_edge_cases.py, and the reference project's recorded items under tests/golden.  Every builder of the case table
runs here too, so each case's claim about what it hits is checked without a GPU."""
import os

import numpy as np
import pytest
import torch

from tests import frame_edge_cases as cases
from tests import frame_ref as ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TIE_SHARE_MAX = 1e-3                     # near-tie entries are the only ones left out against the host, at most 0.1 %
LABELS = cases.labels((12, 10, 8), "random")


def bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(cases.bits(a), cases.bits(b))


@pytest.mark.parametrize("name,build", cases.POINT_BUILDERS, ids=[n for n, _ in cases.POINT_BUILDERS])
def test_points_cases_claims_and_host(name, build):
    """Each builder asserts its own claim (mask, branches, special rows); the clouds in one of the two dataset layouts are
    also run through that dataset's host restatement: features bit for bit, voxel indices through `transform_coords`."""
    from pasco_amd.data.kitti360 import build_item_kitti360
    from pasco_amd.data.semantic_kitti import build_item
    case = build()
    feat, voxel, src, K = ref.ref_points(case.pts, case.args)
    assert feat.shape == (K, 7 + sum(s.shape[1] for s in list(case.args.pre) + list(case.args.post))) and voxel.shape == (K, 3)
    if case.host is None:
        return
    sem, ins = LABELS
    if case.host == "kitti360":
        item = build_item_kitti360(case.pts, sem, ins)
    else:
        vote, inten, emb = case.args.pre[0], case.args.pre[1], case.args.post[0]
        plab = np.arange(case.pts.shape[0], dtype=np.int32)[:, None]
        item = build_item(case.pts[:, :3], vote, inten, emb, sem, ins, None, 8, plab)
        assert np.array_equal(item["input_pcd_instance_label"].numpy().ravel(), src)
    assert bit_equal(item["in_feat"].numpy(), feat), name
    to, _, near = ref.ref_transform(voxel, [np.eye(4, dtype=np.float32)], False)
    assert not near.any() and np.array_equal(item["in_coord"].numpy(), to[0]), name
    assert np.array_equal(to[0], voxel.astype(np.int64))


def test_flag_cloud_claims():
    cases.flag_claims()


def test_real_size_cloud_against_build_item():
    from pasco_amd.data.semantic_kitti import build_item
    case = cases.real_size()
    feat, voxel, src, K = ref.ref_points(case.pts, case.args)
    item = build_item(case.pts[:, :3], case.args.pre[0], case.args.pre[1], case.args.post[0], *LABELS)
    assert feat.shape[1] == 283 and bit_equal(item["in_feat"].numpy(), feat)


def _against_items(g, tags, feat, voxel):
    """The bit-exact `in_feat` comparison is what ties `ref_points` to the recorded items.  The `in_coord` comparison adds
    little on them: the recorded transforms include half-voxel shifts, so a large share of the coordinates (printed by the
    callers, not bounded) sits within one ulp of a tie and is excused; `test_transform_against_the_host` is the bounded check."""
    ties = total = 0
    for tag in tags:
        assert bit_equal(g[f"{tag}_in_feat"], feat), tag
        to, _, near = ref.ref_transform(voxel, [g[f"{tag}_T"]], False)
        bad = to[0] != g[f"{tag}_in_coord"]
        assert not (bad & ~near[0]).any(), tag
        ties += int(near.sum())
        total += near.size
    return ties, total


def test_points_against_the_recorded_kitti360_items():
    g = np.load(os.path.join(GOLD, "kitti360_items.npz"))
    pc = np.fromfile(os.path.join(GOLD, "kitti360_mini", "data_3d_raw", "2013_05_28_drive_0009_sync", "velodyne_points", "data",
                                  "0000000137.bin"), np.float32).reshape(-1, 4)
    feat, voxel, _, K = ref.ref_points(pc, cases.k360_args(pc))
    assert 0 < K < pc.shape[0]
    ties, total = _against_items(g, [str(t) for t in g["tags"]], feat, voxel)
    print(f"[kitti360 items] {ties} of {total} coordinates near a tie (the recorded transforms include half-voxel shifts)")


def test_points_against_the_recorded_semantic_kitti_items():
    from pasco_amd.data.semantic_kitti import read_waffleiron_features
    g = np.load(os.path.join(GOLD, "io_items.npz"))
    path = os.path.join(GOLD, "kitti_mini", "preprocess", "waffleiron_v2", "sequences", "08", "seg_feats_tta", "000005.pkl")
    ties = total = 0
    for tag in ("eye", "rigid"):
        xyz, vote, inten, emb = read_waffleiron_features(path, embedding_index=int(g[f"{tag}_emb_index"]))
        pts = np.concatenate([xyz, inten], 1).astype(np.float32)
        assert np.array_equal(pts[:, :3], xyz)
        feat, voxel, _, K = ref.ref_points(pts, cases.sk_args(pts, vote, emb))
        assert feat.shape[1] == 283 and K > 0
        t, n = _against_items(g, [tag], feat, voxel)
        ties, total = ties + t, total + n
    print(f"[semantic kitti items] {ties} of {total} coordinates near a tie")


def test_fmaf_is_exact_against_rationals():
    """The error-free sum against Python's exact rationals, on random operands and on sums built to land on an fp32 midpoint
    with a non-zero remainder - where a plain fp64 sum rounded to fp32 breaks the tie the wrong way."""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = (rng.standard_normal(4000) * 50).astype(np.float32)
    c = (rng.standard_normal(4000) * 50).astype(np.float32)
    a[4:8] = np.float32(1 + 2.0 ** -12)                                  # a b = 1 + 2^-11 + 2^-24 exactly ...
    b[4:8] = np.float32(1 + 2.0 ** -12)
    c[4:8] = np.array([2.0 ** -60, -2.0 ** -60, 2.0 ** 20, 0.0], np.float32)     # ... a midpoint, nudged either way by c
    got = ref.fmaf(a, b, c)

    def round_f32(q):
        f = np.float32(float(q))                                         # float(q) is correctly rounded to fp64; then refine
        cands = [np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))]
        err = [abs(Fraction(float(x)) - q) for x in cands]
        best = min(err)
        win = [x for x, e in zip(cands, err) if e == best]
        if len(win) == 2:                                                # a true tie: the even mantissa
            win = [x for x in win if (int(np.float32(x).view(np.int32)) & 1) == 0]
        return win[0]

    exp = np.array([round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(np.int32), exp.view(np.int32))
    plain = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert (plain[4:6] != exp[4:6]).any(), "the midpoint operands do not separate a double rounding from the exact result"


def test_transform_against_the_host():
    """The eval table over -64..320 on both paths: equal to torch's `transform_coords` except within one ulp of a tie."""
    from pasco_amd.data.semantic_kitti import transform_coords
    rng = np.random.default_rng(3)
    Ts = cases.transforms("table", 8)
    ints = rng.integers(-64, 321, (200_000, 3)).astype(np.int64)
    ties = total = 0
    for int_path, coords in ((True, ints), (False, ints.astype(np.float64))):
        to, _, near = ref.ref_transform(coords, Ts, int_path)
        for m, T in enumerate(Ts):
            host = transform_coords(torch.from_numpy(coords), torch.from_numpy(T)).long().numpy()
            assert not ((host != to[m]) & ~near[m]).any(), (int_path, m)
        ties += int(near.sum())
        total += near.size
    print(f"[transform] tie share {ties / total:.2e} ({ties} of {total})")
    assert ties <= TIE_SHARE_MAX * total
    for kind in ("identity", "quarter", "shift40", "quarter_shift"):
        for int_path, coords in ((True, ints[:5000]), (False, ints[:5000].astype(np.float64))):
            Tk = cases.transforms(kind)
            to, _, near = ref.ref_transform(coords, Tk, int_path)
            assert not near.any()
            for m, T in enumerate(Tk):
                assert np.array_equal(transform_coords(torch.from_numpy(coords), torch.from_numpy(T)).long().numpy(), to[m]), kind


def test_label_bounds_against_transformed_labels():
    """Every bounds case the reference marks tie-free against `transformed_labels(..., complete_scale=1)`, whose min_C /
    max_C are the raw words 6..11, and words 0..5 against the host's `transform_coords` over the known sites.  At most a
    quarter of the cases may be skipped for ties."""
    from pasco_amd.data.semantic_kitti import transform_coords, transformed_labels
    skipped, run = [], 0
    for kw in cases.BOUNDS_CASES:
        sem, ins, Ts, Tinvs = cases.bounds_inputs(kw["grid"], kw["kind"], kw["M"], kw.get("pattern", "random"))
        exp, tie = ref.ref_label_bounds(sem, ins, Ts, Tinvs)
        if tie:
            skipped.append(kw)
            continue
        run += 1
        if not (sem != 255).any():
            assert (exp[:, [0, 1, 2, 6, 7, 8]] == ref.INT32_MAX).all() and (exp[:, [3, 4, 5, 9, 10, 11]] == ref.INT32_MIN).all()
            continue                                                    # the host path has nothing to resample
        known = torch.nonzero(torch.from_numpy(sem) != 255)
        for m, T in enumerate(Ts):
            T = torch.from_numpy(T)
            *_, min_c, max_c = transformed_labels(sem, ins, T, complete_scale=1)
            assert exp[m, 6:9].tolist() == min_c.tolist() and exp[m, 9:12].tolist() == max_c.tolist(), (kw, m, exp[m], min_c, max_c)
            to = transform_coords(known, T)
            assert exp[m, 0:3].tolist() == to.min(0)[0].tolist() and exp[m, 3:6].tolist() == to.max(0)[0].tolist(), (kw, m)
    print(f"[label bounds] {len(skipped)} of {len(cases.BOUNDS_CASES)} cases skipped for ties: "
          + ", ".join(f"{k['grid']} {k['kind']} M={k['M']}" for k in skipped))
    assert any(k["kind"] == "half" for k in skipped), "the half-voxel case is expected to sit on ties"
    assert 4 * len(skipped) <= len(cases.BOUNDS_CASES)
