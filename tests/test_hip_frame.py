"""Frame preparation on the MI355X (include/pasco_frame.h, csrc/frame.hip) against the host restatements
(data/semantic_kitti.py `build_item`, data/kitti360.py `build_item_kitti360`): bit for bit."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
GOLD = os.path.join(HERE, "golden")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def cuda_only():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def same_batch(a, b, what=""):
    """Every field of two collated batches equal (device tensors compared on the host)."""
    for key in ("in_feats", "in_coords", "min_Cs", "max_Cs"):
        assert len(a[key]) == len(b[key])
        for i, (x, y) in enumerate(zip(a[key], b[key])):
            x, y = torch.as_tensor(x).cpu(), torch.as_tensor(y).cpu()
            assert x.dtype == y.dtype and x.shape == y.shape, (what, key, i, x.dtype, y.dtype, x.shape, y.shape)
            assert torch.equal(x, y), (what, key, i)
    for key in ("global_min_Cs", "global_max_Cs"):
        assert torch.equal(torch.as_tensor(a[key]).cpu(), torch.as_tensor(b[key]).cpu()), (what, key)
    for x, y in zip(a["xyz"], b["xyz"]):
        assert np.array_equal(torch.as_tensor(x).cpu().numpy(), torch.as_tensor(y).cpu().numpy()), (what, "xyz")
    for x, y in zip(a["input_pcd_instance_label"], b["input_pcd_instance_label"]):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(torch.as_tensor(x).cpu().reshape(-1), torch.as_tensor(y).cpu().reshape(-1)), (what, "labels")


def edge_cloud(rng, n):
    """n random points over (and past) the extent, plus every bound and voxel boundary and their +-1 fp32 ulp neighbours."""
    xyz = np.stack([rng.uniform(-3, 54, n), rng.uniform(-27, 27, n), rng.uniform(-2.5, 5, n)], 1)
    pts = [np.concatenate([xyz, rng.random((n, 1))], 1).astype(np.float32)]
    for d, bounds in enumerate(((0.0, 51.2, 1.0, 0.2, 12.6), (-25.6, 25.6, -25.4, 0.0, 3.0), (-2.0, 4.4, -1.8, 0.6, 4.0))):
        for b in bounds:
            f = np.float32(b)
            for v in (np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf)), np.float32(np.float64(b))):
                p = np.array([5.0, -3.0, 0.5, 0.25], np.float32)
                p[d] = v
                pts.append(p[None])
    return np.concatenate(pts).astype(np.float32)


def small_labels(rng, grid=(12, 10, 8), with_ins=True):
    sem = rng.integers(0, 20, grid).astype(np.uint8)
    sem[rng.random(grid) < 0.4] = 255
    ins = np.zeros(grid, np.uint8)
    if with_ins:
        ins[rng.random(grid) < 0.1] = rng.integers(1, 9)
        ins[rng.random(grid) < 0.05] = 255
    return sem, ins


def tables(m):
    from pasco_amd.eval.kitti import subnet_transforms
    return subnet_transforms(m)


def test_points_kitti360_layout_bit_equal():
    """8-channel layout (fp64 lower bound, fp32 upper bound, fp64 centre): edges, P not a multiple of the block, P = 0,
    all cropped, and P > 2048 * 256 (several tiles per block)."""
    cuda_only()
    from pasco_amd.data.kitti360 import build_item_kitti360, prepare_kitti360_on_device
    from pasco_amd.data.semantic_kitti import collate
    rng = np.random.default_rng(1)
    sem, ins = small_labels(rng)
    Ts = tables(2)
    far = np.full((300, 4), 80.0, np.float32)
    for name, pc in (("edges", edge_cloud(rng, 1000)), ("empty", np.zeros((0, 4), np.float32)), ("cropped", far),
                     ("large", edge_cloud(rng, 600_001))):
        host = collate([build_item_kitti360(pc, sem, ins, T) for T in Ts])
        dev = prepare_kitti360_on_device(pc, sem, ins, Ts, DEV)
        same_batch(dev, host, name)
        if name == "cropped":
            assert dev["in_feats"][0].shape[0] == 0


def _write_waffle(path, rng, pc, V=19, E=2, dtype=np.float32):
    P = pc.shape[0]
    with open(path, "wb") as f:
        pickle.dump({"embedding": rng.standard_normal((E, 256, P)).astype(dtype), "coords": pc,
                     "vote": rng.random((P, V)).astype(np.float32)}, f)


def test_points_semantic_kitti_layout_bit_equal(tmp_path):
    """283-channel layout (fp32 bounds, fp32 centre; votes + intensity before the radius, the transposed embedding after)."""
    cuda_only()
    from pasco_amd.data.semantic_kitti import (build_item, collate, prepare_semantic_kitti_on_device,
                                               read_waffleiron_features)
    rng = np.random.default_rng(2)
    sem, ins = small_labels(rng)
    Ts = tables(3)
    for name, pc in (("edges", edge_cloud(rng, 777)), ("empty", np.zeros((0, 4), np.float32))):
        path = os.path.join(tmp_path, name + ".pkl")
        _write_waffle(path, rng, pc)
        xyz, vote, inten, emb = read_waffleiron_features(path, embedding_index=1)
        plab = rng.integers(0, 1 << 16, (pc.shape[0], 1)).astype(np.int32)
        host = collate([build_item(xyz, vote, inten, emb, sem, ins, T, 8, plab) for T in Ts])
        dev = prepare_semantic_kitti_on_device(path, sem, ins, Ts, DEV, embedding_index=1, point_labels=plab)
        same_batch(dev, host, name)
        if pc.shape[0]:
            assert dev["in_feats"][0].shape[1] == 283


def _restated(coords, T, int_path):
    """The defined order of pasco_frame.h: metres, then the fmaf chain k = 0..3 (fmaf emulated in long double), then
    ((v - min_bound) - 0.1) / 0.2 in fp32.  -> (int64 [n, 3], the fp32 value before rounding)."""
    f32, ld = np.float32, np.longdouble
    mb = np.array([0, -25.6, -2], np.float32)
    if int_path:
        h = mb + (coords.astype(f32) * f32(0.2) + f32(0.1))
    else:
        h = (mb.astype(np.float64) + (coords * 0.2 + 0.1)).astype(f32)
    h4 = np.concatenate([h, np.ones((h.shape[0], 1), f32)], 1)
    T = np.asarray(T, np.float32)
    out = np.empty_like(h)
    for i in range(3):
        acc = (T[i, 0].astype(ld) * h4[:, 0].astype(ld)).astype(f32)
        for k in (1, 2, 3):
            acc = (T[i, k].astype(ld) * h4[:, k].astype(ld) + acc.astype(ld)).astype(f32)
        out[:, i] = ((acc - mb[i]) - f32(0.1)) / f32(0.2)
    return np.rint(out).astype(np.int32).astype(np.int64), out


def test_transform_coords_both_paths_under_the_table():
    """2 M fuzzed coordinates per path, the 8 transforms of the eval table in one launch: bit-equal to the restatement of
    the defined order; against torch's host `transform_coords` only at points within 1 ulp of a .5 tie."""
    cuda_only()
    from pasco_amd.data.frame_lib import frame_lib
    from pasco_amd.data.semantic_kitti import transform_coords
    rng = np.random.default_rng(3)
    Ts = tables(8)
    n = 2_000_000
    ints = rng.integers(-64, 320, (n, 3)).astype(np.int64)
    ties = 0
    for int_path, coords in ((True, ints), (False, ints.astype(np.float64))):
        got = frame_lib().transform_coords(torch.from_numpy(coords).to(DEV), Ts).cpu().numpy()
        for m, T in enumerate(Ts):
            exp, v = _restated(coords, T.numpy(), int_path)
            assert np.array_equal(got[m], exp), (int_path, m, int((got[m] != exp).any(1).sum()))
            host = transform_coords(torch.from_numpy(coords), T).long().numpy()
            bad = host != got[m]
            near = np.abs(np.abs(v - np.floor(v)) - np.float32(0.5)) <= np.spacing(np.abs(v))
            assert not (bad & ~near).any(), (int_path, m, int((bad & ~near).sum()))
            ties += int(bad.sum())
    print(f"[transform_coords] {ties} coordinates differ from the host at a .5 tie (within 1 ulp)")


def test_label_bounds_match_build_item():
    """Random grids, a grid without instances, a full-size 256 x 256 x 32 grid; two runs identical.  Words 6..11 against the
    host's bounds at the completion scale and as written (scale 1), words 0..5 against the host's box of the known sites."""
    cuda_only()
    from pasco_amd.data.frame_lib import BOUNDS, box_upper_bound, frame_lib
    from pasco_amd.data.semantic_kitti import completion_bounds, transform_coords, transformed_labels
    rng = np.random.default_rng(4)
    cases = [small_labels(rng, (20, 24, 10)), small_labels(rng, (9, 31, 7)), small_labels(rng, (16, 16, 16), with_ins=False)]
    full_sem = np.zeros((256, 256, 32), np.uint8)
    full_sem[:, :, 20:] = 255
    full_sem[rng.random(full_sem.shape) < 0.2] = 255
    full_sem[100:110, 30:40, 3:9] = 1
    full_ins = np.zeros_like(full_sem)
    full_ins[100:110, 30:40, 3:9] = 4
    full_ins[0:256, 250:256, 0:32] = 255
    cases.append((full_sem, full_ins))
    for ci, (sem, ins) in enumerate(cases):
        Ts = tables(3 if ci < 3 else 2)
        sd, idv = torch.from_numpy(sem).to(DEV), torch.from_numpy(ins).to(DEV)
        Tinv = [torch.inverse(T) for T in Ts]
        bb = box_upper_bound(sem.shape, Ts)
        out = frame_lib().label_bounds(sd, idv, Ts, Tinv, bb).cpu()
        again = frame_lib().label_bounds(sd, idv, Ts, Tinv, bb).cpu()
        assert torch.equal(out, again) and out.shape == (len(Ts), BOUNDS)
        for m, T in enumerate(Ts):
            *_, min_c, max_c = transformed_labels(sem, ins, T)
            dmin, dmax = completion_bounds(out[m, 6:9].clone(), out[m, 9:12].clone())
            assert torch.equal(dmin, min_c) and torch.equal(dmax, max_c), (ci, m, dmin, min_c, dmax, max_c)
            assert (out[m, :3] >= bb[m, :3]).all() and (out[m, 3:6] <= bb[m, 3:]).all()
            # the twelve words as written: the raw minimum / maximum (scale 1 floors nothing) and the box itself
            *_, raw_min, raw_max = transformed_labels(sem, ins, T, complete_scale=1)
            assert torch.equal(out[m, 6:9], raw_min.int()) and torch.equal(out[m, 9:12], raw_max.int()), (ci, m, out[m], raw_min, raw_max)
            to = transform_coords(torch.nonzero(torch.from_numpy(sem) != 255), T)
            assert torch.equal(out[m, :3], to.min(0)[0]) and torch.equal(out[m, 3:6], to.max(0)[0]), (ci, m, out[m])


def _k360_reader():
    from pasco_amd.data import Kitti360FrameReader
    mini = os.path.join(GOLD, "kitti360_mini")
    return Kitti360FrameReader(mini, os.path.join(mini, "preprocess"), os.path.join(mini, "sscbench"),
                               os.path.join(mini, "match.txt"))


def test_readers_batch_on_the_device_equals_the_host():
    """Both readers on their mini trees; the device batch twice: identical."""
    cuda_only()
    from pasco_amd.data import FrameReader
    g = np.load(os.path.join(GOLD, "kitti360_items.npz"))
    Ts = [torch.from_numpy(g[f"{t}_T"]) for t in g["tags"]]
    r = _k360_reader()
    seq, fid = r.frames("test")[0]
    host = r.batch(seq, fid, Ts)
    dev = r.batch(seq, fid, Ts, device=DEV)
    same_batch(dev, host, "kitti360")
    same_batch(r.batch(seq, fid, Ts, device=DEV), dev, "kitti360 rerun")
    assert dev["in_feats"][0].is_cuda and dev["in_feats"][0].shape[1] == 8
    mini = os.path.join(GOLD, "kitti_mini")
    io = np.load(os.path.join(GOLD, "io_items.npz"))
    fr = FrameReader(mini, os.path.join(mini, "preprocess"))
    Ts = [torch.from_numpy(io["eye_T"]), torch.from_numpy(io["rigid_T"])]
    same_batch(fr.batch("08", "000005", Ts, device=DEV), fr.batch("08", "000005", Ts), "semantic kitti")


def _tensors(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif hasattr(x, "F") and hasattr(x, "C"):
        out += [x.F, x.C]
    elif isinstance(x, dict):
        for k in sorted(x, key=str):
            _tensors(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _tensors(v, out)
    return out


def test_step_inference_on_device_and_host_prepared_batches_is_bit_equal(hip, tmp_path, capsys):
    """The mini KITTI-360 frame through `step_inference` from both preparations, and the CLI on the mini tree."""
    from test_kitti360_cpu import kitti360_checkpoint
    from pasco_amd.data import net_from_checkpoint
    from pasco_amd.data.kitti360 import THING_IDS
    ck = kitti360_checkpoint(os.path.join(tmp_path, "k360.ckpt"))
    net = net_from_checkpoint(ck, device=DEV, thing_ids=THING_IDS)
    r = _k360_reader()
    seq, fid = r.frames("test")[0]
    sem, _ = r.labels(seq, fid)
    net.ensembler.scene_size = tuple(int(v) for v in sem.shape)
    Ts = tables(net.n_infers)
    res = []
    for device in (None, DEV):
        b = r.batch(seq, fid, Ts, device=device)
        with torch.no_grad():
            outs, sem_probs, _ = net.step_inference([t.to(DEV) for t in b["in_feats"]], [t.to(DEV) for t in b["in_coords"]],
                                                    [t.to(DEV) for t in b["Ts"]], b["global_min_Cs"], b["global_max_Cs"],
                                                    b["min_Cs"], b["max_Cs"])
        res.append([t.detach().cpu() for t in _tensors([outs, sem_probs], [])])
    assert len(res[0]) == len(res[1]) > 0
    for a, b in zip(*res):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    import pasco_amd.eval.kitti360 as E
    mini = os.path.join(GOLD, "kitti360_mini")
    E.main(["--root", mini, "--preprocess-root", os.path.join(mini, "preprocess"), "--label-root",
            os.path.join(mini, "sscbench"), "--match-file", os.path.join(mini, "match.txt"), "--ckpt", ck])
    text = capsys.readouterr().out
    assert "road" in text and "other-object" in text and "bicyclist" not in text
    print(text)
