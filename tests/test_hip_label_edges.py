"""The label kernels (include/pasco_label.h, csrc/label.hip) where tests/test_hip_instances.py does not reach: friendly
shapes on unfriendly pointers (every alignment fallback of k_local, k_write and k_semantic), 32 thing classes surviving
inside one wave, thing id 254, a `sizes` array shorter than the instance count or absent, a workspace full of 0xFF, and
a record that already holds numbers.  The reference is the host restatement (`instance_labels_host`,
`semantic_grid_from_raw`), itself pinned to the reference generator's fixture in tests/test_instances_cpu.py."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "semantic-kitti.yaml")
PAD = 16                                  # elements around every placed array; they keep their fill


def placed(n, dtype, offset, fill):
    """A view of n elements `offset` ELEMENTS into a larger buffer of `fill` whose base is 256-byte aligned."""
    buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=DEV)
    assert buf.data_ptr() % 256 == 0 and offset <= PAD
    return buf, buf[offset:offset + n]


def untouched(buf, view_off, n, fill):
    rest = torch.cat([buf[:view_off], buf[view_off + n:]]).cpu()
    return bool((rest == fill).all())


def noise(shape, seed, p=0.5, classes=4):
    rng = np.random.default_rng(seed)
    g = (rng.integers(0, classes, shape) * (rng.random(shape) < p)).astype(np.uint8)
    g[rng.random(shape) < 0.02] = 255
    return g


def run(grid, things, min_size, sem_off=0, ins_off=0, out_off=0, sizes_cap=None, with_sizes=True):
    """pl_instances with every array placed at an offset (sem and semantic_out in bytes, instance in int32 words) against
    the host; the workspace is 64 bytes larger than needed and full of 0xFF, the record starts as 7s."""
    from pasco_amd.data.instances import instance_labels_host
    from pasco_amd.data.label_lib import label_lib
    lib = label_lib()
    e_ins, e_sem, info = instance_labels_host(grid, things, min_size)
    n, S = info["n_instances"], grid.size
    cap = n + 3 if sizes_cap is None else sizes_cap
    sem_buf, sem = placed(S, torch.uint8, sem_off, 0x33)
    sem.copy_(torch.from_numpy(grid.ravel()).to(DEV))
    ins_buf, ins = placed(S, torch.int32, ins_off, -5)
    out_buf, out = placed(S, torch.uint8, out_off, 0x77)
    assert sem.data_ptr() % 256 == sem_off and ins.data_ptr() % 256 == 4 * ins_off and out.data_ptr() % 256 == out_off
    rec = torch.full((4,), 7, dtype=torch.int32, device=DEV)
    sizes = torch.full((cap + 3,), -9, dtype=torch.int32, device=DEV)
    ws = torch.full((lib.workspace_bytes(grid.shape, len(things)) + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    lib.instances_into(sem.view(grid.shape), things, min_size, ins.view(grid.shape), out.view(grid.shape), rec,
                       sizes if with_sizes else None, cap, ws)
    torch.cuda.synchronize(DEV)
    what = (grid.shape, sem_off, ins_off, out_off, cap)
    assert rec.tolist() == [n, info["n_dropped"], info["n_unknown"], 0], (what, rec.tolist(), info)
    assert torch.equal(sem.cpu(), torch.from_numpy(grid.ravel())) and untouched(sem_buf, sem_off, S, 0x33), what
    assert torch.equal(ins.cpu().view(grid.shape), torch.from_numpy(e_ins)) and untouched(ins_buf, ins_off, S, -5), what
    assert torch.equal(out.cpu().view(grid.shape), torch.from_numpy(e_sem)) and untouched(out_buf, out_off, S, 0x77), what
    k = min(n, cap)
    if with_sizes:
        assert torch.equal(sizes[:k].cpu(), torch.from_numpy(info["sizes"][:k])), what
        assert bool((sizes[k:] == -9).all()), (what, "sizes written past min(n, sizes_cap)")
    else:
        assert bool((sizes == -9).all())
    return info


@pytest.mark.parametrize("shape", [(16, 16, 32), (8, 8, 64)])
@pytest.mark.parametrize("sem_off", [1, 4, 8])
def test_sem_on_an_unaligned_pointer(hip, shape, sem_off):
    """Z % 8 == 0 and S % 4 == 0, `sem` 1, 4 and 8 bytes into a buffer: the narrow loads of k_local (1, 4) and k_write (1)."""
    info = run(noise(shape, sem_off), [1, 2, 3], 3, sem_off=sem_off)
    assert info["n_instances"] > 3 and info["n_dropped"] > 3


@pytest.mark.parametrize("shape", [(16, 16, 32), (8, 8, 64)])
@pytest.mark.parametrize("ins_off,out_off", [(1, 0), (0, 1), (1, 1), (0, 4)])
def test_outputs_on_unaligned_pointers(hip, shape, ins_off, out_off):
    """`instance` 4 bytes and `semantic_out` 1 byte into a buffer: k_write<1> on a shape k_write<4> would take."""
    run(noise(shape, 10 + ins_off + 2 * out_off), [2, 1, 3], 3, ins_off=ins_off, out_off=out_off)


def wave_of_classes():
    """16 x 8 x 8: ids 1..31 and 254, one 2-voxel blob each, all inside the first 64 sites (one wave of k_rank); the ids in a
    seeded order, so the instance numbering (class position first) is no raster order."""
    ids = list(range(1, 32)) + [254]
    g = np.zeros((16, 8, 8), np.uint8)
    flat = g.reshape(-1)
    order = np.random.default_rng(4).permutation(32)
    for k, j in enumerate(order):
        flat[2 * k] = flat[2 * k + 1] = ids[j]
    assert (flat[:64] != 0).all() and not flat[64:].any()
    return g, ids


def test_32_classes_survive_inside_one_wave(hip):
    g, ids = wave_of_classes()
    info = run(g, ids, 2)
    assert info["n_instances"] == 32 and info["sizes"].tolist() == [2] * 32 and info["n_dropped"] == 0
    info = run(g, ids, 3)
    assert info["n_instances"] == 0 and info["n_dropped"] == 32 and info["n_unknown"] == 64
    from pasco_amd.data.instances import instance_labels_host
    assert (instance_labels_host(g, ids, 3)[1].reshape(-1)[:64] == 255).all()
    run(g, ids[::-1], 2, sem_off=1)


def test_sizes_shorter_than_the_instances_or_absent(hip):
    g = noise((16, 16, 32), 21)
    n = run(g, [1, 2, 3], 3)["n_instances"]
    assert n > 4
    for cap in (0, 1, n - 1, n):
        run(g, [1, 2, 3], 3, sizes_cap=cap)
    run(g, [1, 2, 3], 3, sizes_cap=n + 2, with_sizes=False)
    run(g, [1, 2, 3], 3, sizes_cap=0, with_sizes=False)


def test_existing_wrapper_is_unchanged(hip):
    """`instances` / `semantic_grid` allocate as before and agree with the placed calls."""
    from pasco_amd.data.instances import instance_labels_host
    from pasco_amd.data.label_lib import label_lib
    g = noise((16, 16, 32), 30)
    e_ins, e_sem, info = instance_labels_host(g, [1, 2, 3], 3)
    ins, out, rec, sizes = label_lib().instances(torch.from_numpy(g).to(DEV), [1, 2, 3], 3, sizes_cap=int(info["n_instances"]))
    assert torch.equal(ins.cpu(), torch.from_numpy(e_ins)) and torch.equal(out.cpu(), torch.from_numpy(e_sem))
    assert rec.tolist() == [info["n_instances"], info["n_dropped"], info["n_unknown"], 0]
    assert torch.equal(sizes.cpu(), torch.from_numpy(info["sizes"]))
    assert label_lib().instances(torch.from_numpy(g).to(DEV), [1], 3)[3] is None


@pytest.mark.parametrize("S", [64, 2048 + 8, 16 * 16 * 32])
def test_semantic_grid_with_sem_unaligned(hip, S):
    """An aligned `raw` with `sem` one byte into a buffer (k_semantic<false> because of `sem`), and both aligned."""
    from pasco_amd.data import instances as I
    from pasco_amd.data.label_lib import label_lib
    lut = I.remap_lut(CONFIG)
    rng = np.random.default_rng(S)
    raw = rng.integers(0, lut.size, S).astype(np.uint16)
    inv = np.packbits((rng.random(S) < 0.3).astype(np.uint8))
    exp = torch.from_numpy(I.semantic_grid_from_raw(raw, inv, lut, (S // 8, 4, 2)).ravel())
    d_raw, d_inv, d_lut = (torch.from_numpy(a).to(DEV) for a in (raw, inv, lut))
    assert d_raw.data_ptr() % 16 == 0
    for off in (1, 0, 4, 8):
        buf, sem = placed(S, torch.uint8, off, 0x77)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        label_lib().semantic_grid_into(d_raw, d_inv, d_lut, sem, status)
        assert int(status.item()) == 0 and torch.equal(sem.cpu(), exp) and untouched(buf, off, S, 0x77), off
