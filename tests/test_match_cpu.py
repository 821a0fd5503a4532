"""The matcher and mask-loss family on the CPU: the torch restatements of pasco_amd/grad/host.py and the modules of
pasco_amd/grad/criterion.py over them, held to tests/match_ref64.py by the ratio rule with PM_HOST_M; pm_assign (the library's
host entry point, no GPU) and its restatement against brute force; the stand-alone solver check under the address and
undefined-behaviour sanitizers; the criterion against the recorded reference scenes.  The device side is tests/test_hip_match.py."""
import os
import shutil
import subprocess

import pytest
import torch

from tests import match_cases as mc
from tests import match_ref64 as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


@pytest.mark.parametrize("pattern", mc.PATTERNS)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "Q%d_T%d_N%d" % s)
def test_host_sums_losses_and_gradient_against_fp64(shape, pattern):
    mc.check_precision(CPU, mref.PM_HOST_M, "host", shape, pattern)


@pytest.mark.parametrize("pattern", mc.PATTERNS)
@pytest.mark.parametrize("shape", [s for s in mc.SHAPES if s[1] >= 1], ids=lambda s: "Q%d_T%d_N%d" % s)
def test_host_assignment_is_near_optimal_under_the_fp64_cost(shape, pattern):
    mc.check_assignment(CPU, mref.PM_HOST_M, "host", shape, pattern)


def test_host_indices_equal_the_fp64_optimum_on_the_seeded_cases():
    mc.check_indices_equal(CPU, mref.PM_HOST_M, "host")


def test_host_garbage_bits_beyond_t_change_nothing():
    mc.check_garbage_bits(CPU)


@pytest.mark.parametrize("t,with_unknown,n_outside", [(1, True, 0), (3, False, 0), (33, True, 6), (128, True, 3)])
def test_host_target_pack_equals_a_numpy_gather(t, with_unknown, n_outside):
    mc.check_target_pack(CPU, t, with_unknown, n_outside)


def test_geometry_mirrors_the_library():
    from pasco_amd.build import build_hip
    from pasco_amd.grad.matchlib import MatchLib, geometry
    lib = MatchLib(build_hip(verbose=False))
    for n in (0, 1, 127, 128, 129, 256, 257, 20000, 32768, 32769, 60000, 10 ** 6):
        for q, t in ((1, 1), (32, 33), (100, 30), (128, 128)):
            g = geometry(n, q, t)
            assert g["ranges"] == lib.ranges(n, q, t) and g["workspace_bytes"] == lib.workspace_bytes(n, q, t), (n, q, t)
            assert g["ranges"] <= 256 and g["range_rows"] % 32 == 0
    assert lib.workspace_bytes(10, 129, 1) == 0 and lib.workspace_bytes(10, 1, 129) == 0 and lib.workspace_bytes(-1, 1, 1) == 0
    assert geometry(10, 129, 1)["workspace_bytes"] == 0


def test_more_than_128_targets_or_queries_raise_value_error():
    from pasco_amd.grad import criterion as crit
    with pytest.raises(ValueError, match="129 targets"):
        crit.pack_targets(torch.zeros(129, 2, 2, 2, dtype=torch.uint8), None, torch.zeros(1, 4, dtype=torch.int32))
    x = mc.inputs((3, 2, 3), "partition")
    with pytest.raises(ValueError, match="129 queries"):
        crit.HungarianMatcher().match_packed(torch.zeros(3, 129), torch.zeros(129, 21), x.labels, x.class_weights, x.packed(CPU))
    with pytest.raises(ValueError, match="129 queries"):
        crit.mask_losses(torch.zeros(3, 129), x.packed(CPU), torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int64),
                         torch.ones(1))


def test_rows_outside_the_grid_raise_index_error():
    from pasco_amd.grad import criterion as crit
    masks, unknown, coords, _ = mc.pack_case(3, n_outside=2)
    packed = crit.pack_targets(masks, unknown, coords, (3, -2, 10))
    assert int(packed.oob) == 2
    n = coords.shape[0]
    with pytest.raises(IndexError, match="2 voxel rows"):
        crit.HungarianMatcher().match_packed(torch.zeros(n, 4), torch.zeros(4, 21), torch.zeros(3, dtype=torch.int64),
                                             torch.ones(21), packed)


def test_double_backward_is_refused():
    from pasco_amd.grad import criterion as crit
    x = mc.inputs((3, 2, 3), "partition")
    logits = x.logits.clone().requires_grad_(True)
    lm, ld = crit.mask_losses(logits, x.packed(CPU), *x.optimum, x.pair_weights)
    w = torch.ones_like(lm).requires_grad_(True)                 # so that the first backward is itself part of a graph
    (g,) = torch.autograd.grad((lm * w).sum() + (ld * w).sum(), logits, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


# ---- pm_assign -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pasco_amd.build import build_hip
    from pasco_amd.grad.matchlib import MatchLib
    return MatchLib(build_hip(verbose=False))


def test_pm_assign_equals_brute_force_on_every_small_case(lib):
    mc.check_assign_against_brute_force(lib.assign)


def test_host_assign_equals_brute_force_on_every_small_case():
    from pasco_amd.grad import host
    mc.check_assign_against_brute_force(host.assign)


def test_pm_assign_refuses_a_non_finite_cost(lib):
    c = torch.rand(4, 3, dtype=torch.float64)
    c[2, 1] = float("nan")
    with pytest.raises(RuntimeError, match="non-finite"):
        lib.assign(c)
    c[2, 1] = float("inf")
    with pytest.raises(RuntimeError, match="non-finite"):
        lib.assign(c)
    from pasco_amd.grad import host
    with pytest.raises(RuntimeError, match="non-finite"):
        host.assign(c)


def test_pm_assign_total_cost_equals_scipy(lib):
    optimize = pytest.importorskip("scipy.optimize")
    g = torch.Generator().manual_seed(11)
    for q, t in ((1, 1), (100, 30), (30, 100), (128, 128), (128, 1), (77, 128)):
        for scale in (1.0, 5.0):
            c = torch.floor(torch.rand(q, t, generator=g, dtype=torch.float64) * scale * 20) / 20 if scale > 1 else \
                torch.randn(q, t, generator=g, dtype=torch.float64)
            row, col = lib.assign(c)
            r, s = optimize.linear_sum_assignment(c.numpy())
            assert row.tolist() == r.tolist()
            assert abs(float(c[row, col].sum()) - float(c.numpy()[r, s].sum())) <= 1e-9, (q, t, scale)


def test_assign_check_program_under_the_sanitizers(tmp_path):
    """tools/pm_assign_check.cpp (its own main, includes csrc/pm_assign.h) built by the host compiler with the address and
    undefined-behaviour sanitizers: brute force on every Q, T <= 5, exchange optimality at 100 x 30 and 128 x 128."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "pm_assign_check")
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
                    os.path.join(ROOT, "tools", "pm_assign_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pm_assign_check: ok" in r.stdout


# ---- the recorded reference scenes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", mc.GOLDEN_SCENES)
def test_criterion_against_the_recorded_reference(scene, oracle_registered):
    mc.check_golden(CPU, mref.PM_HOST_M, "host", scene)


def test_matcher_forward_takes_the_reference_call(oracle_registered):
    """HungarianMatcher(outputs, targets, class_weights, unknown_mask_dense) with sparse `voxel_logits` and `masks` over the same
    rows, as the reference's criterion calls it: the recorded reference matches of scene a."""
    import pasco_amd.me as ME
    from pasco_amd.grad import criterion as crit
    z = mc.golden("a")
    coords = torch.from_numpy(z["coords"]).clone()
    coords[:, 1:] -= torch.from_numpy(z["min_c"])
    c = coords.long()
    masks = torch.from_numpy(z["masks"])
    logits = ME.SparseTensor(features=torch.from_numpy(z["logits0"]).float(), coordinates=coords)
    tgt_rows = masks[:, c[:, 1], c[:, 2], c[:, 3]].t().float()
    outputs = {"voxel_logits": logits, "query_logits": torch.from_numpy(z["query_logits0"])[0]}
    targets = {"labels": torch.from_numpy(z["labels"]), "masks": ME.SparseTensor(features=tgt_rows, coordinates=coords)}
    matcher = crit.HungarianMatcher(cost_class=1, cost_mask=1, cost_dice=1)
    src, tgt = matcher(outputs, targets, torch.from_numpy(z["class_weights"]), torch.from_numpy(z["unknown"]).bool()[None])
    assert src.dtype == torch.int64 and tgt.dtype == torch.int64
    assert torch.equal(src, torch.from_numpy(z["src0"])) and torch.equal(tgt, torch.from_numpy(z["tgt0"]))
    assert "cost_class: 1" in repr(matcher)
    with pytest.raises(AssertionError):
        crit.HungarianMatcher(0, 0, 0)


def test_criterion_with_two_batch_elements_is_the_mean_of_the_two(oracle_registered):
    """Two target dicts: the rows of each batch index are matched and supervised against their own targets, and every loss is
    the mean over the two elements - scenes a and b of the recorded reference, stacked."""
    import pasco_amd.me as ME
    za, zb = mc.golden("a"), mc.golden("b")
    criterion = mc.build_criterion(za, CPU)
    assert torch.equal(torch.from_numpy(za["class_weights"]), criterion.class_weights[0])
    min_c = torch.from_numpy(za["min_c"])
    assert torch.equal(min_c, torch.from_numpy(zb["min_c"]))

    def scene(z, b):
        c = torch.from_numpy(z["coords"]).clone()
        c[:, 0] = b
        return c, torch.from_numpy(z["logits0"]).float(), torch.from_numpy(z["query_logits0"])[0]

    def run(parts, targets):
        coords = torch.cat([p[0] for p in parts])
        feats = torch.cat([p[1] for p in parts]).requires_grad_(True)
        ql = torch.stack([p[2] for p in parts])
        out = {"voxel_logits": ME.SparseTensor(features=feats, coordinates=coords), "query_logits": ql}
        return criterion(None, out, targets, None, None, 0, [], min_c), feats

    ta = {"labels": torch.from_numpy(za["labels"]), "masks": torch.from_numpy(za["masks"])}
    tb = {"labels": torch.from_numpy(zb["labels"]), "masks": torch.from_numpy(zb["masks"])}
    both, feats = run([scene(za, 0), scene(zb, 1)], [ta, tb])
    assert [tuple(len(s) for s, _ in lv) for lv in criterion.matched] == [(7, 12)]
    one_a, _ = run([scene(za, 0)], [ta])
    one_b, _ = run([scene(zb, 0)], [tb])
    for k in ("loss_ce", "loss_mask", "loss_dice"):
        want = float(((one_a[k] + one_b[k]) / 2).detach())
        assert abs(float(both[k].detach()) - want) <= 1e-6 * abs(want), k
    (both["loss_mask"] + both["loss_dice"]).backward()
    n_a = za["coords"].shape[0]
    assert bool(feats.grad[:n_a].any()) and bool(feats.grad[n_a:].any())


def test_criterion_state_dict_and_ssc_terms():
    mc.check_state_dict_and_ssc(CPU)
