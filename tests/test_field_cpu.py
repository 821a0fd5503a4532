"""The point <-> voxel operators without a GPU: the host restatement (pasco_amd/grad/host.py field_*) against the independent
references of tests/field_ref64.py, and `TensorField`, the quantisation modes, `slice` and `MinkowskiInterpolation` of
pasco_amd.me through the CPU checker backend.  The same checks run on the pq_* kernels in tests/test_hip_field.py."""
import pytest
import torch

import pasco_amd.grad as G
from tests import field_cases as fc

CPU = torch.device("cpu")


@pytest.fixture()
def ops(oracle_registered):
    return G.field_ops(torch.zeros(1))


@pytest.mark.parametrize("pattern", fc.GROUP_PATTERNS)
def test_group_against_the_stable_sort(pattern, ops):
    for n in fc.GROUP_N:
        fc.check_group(ops, CPU, pattern, n)


@pytest.mark.parametrize("c", (1, 4, 33))
def test_segment_sums_and_averages(c, ops):
    fc.check_seg_sums(ops, CPU, c)


def test_segment_max_with_arg_bit_for_bit(ops):
    fc.check_seg_max(ops, CPU)
    fc.check_seg_max(ops, CPU, c=33)


def test_gather_w(ops):
    for c in (1, 4, 33):
        fc.check_gather_w(ops, CPU, c)


@pytest.mark.parametrize("ts,batch,one", [(1, 0, False), (2, 3, False), (4, 0, False), (3, 0, False), (1, 3, True)])
def test_interpolation_map_against_the_literal_loop(ts, batch, one, ops):
    fc.check_interp_map(ops, CPU, ts, batch, one)


def test_interpolation_forward_and_backward(ops):
    fc.check_interp_fwd(ops, CPU, 5)
    fc.check_interp_bwd(ops, CPU, 5)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_sparse_in_every_mode_against_the_dense_twin(dtype, ops):
    fc.check_sparse_against_dense(CPU, dtype)
    fc.check_sparse_against_dense(CPU, dtype, ts=2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_slice_and_interpolation_modules(dtype, ops):
    fc.check_slice_and_interpolation(CPU, dtype)
    fc.check_interpolation_against_grid_sample(CPU, dtype)


@pytest.mark.parametrize("name", fc.MODULE_NAMES)
def test_module_modes_give_the_same_bits(name, ops):
    fc.check_module_modes(CPU, torch.float64, name)


@pytest.mark.parametrize("name", ["sparse_unweighted_average", "sparse_unweighted_sum", "sparse_max_pool", "sparse_ts2",
                                  "tensor_unweighted_average", "slice", "cat_slice", "interpolation"])
def test_gradients_in_fp64(name, ops):
    fc.check_gradients_against_differences(name)


def test_pending_prologue_is_applied(ops):
    fc.check_prologue(CPU)


def test_existing_behaviour_is_held(ops):
    fc.check_existing_behaviour(CPU)


def test_refusals(ops):
    fc.check_refusals(CPU)
    fc.check_dtype_refusals(G)


def test_no_double_backward(ops):
    feats, runs = fc.module_runs(CPU, torch.float64, c=2, n=40)
    f = feats.clone().requires_grad_(True)
    out = runs["sparse_unweighted_average"](f)
    (g,) = torch.autograd.grad(out, f, torch.ones_like(out).requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g.sum().backward()


def test_small_net_against_the_dense_fp64_twin(ops):
    """The end-to-end net of tests/test_hip_field.py on the CPU checker in fp32: every gradient within 1e-4 of the largest entry
    of the dense fp64 twin's."""
    params, grads, (feats, coords, target) = fc.net_gradients(CPU)
    twin = fc.net_twin_gradients(params, feats, coords, target)
    assert set(twin) == set(grads) and len(grads) == 6
    for k, g in grads.items():
        w = twin[k]
        assert g.shape == w.shape and float((g.double() - w).abs().max()) <= 1e-4 * float(w.abs().max()), k


def test_batched_coordinates_floor_for_integer_dtypes_only():
    """`ME.utils.batched_coordinates`: an integer dtype floors float points as it always did (-0.5 -> -1); a float dtype keeps the
    fractions, so that a `TensorField` is given the points where they are (reference: maskpls/mink.py:461)."""
    import pasco_amd.me as ME
    pts = [torch.tensor([[0.5, -0.5, 2.75], [-1.0, 3.25, 0.0]]), torch.tensor([[1.5, 1.5, -2.25]])]
    want = torch.tensor([[0, 0.5, -0.5, 2.75], [0, -1.0, 3.25, 0.0], [1, 1.5, 1.5, -2.25]])
    got = ME.utils.batched_coordinates(pts)
    assert got.dtype == torch.int32 and got.device.type == "cpu" and torch.equal(got, torch.floor(want).to(torch.int32))
    assert got.tolist() == [[0, 0, -1, 2], [0, -1, 3, 0], [1, 1, 1, -3]]
    for dtype in (torch.int32, torch.int64):
        assert torch.equal(ME.utils.batched_coordinates(pts, dtype=dtype), torch.floor(want).to(dtype))
    for dtype in (torch.float32, torch.float64, torch.float):
        got = ME.utils.batched_coordinates(pts, dtype=dtype)
        assert got.dtype == dtype and torch.equal(got, want.to(dtype))
    ints = [torch.tensor([[1, -2, 3]]), torch.tensor([[4, 5, -6]])]
    assert ME.utils.batched_coordinates(ints).tolist() == [[0, 1, -2, 3], [1, 4, 5, -6]]
    assert ME.utils.batched_coordinates(ints, dtype=torch.float32).tolist() == [[0.0, 1.0, -2.0, 3.0], [1.0, 4.0, 5.0, -6.0]]


def test_voxel_floor_at_a_stride_that_is_no_power_of_two(ops):
    fc.check_floor_below_boundaries(CPU)
    fc.check_interp_map(ops, CPU, 3, 0)
