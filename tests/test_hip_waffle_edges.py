"""The point-feature kernels on the MI355X (include/pasco_waffle.h, csrc/waffle.hip) on the edge cases of
tests/waffle_edge_cases.py, held to the literal references of tests/waffle_ref.py (which tests/test_waffle_edges_cpu.py ties
to the restatement without a GPU) and, for the float kernels, to the restatement in every bit.  `waffle_device.DeviceOps`
puts guard entries behind every output and checks that every input allocation comes back unwritten.  The status paths keep
the safety rule stated at the top of the case module: no bad index leaves the test's own allocations."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import waffle_edge_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
HOST = EC.HostOps()


@pytest.fixture(scope="module")
def ops(hip):
    from pasco_amd.waffle.lib import waffle_lib
    from waffle_device import DeviceOps
    return DeviceOps(waffle_lib())


@pytest.mark.parametrize("name", [r[0] for r in EC.SEARCH_TABLE])
def test_search(ops, name):
    EC.check_search(ops, name)


def test_voxel_keys_at_the_key_bound(ops):
    EC.check_voxel_keys(ops)


def test_cell_index_around_minus_one_and_the_far_edge(ops):
    EC.check_cell_index(ops)


def test_cells_build_refuses_a_bad_order_or_cell(ops):
    EC.check_cells_build(ops)


def test_float_kernels_at_both_vector_widths(ops):
    EC.check_float_kernels(ops, restatement=HOST)
    print("worst errors against float64:", {k: f"{v:.3e}" for k, v in EC.WORST.items()})


def test_neigh_rows_and_group_max_at_their_limits(ops):
    EC.check_neigh_rows(ops, restatement=HOST)
    print("worst errors against float64:", {k: f"{v:.3e}" for k, v in EC.WORST.items()})


def test_status_flatten(ops):
    EC.check_status_flatten(ops)


def test_status_inflate(ops):
    EC.check_status_inflate(ops)


def test_status_neigh_rows(ops):
    EC.check_status_neigh_rows(ops)


def test_status_search_on_a_damaged_csr(ops):
    EC.check_status_search(ops)
