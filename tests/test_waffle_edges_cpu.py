"""The restatement of the point-feature kernels (pasco_amd/waffle/host.py) on the edge cases of tests/waffle_edge_cases.py,
held to the literal references of tests/waffle_ref.py: k at both ends and at n - 1, coincident points, degenerate grids, row
strides, the key and cell bounds, damaged CSRs and every status path.  No GPU; tests/test_hip_waffle_edges.py runs the same
builders on the kernels.  Importing the case module runs its launch-class assertions."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import waffle_edge_cases as EC  # noqa: E402
import waffle_ref as R  # noqa: E402
from pasco_amd.waffle import host  # noqa: E402

OPS = EC.HostOps()


def test_reference_restates_the_header_s_constants():
    import re
    header = open(os.path.join(os.path.dirname(HERE), "include", "pasco_waffle.h")).read()
    for name, value in (("MAX_K", R.MAX_K), ("MAX_FEAT", R.MAX_FEAT), ("STATUS_OFF_GRID", R.STATUS_OFF_GRID),
                        ("STATUS_ORDER", R.STATUS_ORDER), ("STATUS_INDEX", R.STATUS_INDEX), ("STATUS_KEY_RANGE", R.STATUS_KEY_RANGE)):
        assert int(re.search(rf"#define PW_{name} (\d+)", header).group(1)) == value, name
    assert "pasco_amd" not in open(os.path.join(HERE, "waffle_ref.py")).read().split('"""', 2)[2]     # shares no code with host.py


def test_launch_classes_of_the_tables():
    """The import-time assertions ran; the geometry helper itself, on numbers worked out by hand from csrc/waffle.hip."""
    assert EC.launch(256) == (1, 0) and EC.launch(257) == (2, 1) and EC.launch(129, EC.SEARCH_BLOCK) == (2, 1)
    assert EC.width(8) == 4 and EC.width(8, aligned=False) == 1 and EC.width(6) == 1
    assert EC.cells_build_threads(40, 100) == 101 and EC.cells_build_threads(300, 7) == 300


def test_the_all_pairs_reference_against_the_restatement_s_own():
    xyz = EC.search_case("coincident groups")["xyz"]
    for k in (1, 16, 32):
        assert np.array_equal(R.all_pairs(xyz, xyz, k, True), host.knn_brute(xyz, xyz, k, True))


@pytest.mark.parametrize("name", [r[0] for r in EC.SEARCH_TABLE])
def test_search(name):
    EC.check_search(OPS, name)


def test_voxel_keys_at_the_key_bound():
    EC.check_voxel_keys(OPS)


def test_cell_index_around_minus_one_and_the_far_edge():
    EC.check_cell_index(OPS)
    probes = EC.cell_probes()
    assert sum(a for _, _, a in probes) == 8 and len(probes) == 16


def test_cells_build_refuses_a_bad_order_or_cell():
    EC.check_cells_build(OPS)


def test_float_kernels_at_both_vector_widths():
    EC.check_float_kernels(OPS)


def test_neigh_rows_and_group_max_at_their_limits():
    EC.check_neigh_rows(OPS)


def test_status_flatten():
    EC.check_status_flatten(OPS)


def test_status_inflate():
    EC.check_status_inflate(OPS)


def test_status_neigh_rows():
    EC.check_status_neigh_rows(OPS)


def test_status_search_on_a_damaged_csr():
    EC.check_status_search(OPS)
