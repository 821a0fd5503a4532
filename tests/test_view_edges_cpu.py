"""The numpy restatement of the view kernels (pasco_amd/viz/host.py) on the edge cases of tests/view_edge_cases.py: shapes
that k does not divide, counts past a byte, the label boundary, negative and tied filter values, partial compose blocks and
repeated ids, rays whose plane crossings tie, origins on a face, -0.0 and the brick step cap.  No GPU;
tests/test_hip_view_edges.py runs the same builders on the kernels.  Importing the case module runs its launch-class
assertions."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import view_edge_cases as EC  # noqa: E402
from pasco_amd.viz import host  # noqa: E402

OPS = EC.HostOps()


def test_case_module_restates_the_header_s_constants():
    import re
    header = open(os.path.join(os.path.dirname(HERE), "include", "pasco_view.h")).read()
    for name, value in (("STATUS_LABEL_RANGE", EC.STATUS_LABEL_RANGE), ("STATUS_STEP_CAP", EC.STATUS_STEP_CAP),
                        ("INSTANCE_BASE", EC.INSTANCE_BASE), ("RAMP_BASE", EC.RAMP_BASE), ("STUFF_FIRST", EC.STUFF_FIRST),
                        ("STUFF_LAST", EC.STUFF_LAST), ("MAX_SEGMENTS", EC.MAX_SEGMENTS), ("BRICK", EC.BRICK)):
        assert int(re.search(rf"#define PV_{name} (\d+)", header).group(1)) == value, name


def test_launch_classes_of_the_cases():
    """The import-time assertions ran; the geometry helper itself, on numbers worked out by hand from csrc/view.hip."""
    assert EC.launch(256) == (1, 0) and EC.launch(259) == (2, 3)
    assert EC.tiles(16, 32) == (1, 2, 0, 0) and EC.tiles(17, 9) == (2, 1, 1, 9)
    assert EC.brick_words((256, 256, 32)) == (4096, 128, 0) and EC.brick_words((9, 8, 8)) == (2, 1, 2)


def test_pool():
    EC.check_pool(OPS)


def test_filter():
    EC.check_filter(OPS)


@pytest.mark.parametrize("n_seg", EC.SEGMENTS)
@pytest.mark.parametrize("shape", EC.COMPOSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compose(shape, n_seg):
    EC.check_compose(OPS, shape, n_seg)


def test_compose_reference_against_the_painting_of_test_view_cpu():
    """The loop reference on the inputs whose expected values tests/test_view_cpu.py paints by hand."""
    shape = (6, 5, 4)
    rng = np.random.default_rng(0)
    pan = rng.integers(0, 6, shape).astype(np.int32)
    seg = np.array([[2, 1, 9, 4, 3], [1, 0, 1, 1, 1], [1, 9, 2, 3, 3],
                    np.float32([0.25, 0.5, 0.75, 1.0, 0.625]).view(np.int32)], np.int32)
    exp = np.zeros(shape, np.uint32)
    for rank, i in ((1, 2), (3, 4), (4, 3)):
        exp[pan == i] = 32 + rank - 1
    assert np.array_equal(EC.compose_reference("mask", shape, 0.0, 1.0, panoptic=pan, seg=seg), exp)


def test_bricks():
    EC.check_bricks(OPS)


def test_render_ties_faces_and_signed_zeros():
    EC.check_render(OPS)


def test_render_coarse_step_cap():
    EC.check_coarse_cap(OPS)


def test_strict_comparison_is_what_the_hand_cases_pin():
    """The rule "ties x, then y, then z" as `<` on the restatement: with `<=` the second hand case would end in (4, 5, 3)."""
    name, colour, cam, site, face = EC.hand_cases()[1]
    hit, f, _, _ = OPS.render(colour, cam, 1, 1, np.zeros((16, 3), np.uint8))
    assert hit[0, 0] == site == EC.site_of(5, 4, 3) and hit[0, 0] != EC.site_of(4, 5, 3) and f[0, 0] == face
    assert host.FACE_INSIDE == 6
