"""The view kernels on the MI355X (include/pasco_view.h, csrc/view.hip) on the edge cases of tests/view_edge_cases.py, held
to the same references as tests/test_view_edges_cpu.py holds the restatement to, and to the restatement in every bit (by
value where the reference leaves the sign of a zero open).  Guard entries sit behind every output, and every input must come
back unwritten."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import view_edge_cases as EC  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GUARD = 64
HOST = EC.HostOps()


def dev(a):
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same(t, a):
    a = np.ascontiguousarray(a)
    return np.array_equal(t.cpu().numpy().reshape(-1).view(np.uint8), a.reshape(-1).view(np.uint8))


def guarded(numel, dtype, fill):
    return torch.full((numel + GUARD,), fill, dtype=dtype, device=DEV)


def taken(buf, numel, fill, shape, dtype):
    """The first `numel` entries as a numpy array of `shape`; the guard behind them must hold `fill`."""
    torch.cuda.synchronize(DEV)
    assert bool((buf[numel:] == fill).all()), "written past the end of the output"
    return buf[:numel].cpu().numpy().view(dtype).reshape(shape)


class DeviceOps:
    """The pv_* entry points behind the methods of `view_edge_cases.HostOps`: numpy in, numpy out."""
    name = "device"

    def __init__(self, lib):
        self.lib = lib

    def pool(self, grid, k):
        shape = tuple(s // k for s in grid.shape)
        numel = int(np.prod(shape))
        d = dev(grid)
        out = guarded(numel, torch.uint8, 77)
        status = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
        self.lib.majority_pool(d, k, out=out, status=status)
        res = taken(out, numel, 77, shape, np.uint8)
        assert same(d, grid) and not status[1:].any()
        return res, int(status[0].item())

    def filter(self, grid, op, mask=None):
        d, dm = dev(grid), None if mask is None else dev(mask)
        out = guarded(grid.size, torch.float32, -3.0)
        self.lib.window_filter(d, op, dm, out=out)
        res = taken(out, grid.size, -3.0, grid.shape, np.float32)
        assert same(d, grid) and (mask is None or same(dm, mask))
        return res

    def compose(self, view, shape, vmin, vmax, **inputs):
        ups = {k: dev(v) for k, v in inputs.items()}
        numel = int(np.prod(shape))
        out = guarded(numel, torch.int32, -5)
        self.lib.compose(view, shape, vmin=vmin, vmax=vmax, out=out, **ups)
        res = taken(out, numel, -5, shape, np.uint32)
        assert all(same(ups[k], v) for k, v in inputs.items())
        return res

    def _bricks(self, d_colour, shape):
        words = self.lib.brick_words(shape)
        assert words == EC.brick_words(shape)[1]
        bits = guarded(words, torch.int32, 0x5A5A5A5A)
        self.lib.bricks(d_colour, out=bits)
        return bits, taken(bits, words, 0x5A5A5A5A, (words,), np.uint32)

    def bricks(self, colour):
        d = dev(colour)
        res = self._bricks(d, colour.shape)[1]
        assert same(d, colour)
        return res

    def render(self, colour, cam, W, H, palette, step_cap=0):
        d, d_cam, d_pal = dev(colour), dev(cam), dev(palette)
        bits, words = self._bricks(d, colour.shape)
        hit, face, rgb = guarded(W * H, torch.int32, -9), guarded(W * H, torch.uint8, 99), guarded(3 * W * H, torch.uint8, 99)
        status = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
        self.lib.render(d, bits, d_cam, W, H, d_pal, EC.FACTORS, EC.BG, step_cap, hit=hit, face=face, rgb=rgb, status=status)
        res = (taken(hit, W * H, -9, (H, W), np.int32), taken(face, W * H, 99, (H, W), np.uint8),
               taken(rgb, 3 * W * H, 99, (H, W, 3), np.uint8), int(status[0].item()))
        assert same(d, colour) and same(d_cam, cam) and same(d_pal, palette) and not status[1:].any()
        assert same(bits[:words.size], words) and bool((bits[words.size:] == 0x5A5A5A5A).all()), "the brick words were written"
        return res


@pytest.fixture(scope="module")
def ops(hip):
    from pasco_amd.viz.lib import view_lib
    return DeviceOps(view_lib())


def test_pool(ops):
    EC.check_pool(ops, restatement=HOST)


def test_pool_with_no_cell_writes_nothing(ops):
    """10 x 7 x 5 at k = 8: one axis is below k.  `DeviceOps.pool` found the whole output buffer at its sentinel."""
    got, status = ops.pool(np.full(EC.POOL_ODD, 40, np.uint8), 8)          # labels that would raise the status if they were read
    assert got.shape == (1, 0, 0) and status == 0


def test_filter(ops):
    EC.check_filter(ops, restatement=HOST)


@pytest.mark.parametrize("n_seg", EC.SEGMENTS)
@pytest.mark.parametrize("shape", EC.COMPOSE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_compose(ops, shape, n_seg):
    EC.check_compose(ops, shape, n_seg, restatement=HOST)


def test_bricks(ops):
    EC.check_bricks(ops, restatement=HOST)


def test_render_ties_faces_and_signed_zeros(ops):
    EC.check_render(ops, restatement=HOST)


def test_render_coarse_step_cap(ops):
    EC.check_coarse_cap(ops, restatement=HOST)
