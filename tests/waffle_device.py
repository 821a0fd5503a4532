"""`DeviceOps`: the pw_* entry points behind the methods of `waffle_cases.HostOps`, shared by tests/test_hip_waffle.py and
tests/test_hip_waffle_edges.py.  numpy in, numpy out; every output buffer has GUARD entries behind it (and, inside
`output_off16`, one in front) that must come back untouched, and every input allocation must come back as it went up.  An
input may be a `placed.Placed` array: its whole allocation goes up and the kernel is handed the view."""
import contextlib

import numpy as np
import torch

from placed import Placed

DEV = torch.device("cuda", 0)
GUARD = 64


class _Up:
    """One uploaded input: `.t` is what the entry point is handed."""

    def __init__(self, a):
        self.host = a.base if isinstance(a, Placed) else np.ascontiguousarray(a)
        self.whole = torch.from_numpy(self.host).to(DEV)
        if isinstance(a, Placed):
            self.t = torch.as_strided(self.whole, a.shape, a.strides, a.offset)
            assert self.whole.data_ptr() % 16 == 0 and self.t.data_ptr() == self.whole.data_ptr() + a.offset * self.host.itemsize
        else:
            self.t = self.whole

    def unchanged(self):
        back = self.whole.cpu().numpy()
        return np.array_equal(back.view(np.uint8).reshape(-1), self.host.view(np.uint8).reshape(-1))


def dev(a):
    return _Up(a).t


class DeviceOps:
    name = "device"

    def __init__(self, lib):
        self.lib = lib
        self.shift = 0                   # entries in front of an output: 1 puts it 4 bytes past a 16-byte boundary

    @contextlib.contextmanager
    def output_off16(self):
        self.shift = 1
        try:
            yield
        finally:
            self.shift = 0

    def _run(self, numel, dtype, fill, inputs, call, status=True):
        shift = self.shift
        whole = torch.full((shift + numel + GUARD,), fill, dtype=dtype, device=DEV)
        out = whole[shift:]
        assert whole.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 * shift
        st = torch.zeros(1 + GUARD, dtype=torch.int32, device=DEV)
        ups = [_Up(a) for a in inputs]
        call(out, st[:1], *[u.t for u in ups])
        torch.cuda.synchronize(DEV)
        assert bool((out[numel:] == fill).all()), "written past the end of the output"
        assert bool((whole[:shift] == fill).all()), "written in front of the output"
        assert not st[1:].any(), "written past the status word"
        for u in ups:
            assert u.unchanged(), "an input was written"
        res = out[:numel].cpu().numpy()
        return (res, int(st[0].item())) if status else res

    def voxel_keys(self, pc, mn, voxel):
        n = pc.shape[0]
        key, st = self._run(3 * n, torch.int32, -7, [pc, mn], lambda o, s, a, b: self.lib.voxel_keys(a, b, voxel, s, out=o))
        return key.reshape(n, 3), st

    def cell_index(self, pc, dims, lo, res, shape):
        return self._run(pc.shape[0], torch.int32, -7, [pc], lambda o, s, a: self.lib.cell_index(a, dims, lo, res, shape, s, out=o))

    def grid_cells(self, xyz, g):
        return self._run(xyz.shape[0], torch.int32, -7, [xyz], lambda o, s, a: self.lib.grid_cells(a, g, s, out=o))

    def cells_build(self, cell, ncell, order=None):
        d_cell = dev(cell)
        d_order = torch.sort(d_cell, stable=True)[1].to(torch.int32) if order is None else dev(order)
        start, st = self._run(ncell + 1, torch.int32, -7, [cell], lambda o, s, a: self.lib.cells_build(a, ncell, s, start=o, order=d_order))
        return start, d_order.cpu().numpy(), st

    def knn(self, xyz, start, order, g, k):
        n = xyz.shape[0]
        return self._run(n * k, torch.int32, -7, [xyz, start, order], lambda o, s, a, b, c: self.lib.knn(a, b, c, g, k, out=o),
                         status=False).reshape(n, k)

    def nearest(self, xyz, start, order, g, q):
        return self._run(q.shape[0], torch.int32, -7, [xyz, start, order, q],
                         lambda o, s, a, b, c, d: self.lib.nearest(a, b, c, g, d, out=o), status=False)

    def flatten(self, tokens, scale, shift, start, order, ncell):
        C = tokens.shape[1]
        grid, st = self._run(ncell * C, torch.float32, -3.0, [tokens, scale, shift, start, order],
                             lambda o, s, a, b, c, d, e: self.lib.flatten(a, b, c, d, e, ncell, s, out=o))
        return grid.reshape(ncell, C), st

    def inflate(self, tokens, scale, grid, cell):
        numel = int(np.prod(tokens.shape))
        out, st = self._run(numel, torch.float32, -3.0, [tokens, scale, grid, cell],
                            lambda o, s, a, b, c, d: self.lib.inflate(a, b, c, d, s, out=o))
        d_tok = dev(tokens)                                      # in place is allowed
        self.lib.inflate(d_tok, dev(scale), dev(grid), dev(cell), torch.zeros(1, dtype=torch.int32, device=DEV), out=d_tok)
        assert np.array_equal(d_tok.cpu().numpy().reshape(-1), out)
        return out.reshape(tokens.shape), st

    def dwconv3x3(self, g, H, W, w, b, relu):
        return self._run(int(np.prod(g.shape)), torch.float32, -3.0, [g, w, b],
                         lambda o, s, a, ww, bb: self.lib.dwconv3x3(a, H, W, ww, bb, relu, out=o), status=False).reshape(g.shape)

    def neigh_rows_status(self, feat, knn, p0, np_, A, b):
        k, C = knn.shape[1], A.shape[1]
        rows, st = self._run(np_ * k * C, torch.float32, -3.0, [feat, knn, A, b],
                             lambda o, s, f, kk, a, bb: self.lib.neigh_rows(f, kk, p0, np_, a, bb, s, out=o))
        return rows.reshape(np_ * k, C), st

    def neigh_rows(self, feat, knn, p0, np_, A, b):
        rows, st = self.neigh_rows_status(feat, knn, p0, np_, A, b)
        assert st == 0
        return rows

    def group_max(self, rows, np_, k, ld_out):
        C = rows.shape[1]
        wide = self._run(np_ * ld_out, torch.float32, -3.0, [rows],
                         lambda o, s, r: self.lib.group_max(r, np_, k, o[:np_ * ld_out].view(np_, ld_out)[:, ld_out - C:]),
                         status=False).reshape(np_, ld_out)
        assert (wide[:, :ld_out - C] == -3.0).all(), "written outside the column slice"
        return wide[:, ld_out - C:]
