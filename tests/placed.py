"""`Placed`: a numpy array together with where it sits inside a larger allocation of the test's own.  numpy only, no case
table and no assertion at import: tests/waffle_edge_cases.py builds such arguments, tests/waffle_device.py uploads the whole
allocation and hands the kernel the view.  That is how a pointer 4 bytes past a 16-byte boundary, a row stride above 3 and
an index just outside an array are reached without leaving memory the test owns."""
import numpy as np


class Placed:
    """`a` is a read-only view of `shape` / `strides` (in elements) at element `offset` of the flat allocation `base`."""

    def __init__(self, base, offset, shape, strides):
        self.base, self.offset, self.shape, self.strides = base, int(offset), tuple(shape), tuple(int(s) for s in strides)

    @property
    def a(self):
        item = self.base.itemsize
        return np.lib.stride_tricks.as_strided(self.base[self.offset:], self.shape, tuple(s * item for s in self.strides),
                                               writeable=False)


def plain(x):
    return x.a if isinstance(x, Placed) else x


def _dense_strides(shape):
    out, step = [], 1
    for s in reversed(shape):
        out.append(step)
        step *= int(s)
    return tuple(reversed(out))


def mid(a, before, after, fill):
    """`a`, contiguous, with `before` / `after` entries of `fill` around it in one allocation."""
    a = np.ascontiguousarray(a)
    base = np.full(before + a.size + after, fill, a.dtype)
    base[before:before + a.size] = a.reshape(-1)
    return Placed(base, before, a.shape, _dense_strides(a.shape))


def off16(a, fill=77):
    """`a` at an address 4 bytes past a 16-byte boundary (the allocation itself starts on one; the GPU leg asserts it)."""
    assert a.dtype.itemsize == 4
    return mid(a, 1, 3, fill)


def columns(a, ld, c0, seed=5):
    """fp32 [n, w] as the columns c0 .. c0 + w - 1 of a row-major [n, ld] matrix whose other entries are noise."""
    n, w = a.shape
    base = np.random.default_rng(seed).uniform(-3.0, 3.0, n * ld).astype(np.float32)
    base.reshape(n, ld)[:, c0:c0 + w] = a
    return Placed(base, c0, (n, w), (ld, 1))
