"""ctypes binding of include/pasco_optim.h (the `po_*` entry points of libpascohip.so): the gradient norm over a table of
tensors, the step's scalars and state records, and the AdamW update with the clip folded in.

Kept apart from `me.backend` like `grad.normlib`.  The tables and records are plain device buffers laid out as the header's
structs (the numpy dtypes below); every method takes device tensors and enqueues on the caller's current stream; nothing
synchronises.  The optimiser over it is `grad.optim.AdamW`."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from .._clib import FamilyLib, shared

PO_ABI_VERSION = 1       # include/pasco_optim.h PO_ABI_VERSION this binding was written against
PO_CHUNK = 4096          # elements of one chunk
PO_MAX_GROUPS = 8
PO_POLICY_PROPAGATE, PO_POLICY_SKIP = 0, 1

# the records of the header, field for field
TENSOR_DTYPE = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i8"), ("group", "<i4"), ("state", "<i4")])
CHUNK_DTYPE = np.dtype([("tensor", "<i4"), ("start", "<i4")])
STATE_DTYPE = np.dtype([("step", "<i8"), ("beta1_pow", "<f8"), ("beta2_pow", "<f8")])
RESULT_DTYPE = np.dtype([("sumsq", "<f8"), ("norm", "<f8"), ("skipped", "<i8")])
STEP_DTYPE = np.dtype([("clip", "<f4"), ("apply", "<i4")])
SCALAR_FIELDS = ("decay", "omb1", "b2", "omb2", "bc2sqrt", "eps", "neg_step", "unused")      # po_scalars: eight floats
assert (TENSOR_DTYPE.itemsize, CHUNK_DTYPE.itemsize, STATE_DTYPE.itemsize, RESULT_DTYPE.itemsize, STEP_DTYPE.itemsize) == \
    (48, 8, 24, 24, 8)


class Group(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double)]


class Groups(C.Structure):
    """po_groups: the hyper-parameters of every group, passed by value."""
    _fields_ = [("g", Group * PO_MAX_GROUPS)]


_vp, _i64, _i32, _f64 = C.c_void_p, C.c_int64, C.c_int32, C.c_double
# name -> argtypes (everything returns int unless listed in _RESTYPES)
_SIGNATURES = {
    "abi_version": [],
    "last_error": [],
    "table_check": [_i64, _i64, _i64, _i32],
    "sqnorm": [_vp, _i32, _vp, _i64, _vp, _vp],
    "prepare": [_vp, _i32, _vp, _i64, Groups, _i32, _f64, _f64, _i32, _vp, _vp, _vp, _vp, _vp],
    "adamw": [_vp, _i32, _vp, _i64, _vp, _vp, _vp],
}
_RESTYPES = {"last_error": C.c_char_p}


def _ptr(t: Optional[torch.Tensor]):
    """The address of a device buffer that holds records (any dtype); None -> NULL."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "a contiguous device buffer"
    return t.data_ptr()


def groups_by_value(hyper) -> Groups:
    """hyper: one (lr, beta1, beta2, eps, weight_decay) per group -> the struct po_prepare takes."""
    out = Groups()
    for i, h in enumerate(hyper):
        out.g[i] = Group(*(float(x) for x in h))
    return out


class OptimLib(FamilyLib):
    def __init__(self, path: Optional[str] = None):
        super().__init__("po_", PO_ABI_VERSION, _SIGNATURES, _RESTYPES, path)

    def table_check(self, n_tensors: int, max_n: int, total: int, n_groups: int):
        """Raises with the header's limit where a table of this size is not served.  Reads no device."""
        self._ok(self.lib.po_table_check(int(n_tensors), int(max_n), int(total), int(n_groups)), "table_check")

    def sqnorm(self, tensors: torch.Tensor, n_tensors: int, chunks: torch.Tensor, n_chunks: int, partials: torch.Tensor):
        """partials fp64 [n_chunks]: per chunk of the table the sum of its squared gradient elements."""
        assert partials.dtype == torch.float64 and partials.numel() >= n_chunks
        self._ok(self.lib.po_sqnorm(_ptr(tensors), n_tensors, _ptr(chunks), n_chunks, _ptr(partials), self._stream(partials)),
                 "sqnorm")

    def prepare(self, tensors, n_tensors: int, partials: torch.Tensor, n_chunks: int, hyper, max_norm: float, grad_scale: float,
                policy: int, states: torch.Tensor, scalars: torch.Tensor, result: torch.Tensor, step: torch.Tensor):
        """The partials summed, the result and step records written, the state records of the table's tensors advanced and
        their scalars written (include/pasco_optim.h po_prepare).  `hyper`: (lr, beta1, beta2, eps, weight_decay) per group."""
        if not 1 <= len(hyper) <= PO_MAX_GROUPS:
            raise ValueError(f"{len(hyper)} parameter groups; the kernels serve 1 .. PO_MAX_GROUPS = {PO_MAX_GROUPS}")
        self._ok(self.lib.po_prepare(_ptr(tensors), n_tensors, _ptr(partials), n_chunks, groups_by_value(hyper), len(hyper),
                                     float(max_norm), float(grad_scale), int(policy), _ptr(states), _ptr(scalars), _ptr(result),
                                     _ptr(step), self._stream(result)), "prepare")

    def adamw(self, tensors, n_tensors: int, chunks, n_chunks: int, scalars: torch.Tensor, step: torch.Tensor):
        """The update over every chunk of the table; returns at once on the device where the step record's flag is clear."""
        self._ok(self.lib.po_adamw(_ptr(tensors), n_tensors, _ptr(chunks), n_chunks, _ptr(scalars), _ptr(step),
                                   self._stream(step)), "adamw")


def optim_lib() -> OptimLib:
    """The process-wide binding of libpascohip.so's optimiser kernels (a missing library is an error)."""
    return shared(OptimLib)
