"""What every ctypes binding of libpascohip.so shares: setting the signatures, the ABI handshake, the error path, the stream
handle and the process-wide instances.  `me.backend` (ph_*) uses `bind` and `_raw_stream`; the side families (pa_*, pe_*, pf_*, pg_*,
pl_*, pm_*, pn_*, po_*, pr_*, ps_*, pt_*, pv_*, pw_*) derive their binding class from `FamilyLib` and keep only their table and wrappers."""
from __future__ import annotations

import ctypes as C
import threading
from typing import Dict, Optional

import torch

# Raw handle of torch's current stream on a device index: the raw getter (0.3 us) instead of building a torch.cuda.Stream
# object (4 us).
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
if _raw_stream is None:      # older torch: the public (slower) route
    def _raw_stream(idx: int) -> int:
        return torch.cuda.current_stream(idx).cuda_stream


def bind(lib: C.CDLL, prefix: str, signatures: dict, restypes: dict) -> Dict[str, object]:
    """Give every `prefix + name` of `lib` its argtypes (`signatures`: name -> [argtypes]) and its return type (`restypes`, int
    unless listed).  Returns name -> function; a missing symbol is an error."""
    fn = {}
    for name, argtypes in signatures.items():
        f = getattr(lib, prefix + name)
        f.argtypes, f.restype = argtypes, restypes.get(name, C.c_int)
        fn[name] = f
    return fn


def dev_ptr(t: torch.Tensor, dtype, what: str) -> int:
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), f"{what}: a contiguous {dtype} device tensor"
    return t.data_ptr()


class FamilyLib:
    """One side family of entry points (`prefix` = "pe_", ...) bound from the library at `path` (default: the path
    `me.backend.HIP_LIB_PATH` names NOW, so a redirect made before the first use covers every family).  A library built from
    another version of the family's header is refused before anything is called."""

    def __init__(self, prefix: str, abi_version: int, signatures: dict, restypes: dict, path: Optional[str] = None):
        if path is None:
            from .me import backend
            path = backend.HIP_LIB_PATH
        self.prefix = prefix
        self.lib = C.CDLL(path)
        fn = bind(self.lib, prefix, signatures, restypes)
        self._last_error = fn["last_error"]
        v = fn["abi_version"]()
        if v != abi_version:
            raise RuntimeError(f"{path}: {prefix[:-1]} ABI {v}, this binding needs {abi_version}; rebuild (pasco_amd/build.py)")

    def _ok(self, rc: int, what: str):
        if rc != 0:
            raise RuntimeError(f"{self.prefix}{what}: {self._last_error().decode()}")

    @staticmethod
    def _stream(t: torch.Tensor):
        """torch's current stream on the device of `t`, as the `void *stream` every launch takes."""
        return C.c_void_p(_raw_stream(t.device.index))


_INSTANCES: Dict[type, FamilyLib] = {}
_LOCK = threading.Lock()


def shared(cls):
    """The process-wide instance of the binding class `cls` (a missing library is an error)."""
    with _LOCK:
        lib = _INSTANCES.get(cls)
        if lib is None:
            lib = _INSTANCES[cls] = cls()
        return lib
