"""What every ctypes binding of libpascohip.so shares: setting the signatures, the ABI handshake, the error path, the stream
handle, the per-stream scratch table and the process-wide instances.  `me.backend` (ph_*) uses `bind`, `_raw_stream` and
`StreamScratch`; the side families (pa_*, pe_*, pf_*, pg_*, pk_*, pl_*, pm_*, pn_*, po_*, pp_*, pq_*, pr_*, ps_*, pt_*, pv_*, pw_*) derive their
binding class from `FamilyLib` and keep only their table and wrappers."""
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


class StreamScratch:
    """Every buffer a backend reuses from launch to launch.  Reuse is only safe in stream order, so there is one set per
    (device, stream): the table is keyed (name, device, raw stream handle).  One instance per `CBackend` (`be.scratch`): the
    oracle and the product backend keep separate status words."""

    def __init__(self):
        self._table: Dict[tuple, torch.Tensor] = {}
        self._status_ptrs: Dict[tuple, int] = {}     # (device type, index, handle) -> address of the status pair: derived, see status_ptr

    @staticmethod
    def key(device: torch.device) -> tuple:
        """(device, raw handle of torch's current stream on it); `cuda` without an index is the current device, the handle is 0 off cuda."""
        if device.type != "cuda":
            return (device, 0)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        return (device, _raw_stream(device.index) or 0)

    def bytes(self, name: str, device: torch.device, need: int, floor: int = 0) -> torch.Tensor:
        """uint8 scratch of at least `need` bytes; a new one has max(need, floor)."""
        k = (name,) + self.key(device)
        t = self._table.get(k)
        if t is None or t.numel() < need:
            t = None                           # the smaller buffer goes before the larger one is allocated (same stream)
            self._table.pop(k, None)
            t = self._table[k] = torch.empty(max(need, floor), dtype=torch.uint8, device=device)
        return t

    def words(self, name: str, device, n: int) -> torch.Tensor:
        """int32 [n], zero when made; never cleared here again."""
        k = (name,) + self.key(torch.device(device))
        t = self._table.get(k)
        if t is None:
            # cleared in place by every later `check_status`: a pair first made under torch.inference_mode() would be an
            # inference tensor, which no call outside that mode may write to
            with torch.inference_mode(False):
                t = self._table[k] = torch.zeros(n, dtype=torch.int32, device=device)
        return t

    def status_ptr(self, device: torch.device) -> int:
        """Address of words("status", device, 2).  ~260 calls per step: looked up by (device index, raw stream handle) without
        building a torch.device, a key tuple or a view."""
        idx = device.index
        if idx is None and device.type == "cuda":
            idx = torch.cuda.current_device()
        k = (device.type, idx, _raw_stream(idx) if device.type == "cuda" else 0)
        hit = self._status_ptrs.get(k)
        if hit is None:
            hit = self._status_ptrs[k] = self.words("status", device, 2).data_ptr()
        return hit

    def get(self, name: str, device) -> Optional[torch.Tensor]:
        return self._table.get((name,) + self.key(torch.device(device)))

    def _keys(self, stream) -> list:
        """The keys of `stream`: a torch.cuda.Stream, or a raw handle = the streams of the current device.  Entries off cuda have
        no stream: handle 0 means them whatever the current device is."""
        handle = int(getattr(stream, "cuda_stream", stream) or 0)
        dev = getattr(stream, "device", None)
        if dev is None and torch.cuda.is_available():
            dev = torch.device("cuda", torch.cuda.current_device())
        return [k for k in self._table if k[2] == handle and (dev is None or k[1] == dev or k[1].type != "cuda")]

    def held(self, stream=None) -> set:
        """The names held (for `stream` only, if given)."""
        return {k[0] for k in (self._table if stream is None else self._keys(stream))}

    def _forget(self, keys) -> int:
        for k in keys:
            del self._table[k]
        self._status_ptrs.clear()              # addresses into the table: rebuilt from it on the next miss
        return len(keys)

    def drop(self, name: str, device=None) -> int:
        """Forget `name` on every stream, or on the current stream of `device` only."""
        at = None if device is None else self.key(torch.device(device))
        return self._forget([k for k in self._table if k[0] == name and at in (None, k[1:])])

    def release(self, stream) -> int:
        """Forget everything held for `stream`; -> the number of buffers dropped."""
        return self._forget(self._keys(stream))


_INSTANCES: Dict[type, FamilyLib] = {}
_LOCK = threading.Lock()


def shared(cls):
    """The process-wide instance of the binding class `cls` (a missing library is an error)."""
    with _LOCK:
        lib = _INSTANCES.get(cls)
        if lib is None:
            lib = _INSTANCES[cls] = cls()
        return lib
