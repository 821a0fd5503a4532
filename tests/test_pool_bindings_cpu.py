"""The ctypes binding of the pp_* family (pasco_amd/grad/poollib.py) against include/pasco_pool.h, as tests/test_bindings_cpu.py
does for the families of its table: the same names, the same number of arguments and the same coarse type in every position, the
same ABI version; another version is refused; refusals on scalar arguments carry their text; and libpascohip.so exports exactly
the pp_ symbols the header declares.  The library is loaded, nothing is launched: no GPU."""
import importlib
import re
import subprocess

import pytest

from tests import test_bindings_cpu as tb


def _pp_family(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pp", ("pasco_pool.h", "pasco_amd.grad.poollib", "PP_ABI_VERSION", "PoolLib", "pool_lib"))
    return importlib.import_module("pasco_amd.grad.poollib")


def test_pp_binding_table_matches_its_header(monkeypatch):
    mod = _pp_family(monkeypatch)
    protos, version = tb.prototypes("pp")
    assert len(protos) == 12
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pp_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert tb.ctypes_coarse(t) == a, f"pp_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, tb.C.c_int)) == ret, f"pp_{name}: return type, the header says {ret}"
    assert mod.PP_ABI_VERSION == version == 1


def test_pp_constants_match_the_header():
    mod = importlib.import_module("pasco_amd.grad.poollib")
    from pasco_amd.grad import host
    from tests import pool_cases as pc
    src = open(tb.os.path.join(tb.ROOT, "include", "pasco_pool.h")).read()
    define = lambda name: int(re.search(rf"^#define {name}\s+(\d+)", src, flags=re.M).group(1))
    assert (define("PP_MAX_KVOL"), define("PP_MAX_BATCH"), define("PP_SEG_ROWS")) == (mod.PP_MAX_KVOL, mod.PP_MAX_BATCH, mod.PP_SEG_ROWS)
    assert (pc.MAX_KVOL, pc.MAX_BATCH, pc.SEG_ROWS) == (mod.PP_MAX_KVOL, mod.PP_MAX_BATCH, mod.PP_SEG_ROWS)
    assert (define("PP_SUM"), define("PP_AVG"), define("PP_MAX")) == (mod.SUM, mod.AVG, mod.MAX) == (host.POOL_SUM, host.POOL_AVG, host.POOL_MAX)
    assert (define("PP_BC_ADD"), define("PP_BC_MUL"), define("PP_BC_CAT"), define("PP_BC_COPY")) == \
        (mod.BC_ADD, mod.BC_MUL, mod.BC_CAT, mod.BC_COPY) == (host.POOL_BC_ADD, host.POOL_BC_MUL, host.POOL_BC_CAT, host.POOL_BC_COPY)


def test_pp_binding_rejects_other_abi_versions_and_keeps_its_error_text(monkeypatch):
    from pasco_amd.build import build_hip
    mod = _pp_family(monkeypatch)
    path = build_hip(verbose=False)
    lib = mod.PoolLib(path)                                  # the version it was written against binds
    L = lib.lib
    # refusals on scalar arguments, before anything touches the HIP runtime: nothing is launched, no pointer is read
    assert L.pp_seg_reduce(None, 1, 4, 4, None, mod.PP_MAX_BATCH + 1, 0, None, None, None, None, 0, None) == 1
    assert b"seg_reduce: B = 65 outside [1, 64] (PP_MAX_BATCH)" in L.pp_last_error()
    assert L.pp_abi_version() == 1 and b"seg_reduce: B = 65" in L.pp_last_error()                  # the text stays
    assert L.pp_pool(None, 1, 4, None, 8, 0, 0, None, None, None) == 0                              # n_out == 0: a no-op
    assert b"seg_reduce: B = 65" in L.pp_last_error()
    assert L.pp_seg_reduce(None, 1 << 24, 4, 4, None, 1, 0, None, None, None, None, 0, None) == 1 and b"n < 2^24" in L.pp_last_error()
    assert L.pp_seg_reduce(None, 1, 4, 3, None, 1, 0, None, None, None, None, 0, None) == 1 and b"ldx = 3 below c = 4" in L.pp_last_error()
    assert L.pp_broadcast(None, 1, 4, None, 5, None, 1, None, 0, None, None) == 1 and b"cg = 5, must equal c = 4" in L.pp_last_error()
    assert L.pp_broadcast(None, 1, 4, None, 4, None, 0, None, 0, None, None) == 1 and b"broadcast: B = 0" in L.pp_last_error()
    assert L.pp_broadcast_mul_bwd(None, None, None, None, 1, 4, 65, None, None, None, 0, None) == 1 and b"PP_MAX_BATCH" in L.pp_last_error()
    assert L.pp_seg_max_bwd(None, None, 1, 0, 1, None, None) == 1 and b"seg_max_bwd: c = 0" in L.pp_last_error()
    assert L.pp_pool(None, 1, 4, None, 65, 1, 0, None, None, None) == 1 and b"pool: K = 65 outside [1, 64]" in L.pp_last_error()
    assert L.pp_pool(None, 1, 4, None, 8, 1, 2, None, None, None) == 1 and b"pool: mode = 2" in L.pp_last_error()
    assert L.pp_pool_bwd(None, 1, 4, None, None, 0, 1, 0, None, None) == 1 and b"pool_bwd: K = 0" in L.pp_last_error()
    assert L.pp_chconv_fwd(None, 1, 0, None, 27, 1, None, None, None, None) == 1 and b"chconv_fwd: c = 0" in L.pp_last_error()
    assert L.pp_chconv_wgrad(None, 1, 4, None, 1, None, 65, None, None, 0, None) == 1 and b"chconv_wgrad: K = 65" in L.pp_last_error()
    assert L.pp_seg_workspace_bytes(1, 4, 65) == -1 and L.pp_seg_workspace_bytes(1 << 24, 4, 1) == -1
    assert L.pp_seg_workspace_bytes(0, 4, 3) == 12 and L.pp_seg_workspace_bytes(257, 4, 3) == (2 * 2 * 3 * 4 + 2 * 3 + 3) * 4
    assert L.pp_chconv_wgrad_workspace_bytes(65, 4, 1) == -1 and L.pp_chconv_wgrad_workspace_bytes(27, 5, 257) == 2 * 27 * 5 * 4
    with pytest.raises(RuntimeError, match="pp_chconv_wgrad: chconv_wgrad: K = 65"):
        lib._ok(1, "chconv_wgrad")
    monkeypatch.setattr(mod, "PP_ABI_VERSION", mod.PP_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.PoolLib(path)


def test_library_exports_exactly_the_headers_pp_symbols(monkeypatch):
    from pasco_amd.build import build_hip
    _pp_family(monkeypatch)
    protos, _ = tb.prototypes("pp")
    out = subprocess.run(["nm", "-D", "--defined-only", build_hip(verbose=False)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("pp_")}
    assert exported == {"pp_" + name for name in protos}, sorted(exported ^ {"pp_" + name for name in protos})
