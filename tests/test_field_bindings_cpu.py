"""The ctypes binding of the pq_* family (pasco_amd/grad/fieldlib.py) against include/pasco_field.h, as
tests/test_bindings_cpu.py does for the families of its table: the same names, the same number of arguments and the same coarse
type in every position, the same ABI version; another version is refused; refusals on scalar arguments carry their text; sizes
of 0 are no-ops; and libpascohip.so exports exactly the pq_ symbols the header declares.  The library is loaded, nothing is
launched: no GPU."""
import importlib
import re
import subprocess

import pytest

from tests import test_bindings_cpu as tb


def _pq_family(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pq", ("pasco_field.h", "pasco_amd.grad.fieldlib", "PQ_ABI_VERSION", "FieldLib", "field_lib"))
    return importlib.import_module("pasco_amd.grad.fieldlib")


def test_pq_binding_table_matches_its_header(monkeypatch):
    mod = _pq_family(monkeypatch)
    protos, version = tb.prototypes("pq")
    assert len(protos) == 9
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pq_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert tb.ctypes_coarse(t) == a, f"pq_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, tb.C.c_int)) == ret, f"pq_{name}: return type, the header says {ret}"
    assert mod.PQ_ABI_VERSION == version == 1


def test_pq_constants_match_the_header():
    mod = importlib.import_module("pasco_amd.grad.fieldlib")
    from pasco_amd.grad import host
    from tests import field_cases as fc
    src = open(tb.os.path.join(tb.ROOT, "include", "pasco_field.h")).read()
    define = lambda name: int(re.search(rf"^#define {name}\s+(\d+)", src, flags=re.M).group(1))
    assert define("PQ_SEG_ROWS") == mod.PQ_SEG_ROWS == fc.SEG_ROWS
    assert define("PQ_CORNERS") == mod.PQ_CORNERS == host.FIELD_CORNERS == 8
    assert (define("PQ_SUM"), define("PQ_AVG"), define("PQ_MAX")) == (mod.SUM, mod.AVG, mod.MAX) == (host.FIELD_SUM, host.FIELD_AVG, host.FIELD_MAX)
    from pasco_amd.me.core import _Q_REDUCE, SparseTensorQuantizationMode as Q
    assert _Q_REDUCE == {Q.UNWEIGHTED_SUM: mod.SUM, Q.UNWEIGHTED_AVERAGE: mod.AVG, Q.MAX_POOL: mod.MAX}


def test_pq_binding_rejects_other_abi_versions_and_keeps_its_error_text(monkeypatch):
    from pasco_amd.build import build_hip
    mod = _pq_family(monkeypatch)
    path = build_hip(verbose=False)
    lib = mod.FieldLib(path)                                  # the version it was written against binds
    L = lib.lib
    # refusals on scalar arguments, before anything touches the HIP runtime: nothing is launched, no pointer is read
    assert L.pq_seg_rows(None, 1, 4, None, None, 1 << 24, 1, None, 1, 0, None, None, None, None) == 1
    assert b"seg_rows: n_list = 16777216 outside the served range (n < 2^24)" in L.pq_last_error()
    assert L.pq_abi_version() == 1 and b"seg_rows: n_list = 16777216" in L.pq_last_error()          # the text stays
    assert L.pq_seg_rows(None, 1, 4, None, None, 1, 0, None, 1, 0, None, None, None, None) == 0       # n_seg == 0: a no-op
    assert L.pq_gather_w(None, 1, 4, None, 0, None, None, None) == 0                                 # n == 0
    assert L.pq_interp_map(None, 0, None, None, 8, 1, None, None, None) == 0                         # m == 0
    assert L.pq_interp_fwd(None, 1, 4, None, None, 0, None, None) == 0
    assert L.pq_seg_max_bwd(None, None, 1, 4, 0, 1, None, None) == 0                                 # n_src == 0
    assert b"seg_rows: n_list = 16777216" in L.pq_last_error()
    assert L.pq_seg_rows(None, 1, 0, None, None, 1, 1, None, 1, 0, None, None, None, None) == 1 and b"seg_rows: c = 0" in L.pq_last_error()
    assert L.pq_seg_rows(None, 1, 4, None, None, 1, 1, None, 1, 3, None, None, None, None) == 1 and b"seg_rows: mode = 3" in L.pq_last_error()
    assert L.pq_seg_rows(None, 1, 4, None, None, 1, -1, None, 1, 0, None, None, None, None) == 1 and b"seg_rows: n_seg = -1" in L.pq_last_error()
    assert L.pq_seg_rows(None, 1, 4, None, None, 1, 1, None, 0, 0, None, None, None, None) == 1 and b"src_mod = 0" in L.pq_last_error()
    assert L.pq_group(None, 1 << 24, 1, None, None, None, 0, None) == 1 and b"group: n = 16777216 outside the served range (n < 2^24)" in L.pq_last_error()
    assert L.pq_group(None, 1, -1, None, None, None, 0, None) == 1 and b"group: n_seg = -1" in L.pq_last_error()
    assert L.pq_group(None, 1, 1 << 31, None, None, None, 0, None) == 1 and b"group: n_seg = 2147483648" in L.pq_last_error()
    assert L.pq_gather_w(None, 1, 0, None, 1, None, None, None) == 1 and b"gather_w: c = 0" in L.pq_last_error()
    assert L.pq_seg_max_bwd(None, None, 1, 0, 1, 1, None, None) == 1 and b"seg_max_bwd: c = 0" in L.pq_last_error()
    assert L.pq_interp_map(None, 1, None, None, 12, 1, None, None, None) == 1 and b"cap = 12 must be a power of two" in L.pq_last_error()
    assert L.pq_interp_map(None, 1, None, None, 8, 0, None, None, None) == 1 and b"tensor stride 0" in L.pq_last_error()
    assert L.pq_interp_fwd(None, 1, 0, None, None, 1, None, None) == 1 and b"interp_fwd: c = 0" in L.pq_last_error()
    assert L.pq_interp_fwd(None, 1, 4, None, None, 1 << 28, None, None) == 1 and b"m < 2^28" in L.pq_last_error()
    assert L.pq_group_workspace_bytes(1 << 24, 1) == -1 and L.pq_group_workspace_bytes(1, -1) == -1
    assert L.pq_group_workspace_bytes(0, 5) == 0 and L.pq_group_workspace_bytes(2049, 5) == 3 * 8448 + 2 * 256 * 4
    with pytest.raises(RuntimeError, match="pq_seg_rows: interp_fwd: m = 268435456"):
        lib._ok(1, "seg_rows")
    monkeypatch.setattr(mod, "PQ_ABI_VERSION", mod.PQ_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.FieldLib(path)


def test_library_exports_exactly_the_headers_pq_symbols(monkeypatch):
    from pasco_amd.build import build_hip
    _pq_family(monkeypatch)
    protos, _ = tb.prototypes("pq")
    out = subprocess.run(["nm", "-D", "--defined-only", build_hip(verbose=False)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("pq_")}
    assert exported == {"pq_" + name for name in protos}, sorted(exported ^ {"pq_" + name for name in protos})
