"""The ctypes binding of the `ps_*` family (pasco_amd/grad/semlib.py) against include/pasco_semloss.h, as
tests/test_match_bindings_cpu.py does for `pm_*`: the same names, the same number of arguments, the same coarse type in every
position and for the return value, the same ABI version; a library of another version is refused; the family's error text stays
its own.  The library is loaded, nothing is launched: no GPU."""
import ctypes as C
import os
import re

import pytest

from tests.test_bindings_cpu import c_coarse, ctypes_coarse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PROTOTYPES = 9


def prototypes():
    src = open(os.path.join(ROOT, "include", "pasco_semloss.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    version = int(re.search(r"^\s*#\s*define PS_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1))
    src = re.sub(r"^\s*#(?:[^\n]*\\\n)*[^\n]*", " ", src, flags=re.M)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\bPS_FN\((\w+)\)\s*\(([^()]*)\)\s*;", src):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        ret = re.split(r"[;{}]", ret)[-1].strip()
        assert name not in out, name
        out[name] = (c_coarse(ret), [] if args == "void" else [c_coarse(a) for a in args.split(",")])
    return out, version


def test_sem_binding_table_matches_its_header():
    from pasco_amd.grad import semlib as mod
    protos, version = prototypes()
    assert len(protos) == N_PROTOTYPES
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"ps_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert ctypes_coarse(t) == a, f"ps_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert ctypes_coarse(mod._RESTYPES.get(name, C.c_int)) == ret, f"ps_{name}: return type, the header says {ret}"
    assert mod.PS_ABI_VERSION == version == 1
    assert protos["workspace_bytes"] == ("i64", ["i64", "i32"])
    assert protos["sort_desc"] == ("i32", ["ptr", "i64", "i64", "ptr", "ptr", "i64", "ptr"])
    header = open(os.path.join(ROOT, "include", "pasco_semloss.h")).read()
    for name, value in (("PS_MIN_C", mod.PS_MIN_C), ("PS_MAX_C", mod.PS_MAX_C), ("PS_SORT_TILE", mod.SORT_TILE),
                        ("PS_LABEL_IGNORE", mod.LABEL_IGNORE), ("PS_LABEL_OUTSIDE", mod.LABEL_OUTSIDE),
                        ("PS_GEOMETRY_WORDS", len(mod.GEOMETRY_WORDS))):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value, name


def test_sem_binding_rejects_other_abi_versions(monkeypatch):
    from pasco_amd.build import build_hip
    from pasco_amd.grad import semlib as mod
    path = build_hip(verbose=False)
    mod.SemLib(path)
    monkeypatch.setattr(mod, "PS_ABI_VERSION", mod.PS_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.SemLib(path)


def test_sem_error_text_stays_with_its_family():
    """A refusal on a scalar argument (no pointer is read, the HIP runtime is not touched) shows in ps_last_error() and in no
    other family's text."""
    from pasco_amd.grad.matchlib import match_lib
    from pasco_amd.grad.semlib import sem_lib
    L, A = sem_lib(), match_lib()
    assert L is sem_lib()
    before = A.lib.pm_last_error()
    rc = L.lib.ps_rows_fwd(None, None, None, None, 1, None, 4, 33, 1, 1, 1, None, None, None, None, None, None, 0, None)
    assert rc != 0 and b"ps_rows_fwd" in L.lib.ps_last_error() and b"33 classes" in L.lib.ps_last_error()
    assert A.lib.pm_last_error() == before and b"ps_rows_fwd" not in A.lib.pm_last_error()
    with pytest.raises(RuntimeError, match="ps_rows_fwd"):
        L._ok(rc, "rows_fwd")
    rc = L.lib.ps_sort_desc(None, 0, 5, None, None, 0, None)
    assert rc != 0 and b"0 segments" in L.lib.ps_last_error()
    rc = L.lib.ps_loss_bwd(None, None, None, None, None, None, None, (1 << 24) + 1, 20, None, None)
    assert rc != 0 and b"rows not served" in L.lib.ps_last_error()
