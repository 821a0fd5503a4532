"""The ctypes binding of the `pm_*` family (pasco_amd/grad/matchlib.py) against include/pasco_match.h, as
tests/test_bindings_cpu.py does for the families it lists: the same names, the same number of arguments, the same coarse type in
every position and for the return value, the same ABI version; a library of another version is refused; the family's error text
stays its own.  The library is loaded, nothing is launched: no GPU."""
import ctypes as C
import os
import re

import pytest

from tests.test_bindings_cpu import c_coarse, ctypes_coarse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PROTOTYPES = 8


def prototypes():
    src = open(os.path.join(ROOT, "include", "pasco_match.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    version = int(re.search(r"^\s*#\s*define PM_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1))
    src = re.sub(r"^\s*#(?:[^\n]*\\\n)*[^\n]*", " ", src, flags=re.M)
    out = {}
    for m in re.finditer(r"([\w\s\*]+?)\bPM_FN\((\w+)\)\s*\(([^()]*)\)\s*;", src):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        ret = re.split(r"[;{}]", ret)[-1].strip()
        assert name not in out, name
        out[name] = (c_coarse(ret), [] if args == "void" else [c_coarse(a) for a in args.split(",")])
    return out, version


def test_match_binding_table_matches_its_header():
    from pasco_amd.grad import matchlib as mod
    protos, version = prototypes()
    assert len(protos) == N_PROTOTYPES
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pm_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert ctypes_coarse(t) == a, f"pm_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert ctypes_coarse(mod._RESTYPES.get(name, C.c_int)) == ret, f"pm_{name}: return type, the header says {ret}"
    assert mod.PM_ABI_VERSION == version == 1
    assert protos["assign"] == ("i32", ["ptr", "i32", "i32", "ptr", "ptr"])
    assert protos["pair_sums_workspace_bytes"] == ("i64", ["i64", "i32", "i32"])


def test_match_binding_rejects_other_abi_versions(monkeypatch):
    from pasco_amd.build import build_hip
    from pasco_amd.grad import matchlib as mod
    path = build_hip(verbose=False)
    mod.MatchLib(path)
    monkeypatch.setattr(mod, "PM_ABI_VERSION", mod.PM_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.MatchLib(path)


def test_match_error_text_stays_with_its_family():
    """A refusal on a scalar argument (no pointer is read, the HIP runtime is not touched) shows in pm_last_error() and in no
    other family's text; the header says which entry takes host pointers."""
    from pasco_amd.grad.attnlib import attn_grad_lib
    from pasco_amd.grad.matchlib import match_lib
    L, A = match_lib(), attn_grad_lib()
    assert L is match_lib()
    before = A.lib.pa_last_error()
    rc = L.lib.pm_pair_sums(None, None, None, 0, 1, 129, 1, None, None, None, None, None, 0, None)
    assert rc != 0 and b"pm_pair_sums" in L.lib.pm_last_error() and b"129 queries" in L.lib.pm_last_error()
    assert A.lib.pa_last_error() == before and b"pm_pair_sums" not in A.lib.pa_last_error()
    with pytest.raises(RuntimeError, match="pm_pair_sums"):
        L._ok(rc, "pair_sums")
    header = open(os.path.join(ROOT, "include", "pasco_match.h")).read()
    assert "HOST pointers" in header
