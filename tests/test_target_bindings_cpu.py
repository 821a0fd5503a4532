"""The ctypes binding of the `pt_*` family (pasco_amd/data/target_lib.py) against include/pasco_target.h, as
tests/test_bindings_cpu.py does for the families it lists (its parser, pointed at this header): the same names, the same number
of arguments, the same coarse type in every position and for the return value, the same ABI version; a library of another
version is refused; the family's error text stays its own.  The library is loaded, nothing is launched: no GPU."""
import ctypes as C
import os
import re

import pytest

from tests import test_bindings_cpu as tb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PROTOTYPES = 9


@pytest.fixture
def protos(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pt", ("pasco_target.h", "pasco_amd.data.target_lib", "PT_ABI_VERSION", "TargetLib", "target_lib"))
    return tb.prototypes("pt")


def test_target_binding_table_matches_its_header(protos):
    from pasco_amd.data import target_lib as mod
    table, version = protos
    assert len(table) == N_PROTOTYPES
    assert set(table) == set(mod._SIGNATURES), sorted(set(table) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in table.items():
        sig = mod._SIGNATURES[name]
        assert len(sig) == len(args), f"pt_{name}: {len(sig)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(sig, args)):
            assert tb.ctypes_coarse(t) == a, f"pt_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, C.c_int)) == ret, f"pt_{name}: return type, the header says {ret}"
    assert mod.PT_ABI_VERSION == version == 1
    assert table["presence"] == ("i32", ["ptr", "ptr", "i64", "ptr", "ptr"])
    assert table["resample_workspace_bytes"] == ("i64", ["i32"])
    header = open(os.path.join(ROOT, "include", "pasco_target.h")).read()
    for name, value in (("PT_MAX_M", mod.MAX_M), ("PT_BOUNDS", mod.BOUNDS), ("PT_CROP_BOUNDS", mod.CROP_BOUNDS),
                        ("PT_TABLE", mod.TABLE), ("PT_MAX_T", mod.MAX_T)):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value, name
    from pasco_amd.data.frame_lib import MAX_M
    from pasco_amd.grad.matchlib import PM_MAX_T
    assert mod.MAX_M == MAX_M and mod.MAX_T == PM_MAX_T


def test_subnet_out_layout_matches_c(tmp_path):
    """The ctypes mirror of `pt_subnet_out` has the C layout."""
    import subprocess
    from pasco_amd.data.target_lib import SubnetOut
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "pasco_target.h"\nint main(){printf("%zu %zu %zu %zu", '
            'sizeof(pt_subnet_out), offsetof(pt_subnet_out, sem_4), offsetof(pt_subnet_out, min_C), offsetof(pt_subnet_out, scene));'
            ' return 0;}')
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(prog)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_sem4, o_min, o_scene = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert C.sizeof(SubnetOut) == size
    assert (SubnetOut.sem_4.offset, SubnetOut.min_C.offset, SubnetOut.scene.offset) == (o_sem4, o_min, o_scene)


def test_target_binding_rejects_other_abi_versions(monkeypatch):
    from pasco_amd.build import build_hip
    from pasco_amd.data import target_lib as mod
    path = build_hip(verbose=False)
    mod.TargetLib(path)
    monkeypatch.setattr(mod, "PT_ABI_VERSION", mod.PT_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.TargetLib(path)


def test_target_error_text_stays_with_its_family():
    """A refusal on a scalar argument (no pointer is read, the HIP runtime is not touched) shows in pt_last_error() and in no
    other family's text."""
    from pasco_amd.data.frame_lib import frame_lib
    from pasco_amd.data.target_lib import target_lib
    L, A = target_lib(), frame_lib()
    assert L is target_lib()
    before = A.lib.pf_last_error()
    rc = L.lib.pt_resample(None, None, 4, 4, 4, None, None, 9, None, None, None, 0, None, None, 0, None)      # M = 9
    assert rc != 0 and b"pt_resample" in L.lib.pt_last_error() and b"M = 9" in L.lib.pt_last_error()
    assert A.lib.pf_last_error() == before and b"pt_resample" not in A.lib.pf_last_error()
    with pytest.raises(RuntimeError, match="pt_resample"):
        L._ok(rc, "resample")
    rc = L.lib.pt_target_pack(None, None, None, None, None, None, 0, 129, 1, 1, 1, 0, 0, 0, None, None, None, None)
    assert rc != 0 and b"129 targets" in L.lib.pt_last_error()
    rc = L.lib.pt_masks(None, None, 6, None, None, 1, None, None)
    assert rc != 0 and b"multiple of 4" in L.lib.pt_last_error()
    rc = L.lib.pt_labels(None, None, 0, None, 1, None, None, 300, None, None)
    assert rc != 0 and b"300 classes" in L.lib.pt_last_error()
