"""The ctypes binding of the pk_* family (pasco_amd/grad/knnlib.py) against include/pasco_knn.h, as
tests/test_field_bindings_cpu.py does it for pq_*: the same names, the same number of arguments and the same coarse type in every
position, the same ABI version; another version is refused; refusals on scalar arguments carry their text; sizes of 0 are no-ops;
libpascohip.so exports exactly the pk_ symbols the header declares; and the Python-level refusal of a backward whose list
pq_group cannot hold.  The library is loaded, nothing is launched: no GPU."""
import importlib
import re
import subprocess

import pytest
import torch

from tests import test_bindings_cpu as tb


def _pk_family(monkeypatch):
    monkeypatch.setitem(tb.FAMILIES, "pk", ("pasco_knn.h", "pasco_amd.grad.knnlib", "PK_ABI_VERSION", "KnnLib", "knn_lib"))
    return importlib.import_module("pasco_amd.grad.knnlib")


def test_pk_binding_table_matches_its_header(monkeypatch):
    mod = _pk_family(monkeypatch)
    protos, version = tb.prototypes("pk")
    assert len(protos) == 5
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"pk_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert tb.ctypes_coarse(t) == a, f"pk_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert tb.ctypes_coarse(mod._RESTYPES.get(name, tb.C.c_int)) == ret, f"pk_{name}: return type, the header says {ret}"
    assert mod.PK_ABI_VERSION == version == 1


def test_pk_constants_match_the_header():
    mod = importlib.import_module("pasco_amd.grad.knnlib")
    from pasco_amd.grad import fieldlib, host
    from pasco_amd.grad import knn as K
    from tests import knn_cases as kc
    src = open(tb.os.path.join(tb.ROOT, "include", "pasco_knn.h")).read()
    define = lambda name: int(re.search(rf"^#define {name}\s+(\d+)", src, flags=re.M).group(1))
    assert define("PK_MAX_K") == mod.PK_MAX_K == host.KNN_MAX_K == max(kc.KS) == 16
    assert define("PK_QUERY_BLOCK") == mod.PK_QUERY_BLOCK == kc.QB
    assert re.search(r"^#define PK_MAX_CELLS\s+\(1 << 24\)", src, flags=re.M) and mod.PK_MAX_CELLS == 1 << 24 >= K.MAX_CELLS
    assert mod.MAX_LIST == fieldlib.MAX_LIST
    waffle = open(tb.os.path.join(tb.ROOT, "include", "pasco_waffle.h")).read()
    assert re.search(r"^#define PW_MAX_CELLS\s+\(1 << 24\)", waffle, flags=re.M)


def test_pk_binding_rejects_other_abi_versions_and_keeps_its_error_text(monkeypatch):
    from pasco_amd.build import build_hip
    mod = _pk_family(monkeypatch)
    path = build_hip(verbose=False)
    lib = mod.KnnLib(path)
    L = lib.lib
    grid = (0.0, 0.0, 0.0, 1.0, 1, 1, 1)
    # refusals on scalar arguments, before anything touches the HIP runtime: nothing is launched, no pointer is read
    assert L.pk_knn(None, 3, 1, None, None, *grid, None, 3, 1, 0, None, None, None) == 1
    assert b"knn: k = 0 outside the served range [1, 16]" in L.pk_last_error()
    assert L.pk_abi_version() == 1 and b"knn: k = 0" in L.pk_last_error()                     # the text stays
    assert L.pk_knn(None, 3, 1, None, None, *grid, None, 3, 0, 3, None, None, None) == 0      # m == 0: a no-op
    assert L.pk_weights(None, None, 3, 0, None, None) == 0
    assert L.pk_interp_fwd(None, 1, 4, None, None, 3, 0, None, None) == 0
    assert b"knn: k = 0" in L.pk_last_error()
    assert L.pk_knn(None, 3, 1, None, None, *grid, None, 3, 1, 17, None, None, None) == 1 and b"knn: k = 17 outside" in L.pk_last_error()
    assert L.pk_knn(None, 2, 1, None, None, *grid, None, 3, 1, 3, None, None, None) == 1 and b"ldc = 2, ldq = 3" in L.pk_last_error()
    assert L.pk_knn(None, 4, 1, None, None, *grid, None, 2, 1, 3, None, None, None) == 1 and b"ldc = 4, ldq = 2" in L.pk_last_error()
    assert L.pk_knn(None, 3, -1, None, None, *grid, None, 3, 1, 3, None, None, None) == 1 and b"knn: n = -1" in L.pk_last_error()
    assert L.pk_knn(None, 3, 1, None, None, *grid, None, 3, 1 << 30, 3, None, None, None) == 1 and b"m * k < 2^31" in L.pk_last_error()
    assert L.pk_knn(None, 3, 1, None, None, 0.0, 0.0, 0.0, 0.0, 1, 1, 1, None, 3, 1, 3, None, None, None) == 1 and b"h = 0" in L.pk_last_error()
    assert L.pk_knn(None, 3, 1, None, None, 0.0, 0.0, 0.0, 1.0, 0, 1, 1, None, 3, 1, 3, None, None, None) == 1 and b"grid 0 x 1 x 1" in L.pk_last_error()
    assert L.pk_knn(None, 3, 1, None, None, 0.0, 0.0, 0.0, 1.0, 4096, 4096, 2, None, 3, 1, 3, None, None, None) == 1
    assert b"grid 4096 x 4096 x 2" in L.pk_last_error()
    assert L.pk_knn(None, 3, 1, None, None, *grid, None, 3, 1, 3, None, None, None) == 1 and b"knn: null pointer" in L.pk_last_error()
    assert L.pk_weights(None, None, 0, 1, None, None) == 1 and b"weights: k = 0" in L.pk_last_error()
    assert L.pk_weights(None, None, 17, 1, None, None) == 1 and b"weights: k = 17" in L.pk_last_error()
    assert L.pk_weights(None, None, 3, -1, None, None) == 1 and b"weights: m = -1" in L.pk_last_error()
    assert L.pk_interp_fwd(None, 1, 0, None, None, 3, 1, None, None) == 1 and b"interp_fwd: c = 0" in L.pk_last_error()
    assert L.pk_interp_fwd(None, 1, 4, None, None, 17, 1, None, None) == 1 and b"interp_fwd: k = 17" in L.pk_last_error()
    assert L.pk_interp_fwd(None, 1 << 31, 4, None, None, 3, 1, None, None) == 1 and b"interp_fwd: n = 2147483648" in L.pk_last_error()
    with pytest.raises(RuntimeError, match="pk_knn: interp_fwd: n = 2147483648"):
        lib._ok(1, "knn")
    monkeypatch.setattr(mod, "PK_ABI_VERSION", mod.PK_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        mod.KnnLib(path)


def test_library_exports_exactly_the_headers_pk_symbols(monkeypatch):
    from pasco_amd.build import build_hip
    _pk_family(monkeypatch)
    protos, _ = tb.prototypes("pk")
    out = subprocess.run(["nm", "-D", "--defined-only", build_hip(verbose=False)], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("pk_")}
    assert exported == {"pk_" + name for name in protos}, sorted(exported ^ {"pk_" + name for name in protos})


def test_backward_refuses_a_list_pq_group_cannot_hold():
    """k * m >= 2^24 list entries: refused with a message before anything is touched (shapes only: meta tensors)."""
    mod = importlib.import_module("pasco_amd.grad.knnlib")
    idx = torch.empty((16, 1 << 20), dtype=torch.int32, device="meta")
    w = torch.empty((16, 1 << 20), dtype=torch.float32, device="meta")
    dy = torch.empty((1 << 20, 4), dtype=torch.float32, device="meta")
    with pytest.raises(ValueError, match=r"k \* m = 16 \* 1048576 = 16777216 list entries, fewer than 2\^24"):
        mod.KnnLib.interp_bwd(None, dy, idx, w, 10)
    for k in (0, 17):
        with pytest.raises(ValueError, match="neighbours are served"):
            mod._check_k(k)
