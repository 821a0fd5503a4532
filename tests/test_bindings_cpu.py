"""The six ctypes bindings of libpascohip.so against the headers they mirror (include/pasco_*.h): the same names, the same
number of arguments, the same coarse type (pointer / 32- or 64-bit integer with its signedness / float / double) in every
position and for the return value, and the same ABI version.  Then the two things the side families share through
pasco_amd/_clib.py and pasco_amd/csrc/side_common.h: a library of another version is refused, and one family's error text
never shows up as another's.  The library is loaded, nothing is launched: no GPU."""
import ctypes as C
import importlib
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# prefix -> (header, binding module, name of its version constant, binding class, accessor)
FAMILIES = {
    "ph": ("pasco_hip.h", "pasco_amd.me.backend", "ABI_VERSION", None, None),
    "pe": ("pasco_eval.h", "pasco_amd.eval.lib", "PE_ABI_VERSION", "EvalLib", "eval_lib"),
    "pf": ("pasco_frame.h", "pasco_amd.data.frame_lib", "PF_ABI_VERSION", "FrameLib", "frame_lib"),
    "pl": ("pasco_label.h", "pasco_amd.data.label_lib", "PL_ABI_VERSION", "LabelLib", "label_lib"),
    "pv": ("pasco_view.h", "pasco_amd.viz.lib", "PV_ABI_VERSION", "ViewLib", "view_lib"),
    "pw": ("pasco_waffle.h", "pasco_amd.waffle.lib", "PW_ABI_VERSION", "WaffleLib", "waffle_lib"),
}
SIDE = [p for p in FAMILIES if p != "ph"]
N_PROTOTYPES = {"ph": 47, "pe": 8, "pf": 8, "pl": 5, "pv": 9, "pw": 13}

C_SCALARS = {"int": "i32", "int32_t": "i32", "uint32_t": "u32", "unsigned": "u32", "int64_t": "i64", "uint64_t": "u64",
             "float": "f32", "double": "f64"}


def c_coarse(decl: str, aliases=()) -> str:
    """Coarse type of one C parameter or return declaration (`const float *x`, `int32_t n`, `const char *`); `aliases` = the
    header's own scalar typedefs, name -> coarse type."""
    if "*" in decl or "[" in decl:
        return "ptr"
    known = {**C_SCALARS, **dict(aliases)}
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in known, decl
    assert len(words) <= 2, decl          # the type and, in a parameter, its name
    return known[words[0]]


def ctypes_coarse(t) -> str:
    if t is C.c_void_p or t is C.c_char_p or issubclass(t, C._Pointer):
        return "ptr"
    if t is C.c_float:
        return "f32"
    if t is C.c_double:
        return "f64"
    for signed, name in ((True, "i"), (False, "u")):
        for bits, types in ((32, (C.c_int32, C.c_int) if signed else (C.c_uint32, C.c_uint)),
                            (64, (C.c_int64, C.c_longlong) if signed else (C.c_uint64, C.c_ulonglong))):
            if t in types:
                assert C.sizeof(t) * 8 == bits
                return f"{name}{bits}"
    raise AssertionError(f"no coarse type for {t}")


def prototypes(prefix: str):
    """name -> (return type, [argument types]) of every `P?_FN(name)(...)` prototype of the family's header, coarse; and
    the header's `*_ABI_VERSION`."""
    src = open(os.path.join(ROOT, "include", FAMILIES[prefix][0])).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    version = int(re.search(rf"^\s*#\s*define {prefix.upper()}_ABI_VERSION\s+(\d+)", src, flags=re.M).group(1))
    src = re.sub(r"^\s*#(?:[^\n]*\\\n)*[^\n]*", " ", src, flags=re.M)        # preprocessor lines with their continuations
    aliases = {m.group(2): c_coarse(m.group(1)) for m in re.finditer(r"\btypedef\s+([^;{}]*?)(\w+)\s*;", src)}
    out = {}
    for m in re.finditer(rf"([\w\s\*]+?)\b{prefix.upper()}_FN\((\w+)\)\s*\(([^()]*)\)\s*;", src):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        ret = re.split(r"[;{}]", ret)[-1].strip()
        assert name not in out, name
        out[name] = (c_coarse(ret, aliases), [] if args == "void" else [c_coarse(a, aliases) for a in args.split(",")])
    return out, version


@pytest.mark.parametrize("prefix", list(FAMILIES))
def test_binding_table_matches_its_header(prefix):
    mod = importlib.import_module(FAMILIES[prefix][1])
    protos, version = prototypes(prefix)
    assert len(protos) == N_PROTOTYPES[prefix]
    assert set(protos) == set(mod._SIGNATURES), sorted(set(protos) ^ set(mod._SIGNATURES))
    assert set(mod._RESTYPES) <= set(mod._SIGNATURES)
    for name, (ret, args) in protos.items():
        table = mod._SIGNATURES[name]
        assert len(table) == len(args), f"{prefix}_{name}: {len(table)} argtypes, the header has {len(args)} parameters"
        for i, (t, a) in enumerate(zip(table, args)):
            assert ctypes_coarse(t) == a, f"{prefix}_{name}: argument {i} is {t.__name__}, the header says {a}"
        assert ctypes_coarse(mod._RESTYPES.get(name, C.c_int)) == ret, f"{prefix}_{name}: return type, the header says {ret}"
    assert getattr(mod, FAMILIES[prefix][2]) == version


def test_the_parser_tells_the_types_apart():
    """The check above is only as good as its two classifiers: each coarse type from both sides, and a wrong width caught."""
    assert [c_coarse(d) for d in ("const float *x", "int32_t n", "uint32_t c", "int64_t n", "uint64_t m", "float v",
                                  "double h", "const char *", "void *stream", "int", "const int32_t ids[4]")] == \
        ["ptr", "i32", "u32", "i64", "u64", "f32", "f64", "ptr", "ptr", "i32", "ptr"]
    assert [ctypes_coarse(t) for t in (C.c_void_p, C.c_char_p, C.POINTER(C.c_int32), C.c_int, C.c_int32, C.c_uint32, C.c_int64,
                                       C.c_uint64, C.c_float, C.c_double)] == \
        ["ptr", "ptr", "ptr", "i32", "i32", "u32", "i64", "u64", "f32", "f64"]
    protos, version = prototypes("pw")
    assert version == 1
    assert protos["voxel_keys"] == ("i32", ["ptr", "i32", "i64", "ptr", "f32", "ptr", "ptr", "ptr"])
    assert protos["last_error"] == ("ptr", [])
    assert prototypes("pv")[0]["render"][1][13] == "u32" and prototypes("pv")[0]["brick_words"][0] == "i64"
    assert prototypes("ph")[0]["panop_write"][1][8:10] == ["f64", "u64"]


@pytest.mark.parametrize("prefix", SIDE)
def test_side_binding_rejects_other_abi_versions(prefix, monkeypatch):
    """As tests/test_abi.py test_binding_rejects_other_abi_versions does for ph_*: a library built from another version of
    the family's header is refused with a 'rebuild' message."""
    from pasco_amd.build import build_hip
    _, module, const, cls, _ = FAMILIES[prefix]
    mod = importlib.import_module(module)
    path = build_hip(verbose=False)
    getattr(mod, cls)(path)                                  # the version it was written against binds
    monkeypatch.setattr(mod, const, getattr(mod, const) + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        getattr(mod, cls)(path)


def _refused_call(prefix, L):
    """One call per family that its entry point refuses on a scalar argument before it touches the HIP runtime (the checks
    at the top of each function; no pointer is read) -> (return code, the function's name)."""
    if prefix == "pe":
        from pasco_amd.eval.lib import MAX_SITES
        return L.lib.pe_ssc(None, None, None, MAX_SITES + 1, 1, None, None, 0, None, None, None), b"pe_ssc"
    if prefix == "pf":
        return L.lib.pf_transform_coords(None, 0, 1, None, None, 0, None, None), b"pf_transform_coords"      # M = 0
    if prefix == "pl":
        return L.lib.pl_semantic_grid(None, None, None, 1, -8, None, None, None), b"pl_semantic_grid"        # S = -8
    if prefix == "pv":
        return L.lib.pv_majority_pool(None, 0, 4, 4, 2, None, None, None), b"pv_majority_pool"               # X = 0
    return L.lib.pw_voxel_keys(None, 3, -1, None, 1.0, None, None, None), b"pw_voxel_keys"                   # n = -1


def test_error_text_stays_with_its_family():
    """Every family's translation unit has its own error buffer: a refusal shows in that family's last_error() and leaves the
    other four as they were."""
    from pasco_amd.build import build_hip
    build_hip(verbose=False)
    libs = {}
    for p in SIDE:
        mod = importlib.import_module(FAMILIES[p][1])
        libs[p] = getattr(mod, FAMILIES[p][4])()
        assert libs[p] is getattr(mod, FAMILIES[p][4])() and isinstance(libs[p], getattr(mod, FAMILIES[p][3]))

    def texts():
        return {p: getattr(libs[p].lib, p + "_last_error")() for p in SIDE}

    for p in SIDE:
        before = texts()
        rc, name = _refused_call(p, libs[p])
        after = texts()
        assert rc != 0 and name in after[p], (p, rc, after[p])
        if p == "pe":
            assert b"at most" in after[p]
        for q in SIDE:
            if q != p:
                assert after[q] == before[q] and name not in after[q], (p, q, after[q])
        with pytest.raises(RuntimeError, match=name.decode()):
            libs[p]._ok(rc, name.decode()[3:])
    assert len(set(texts().values())) == len(SIDE)
