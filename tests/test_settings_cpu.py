"""`pasco_amd.settings`: the one table of the Python layer's switches - what the environment means for each field, how the
process-wide instance is changed and restored, that nothing else in the package reads the environment, and that
INTEGRATION.md lists the same names."""
import ast
import dataclasses
import os
import re
import subprocess
import sys
import threading

import pytest

from pasco_amd import settings
from pasco_amd.settings import Settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (field, environment name, default): the issue's table, restated
ON_UNLESS_0 = ["query_graph", "mask_block", "pe_table", "head_absorb", "attn_feat", "attn_split", "keep_fused", "resize_absorb",
               "input_fused", "optimistic", "panoptic_kernel", "conv_rl", "bench_pin", "me_defer"]
TABLE = [(f, "PASCO_" + f.upper(), True) for f in ON_UNLESS_0] + [
    ("conv_win_wide", "PASCO_CONV_WIN", False),
    ("c4_exchange", "PASCO_C4_EXCHANGE", "slab"),
    ("me_conv", "PASCO_ME_CONV", "guarded"),
    ("me_norm", "PASCO_ME_NORM", "torch"),
    ("conv_precision", None, "f16x3"),
    ("presplit", None, True),
    ("fusion", None, True)]


def test_table_and_defaults():
    assert [f.name for f in dataclasses.fields(Settings)] == [f for f, _, _ in TABLE]
    for s in (Settings(), Settings.from_env({})):
        for field, _, default in TABLE:
            assert getattr(s, field) == default and type(getattr(s, field)) is type(default), field
    assert Settings.from_env({}) == Settings()


@pytest.mark.parametrize("field", ON_UNLESS_0)
def test_boolean_is_on_unless_exactly_0(field):
    name = "PASCO_" + field.upper()
    off = Settings.from_env({name: "0"})
    assert getattr(off, field) is False and off == dataclasses.replace(Settings(), **{field: False})     # and nothing else moved
    assert getattr(Settings.from_env({name: "1"}), field) is True
    assert getattr(Settings.from_env({name: ""}), field) is True


def test_conv_win_wide_is_on_only_for_2():
    assert Settings.from_env({"PASCO_CONV_WIN": "2"}).conv_win_wide is True
    assert Settings.from_env({"PASCO_CONV_WIN": "0"}).conv_win_wide is False
    assert Settings.from_env({"PASCO_CONV_WIN": "1"}).conv_win_wide is False


def test_string_fields():
    s = Settings.from_env({"PASCO_C4_EXCHANGE": "f16", "PASCO_ME_CONV": "exact", "PASCO_ME_NORM": "device"})
    assert (s.c4_exchange, s.me_conv, s.me_norm) == ("f16", "exact", "device")
    assert Settings.from_env({"PASCO_C4_EXCHANGE": "allgather"}).c4_exchange == "allgather"
    with pytest.raises(AssertionError, match=re.escape("PASCO_ME_NORM='x': 'torch' or 'device'")):
        Settings.from_env({"PASCO_ME_NORM": "x"})
    with pytest.raises(AssertionError, match=re.escape("PASCO_ME_CONV='x': 'guarded' or 'exact'")):
        Settings.from_env({"PASCO_ME_CONV": "x"})


def test_frozen_and_unknown_fields():
    before = settings.current()
    with pytest.raises(dataclasses.FrozenInstanceError):
        before.attn_feat = False
    with pytest.raises(TypeError):
        settings.replace(no_such_field=1)
    with pytest.raises(TypeError):
        with settings.override(no_such_field=1):
            pass
    for bad in (dict(me_conv="x"), dict(me_norm="x"), dict(conv_precision="f16")):
        with pytest.raises(AssertionError):
            settings.replace(**bad)
    assert settings.current() is before


def test_override_restores_after_an_exception_and_unwinds_in_order():
    before = settings.current()
    with pytest.raises(RuntimeError):
        with settings.override(attn_feat=False):
            assert settings.current().attn_feat is False
            raise RuntimeError("inside")
    assert settings.current() is before
    with settings.override(attn_feat=False) as outer:
        assert outer is settings.current()
        with settings.override(pe_table=False) as inner:
            assert (inner.attn_feat, inner.pe_table) == (False, False) and settings.current() is inner
        assert settings.current() is outer and outer.pe_table is True
    assert settings.current() is before


def test_setters_land_in_the_object():
    from pasco_amd.graph import fused
    from pasco_amd.me import modules
    before = settings.current()
    try:
        fused.set_conv_precision("f16x3-inline")
        assert (settings.current().conv_precision, settings.current().presplit) == ("f16x3", False)
        fused.set_conv_precision("f32")
        assert (settings.current().conv_precision, settings.current().presplit) == ("f32", True)
        assert fused.conv_precision() == "f32"
        fused.set_conv_precision("f16x3")
        assert (settings.current().conv_precision, settings.current().presplit) == ("f16x3", True)
        with pytest.raises(AssertionError):
            fused.set_conv_precision("f16")
        fused.set_fusion(False)
        assert fused.fusion() is False and settings.current().fusion is False
        fused.set_fusion(True)
        modules.set_me_conv("exact")
        modules.set_me_norm("device")
        assert (settings.current().me_conv, settings.current().me_norm) == ("exact", "device")
        for setter in (modules.set_me_conv, modules.set_me_norm):
            with pytest.raises(AssertionError):
                setter("x")
    finally:
        settings.replace(**dataclasses.asdict(before))
    assert settings.current() == before


def test_precision_override_is_the_thread_s_own():
    from pasco_amd.graph import fused
    seen = []
    with fused.precision_override("f32"):
        assert fused.conv_precision() == "f32" and settings.current().conv_precision == "f16x3"
        t = threading.Thread(target=lambda: seen.append(fused.conv_precision()))
        t.start()
        t.join()
    assert seen == ["f16x3"] and fused.conv_precision() == "f16x3"


def test_environment_is_read_at_import_in_a_fresh_process():
    env = dict(os.environ, PASCO_ATTN_FEAT="0", PASCO_CONV_WIN="2", PASCO_ME_NORM="device", PYTHONPATH=ROOT)
    code = "from pasco_amd import settings as s; c = s.current(); print(c.attn_feat, c.conv_win_wide, c.me_norm)"
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    assert out.split() == ["False", "True", "device"]


def _package_files():
    for base, _, names in os.walk(os.path.join(ROOT, "pasco_amd")):
        for n in names:
            if n.endswith(".py"):
                yield os.path.join(base, n)


def test_only_settings_reads_the_environment():
    readers, named = set(), set()
    for path in _package_files():
        rel = os.path.relpath(path, ROOT)
        source = open(path).read()
        if not any(word in source for word in ("environ", "getenv", "PASCO_")):      # nothing for the walk to find
            continue
        tree = ast.parse(source)
        docstrings = set()
        for node in ast.walk(tree):
            if isinstance(node, (ast.Module, ast.ClassDef, ast.FunctionDef, ast.AsyncFunctionDef)) and node.body and \
                    isinstance(node.body[0], ast.Expr) and isinstance(node.body[0].value, ast.Constant):
                docstrings.add(id(node.body[0].value))
        for node in ast.walk(tree):
            if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name) and node.value.id == "os" and \
                    node.attr in ("environ", "getenv"):
                readers.add(rel)
            if isinstance(node, ast.ImportFrom) and node.module == "os" and any(a.name in ("environ", "getenv") for a in node.names):
                readers.add(rel)
            if isinstance(node, ast.Constant) and isinstance(node.value, str) and node.value.startswith("PASCO_") and \
                    id(node) not in docstrings:
                named.add(rel)
    assert readers == {os.path.join("pasco_amd", "settings.py"), os.path.join("pasco_amd", "build.py")}
    assert named <= {os.path.join("pasco_amd", "settings.py")}


# paragraphs of INTEGRATION.md that speak of other PASCO_* names, by a phrase of theirs: the development build's dispatch
# switches and the names bench.py reads for itself
KNOWN_EXCEPTIONS = ("development build", "`bench.py` reads for itself")


def test_integration_md_lists_the_table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    names = {env for _, env, _ in TABLE if env}
    for env in names:
        assert env in text, env
    for para in re.split(r"\n\s*\n|\n(?=[*-] )", text):
        if any(k in para for k in KNOWN_EXCEPTIONS):
            continue
        for env in re.findall(r"PASCO_[A-Z0-9_]+", para):
            assert env in names, (env, para[:80])
