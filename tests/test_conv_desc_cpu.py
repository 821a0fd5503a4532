"""What `CBackend.conv_fwd` hands to `ph_conv_fwd`, pinned: tests/golden/conv_desc.json holds the descriptor of every call of
tests/golden/make_golden_convdesc.py::cases as the binding filled it before `conv_fwd` was cut into named steps (every keyword,
every branch that writes a field, the split-K sizing rule on both sides of its boundary).  The replay is the recorder's own
`record()`: the oracle as the backend, the library's entry point swapped for a capture, `win_wfrag` with `_serves_cuda` patched.
The second test holds every refusal of `conv_fwd` to its type and text."""
import json
import os
import re

import pytest
import torch

from tests.golden import make_golden_convdesc as G

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(G.__file__)), "conv_desc.json")


def test_descriptors_equal_the_recorded_ones():
    with open(FIXTURE) as f:
        want = json.load(f)["calls"]
    got = json.loads(json.dumps(G.record()))
    assert [r["name"] for r in got] == [r["name"] for r in want]
    for g, w in zip(got, want):
        if g != w:
            fields = [k for k in w["desc"] or {} if (g["desc"] or {}).get(k) != w["desc"][k]]
            head = {k: (g[k], w[k]) for k in w if k != "desc" and g[k] != w[k]}
            raise AssertionError(f"{w['name']}: (got, recorded) {head}; fields that differ: " + ", ".join(f"{k} = {(g['desc'] or {}).get(k)!r} (recorded {w['desc'][k]!r})" for k in fields))
    assert sum(r["launched"] for r in want) >= 25


def _refusals(be):
    """(name, exception type, message as the binding words it, positional arguments, keywords[, device type to pose as])."""
    f, i = G._f, G._i
    x, w, nbr, n = f(G.N_IN, 8), f(3, 8, 16), i(3, G.N_OUT), G.N_OUT
    w32 = f(3, 8, 32)
    m1, m2, m2_32, xs = be.split_weight_f16(w), be.split_weight_rows(w), be.split_weight_rows(w32), be.split_rows(x)
    half = torch.zeros(4, dtype=torch.float16)
    return [
        ("x_none_bare", ValueError, "conv: x=None needs xshape, in_split and a mode-2 split on the device backend",
         (None, w, nbr, n), dict(split=m2, in_split=xs)),
        ("x_none_mode1", ValueError, "conv: x=None needs xshape, in_split and a mode-2 split on the device backend",
         (None, w, nbr, n), dict(split=m1, in_split=xs, xshape=(G.N_IN, 8))),
        ("x_none_prologue", ValueError, "conv: a pre-split input already carries its prologue",
         (None, w, nbr, n), dict(split=m2, in_split=xs, xshape=(G.N_IN, 8), pro_scale=f(8))),
        ("weight_none_bare", ValueError, "conv: weight=None needs wshape and a mode-2 split on the device backend",
         (x, None, nbr, n), dict(split=m2)),
        ("x_dtype", TypeError, "in: expected torch.float32, got torch.float64", (x.double(), w, nbr, n), {}),
        ("weight_strided", ValueError, "weight: tensor must be contiguous", (x, f(3, 16, 8).transpose(1, 2), nbr, n), {}),
        ("nbr_dtype", TypeError, "nbr: expected torch.int32, got torch.int64", (x, w, nbr.long(), n), {}),
        ("channels", ValueError, "conv: input has 16 channels, kernel expects 8", (f(G.N_IN, 16), w, nbr, n), {}),
        ("nbr_shape", ValueError, "conv: nbr shape (3, 20) != (3, 19)", (x, w, nbr, n - 1), {}),
        ("emit_exact", ValueError, "conv: emit_split needs a mode-2 split and cout % 32 == 0",
         (x, w32, nbr, n), dict(emit_split=(None, None, 0))),
        ("emit_cout16", ValueError, "conv: emit_split needs a mode-2 split and cout % 32 == 0",
         (x, w, nbr, n), dict(split=m2, in_split=xs, emit_split=(None, None, 0))),
        ("out_split_size", ValueError, "conv: out_split must be contiguous f16 [n_out, cout / 32, 2, 32]",
         (x, w32, nbr, n), dict(split=m2_32, in_split=xs, emit_split=(None, None, 0), out_split=half)),
        ("osp_scale_size", ValueError, "conv: osp_scale has 16 entries, expected 32",
         (x, w32, nbr, n), dict(split=m2_32, in_split=xs, emit_split=(f(16), None, 0))),
        ("osp_shift_size", ValueError, "conv: osp_shift has 8 entries, expected 32",
         (x, w32, nbr, n), dict(split=m2_32, in_split=xs, emit_split=(None, f(8), 0))),
        ("pro_scale_size", ValueError, "conv: pro_scale has 16 entries, expected 8", (x, w, nbr, n), dict(pro_scale=f(16))),
        ("bias_size", ValueError, "conv: bias has 8 entries, expected 16", (x, w, nbr, n), dict(bias=f(8))),
        ("epi2_shift_dtype", TypeError, "epi2_shift: expected torch.float32, got torch.float16", (x, w, nbr, n), dict(epi2_shift=f(16).half())),
        ("residual_shape", ValueError, "conv: residual shape mismatch", (x, w, nbr, n), dict(residual=f(n, 8))),
        ("axis_shape", ValueError, "conv: axis = (table [3, T, cout], coords [n_out, 4], lo)",
         (x, w, nbr, n), dict(axis=(f(3, 5, 8), i(n, 4), 0))),
        ("axis_exact_on_device", ValueError, "conv: the axis-table residual is served by the pre-split (mode 2) path",
         (x, w, nbr, n), dict(axis=(f(3, 5, 16), i(n, 4), 0)), "cuda"),
        ("in_split_with_prologue", ValueError,
         "conv: in_split given together with a prologue - pass in_split_has_prologue=True if the operand was built with "
         "split_rows(x, pro_scale=..., pro_shift=..., pro_act=...), else drop in_split",
         (x, w, nbr, n), dict(split=m2, in_split=xs, pro_act=1)),
        ("in_split_size", ValueError, "conv: in_split does not match the input rows", (x, w, nbr, n), dict(split=m2, in_split=half)),
        ("w_split_size", ValueError, "conv: w_split does not match the kernel", (x, w, nbr, n), dict(split=(half, 1.0), in_split=xs)),
        ("grid_volume", ValueError, "conv: grid = ((B, X, Y, Z), (kx, ky, kz)) must describe the whole map (odd kernel sizes)",
         (x, w, nbr, n), dict(split=m2, in_split=xs, grid=((1, 2, 5, 2), (3, 1, 1)))),
        ("grid_even_kernel", ValueError, "conv: grid = ((B, X, Y, Z), (kx, ky, kz)) must describe the whole map (odd kernel sizes)",
         (f(n, 8), f(2, 8, 16), i(2, n), n), dict(split=be.split_weight_rows(f(2, 8, 16)), grid=((1, 2, 5, 2), (2, 1, 1)))),
        ("exact_if_split", ValueError, "conv: exact_if guards an exact fp32 launch (no split)",
         (x, w, nbr, n), dict(split=m1, exact_if=i(1))),
    ]


def test_every_refusal_keeps_its_type_and_text():
    be = G.fresh_backend()
    launched = []
    be.fn["conv_fwd"] = lambda ref, stream: launched.append(1) or 0
    table = _refusals(be)
    assert len(table) >= 15
    for name, exc, text, args, kw, *pose in table:
        be.device_type = pose[0] if pose else "cpu"
        try:
            with pytest.raises(exc, match="^" + re.escape(text) + "$"):
                be.conv_fwd(*args, **kw)
        except BaseException as e:
            raise AssertionError(f"{name}: {e}") from e
        finally:
            be.device_type = "cpu"
    assert not launched, "a refused call reached the library"
