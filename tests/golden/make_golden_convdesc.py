"""Generate tests/golden/conv_desc.json: the `ph_conv_desc` that `CBackend.conv_fwd` hands to `ph_conv_fwd` for a table of calls
which between them use every keyword and every branch that writes a field - the pin tests/test_conv_desc_cpu.py holds the
binding to.  The fixture in the repository was recorded from pasco_amd/me/backend.py as it stood BEFORE conv_fwd was cut into
named steps; regenerate it only from a binding whose descriptors are known to be right.

Runs on the CPU with the oracle as the backend (`checker_split` lets the mode-2 descriptors through); never collected by pytest.
The library's `conv_fwd` is swapped for a capture that copies the descriptor and returns 0, so nothing is computed and the
shapes of the two calls above the split-K boundary cost nothing (they take the operand-only route: no rows exist).  Every call
gets a backend of its own, so the bytes of split-K scratch are what the sizing rule asks for, not what an earlier call left.
The `win_wfrag` call needs a backend that serves the device: it is recorded (and replayed) with `_serves_cuda` patched true.

Per call: every non-pointer field; for every pointer field "null", the argument whose storage it points to ("x", "bias",
"split[0]", "win[rows]", ...) or "set" for a buffer the binding made itself; whether the library was called at all, whether
the call returned a tuple, and for every split operand the call made itself whether it was still alive at the launch.  Data only - settings and recorded results.

    python tests/golden/make_golden_convdesc.py [--out tests/golden/conv_desc.json]
"""
import ctypes as C
import json
import os
import sys
import weakref

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_IN, N_OUT = 24, 20
BIG = 1 << 17            # rows: BIG * 64 channels = 1 << 23, the boundary of the split-K sizing rule


def fresh_backend():
    from tests.conftest import load_oracle
    be = load_oracle()
    be.checker_split = True
    return be


def _f(*shape):
    n = 1
    for s in shape:
        n *= s
    return (((torch.arange(n) % 7) - 3).float() / 4).reshape(shape).contiguous()        # |values| <= 0.75, exact


def _i(*shape):
    return torch.zeros(shape, dtype=torch.int32)


def cases(be):
    """-> list of (name, positional arguments, keywords, {"route": bits} | {"serves_cuda": True} | {})."""
    from pasco_amd.me import backend as B
    x8, w3, nbr3 = _f(N_IN, 8), _f(3, 8, 16), _i(3, N_OUT)
    w32 = _f(3, 8, 32)
    word = _i(1)
    m1, m2, m2_32 = be.split_weight_f16(w3), be.split_weight_rows(w3), be.split_weight_rows(w32)
    xs = be.split_rows(x8)
    out = [
        ("exact_plain", (x8, w3, nbr3, N_OUT), {}, {}),
        ("exact_k1_weight_2d", (x8, _f(8, 16), None, N_IN), {}, {}),
        ("exact_if", (x8, w3, nbr3, N_OUT), dict(exact_if=word), {}),
        ("exact_status", (x8, w3, nbr3, N_OUT), dict(status=word), {}),
        ("exact_acts", (x8, w3, nbr3, N_OUT), dict(pro_act=B.ACT_RELU, epi_act=B.ACT_LEAKY, slope=0.25, res_act=B.ACT_RELU), {}),
        ("exact_caller_out", (x8, w3, nbr3, N_OUT), dict(out=_f(N_OUT, 16)), {}),
        ("exact_empty", (x8, w3, _i(3, 0), 0), {}, {}),
        ("routed", (x8, w3, nbr3, N_OUT), {}, {"route": B.ROUTE_WIN_NEVER | B.ROUTE_LIN_NEVER}),
        ("residual", (x8, w3, nbr3, N_OUT), dict(residual=_f(N_OUT, 16), res_act=B.ACT_LEAKY), {}),
        ("axis_exact", (x8, w3, nbr3, N_OUT), dict(axis=(_f(3, 5, 16), _i(N_OUT, 4), -2)), {}),
    ]
    for name, c in (("pro_scale", 8), ("pro_shift", 8), ("bias", 16), ("epi_scale", 16), ("epi_shift", 16), ("epi2_scale", 16),
                    ("epi2_shift", 16)):
        out.append(("affine_" + name, (x8, w3, nbr3, N_OUT), {name: _f(c)}, {}))
    out += [
        ("mode1", (x8, w3, nbr3, N_OUT), dict(split=m1), {}),
        ("mode1_status", (x8, w3, nbr3, N_OUT), dict(split=m1, status=word), {}),
        ("mode2_given", (x8, w3, nbr3, N_OUT), dict(split=m2, in_split=xs), {}),
        ("mode2_status", (x8, w3, nbr3, N_OUT), dict(split=m2, in_split=xs, status=word), {}),
        ("mode2_derived", (x8, w3, nbr3, N_OUT), dict(split=m2, pro_scale=_f(8), pro_shift=_f(8), pro_act=B.ACT_RELU), {}),
        ("mode2_given_with_prologue", (x8, w3, nbr3, N_OUT),
         dict(split=m2, in_split=xs, pro_scale=_f(8), in_split_has_prologue=True), {}),
        ("mode2_x_none", (None, w3, nbr3, N_OUT), dict(split=m2, in_split=xs, xshape=(N_IN, 8)), {}),
        ("mode2_weight_none", (x8, None, nbr3, N_OUT), dict(split=m2, in_split=xs, wshape=(3, 8, 16)), {}),
        ("mode2_axis", (x8, w3, nbr3, N_OUT), dict(split=m2, in_split=xs, axis=(_f(3, 7, 16), _i(N_OUT, 4), 3), residual=_f(N_OUT, 16)), {}),
        ("emit", (x8, w32, nbr3, N_OUT), dict(split=m2_32, in_split=xs, emit_split=(_f(32), _f(32), B.ACT_RELU)), {}),
        ("emit_bare", (x8, w32, nbr3, N_OUT), dict(split=m2_32, in_split=xs, emit_split=(None, None, B.ACT_NONE)), {}),
        ("emit_no_out", (x8, w32, nbr3, N_OUT), dict(split=m2_32, in_split=xs, emit_split=(None, _f(32), B.ACT_LEAKY), want_out=False), {}),
        ("emit_caller_buffers", (x8, w32, nbr3, N_OUT),
         dict(split=m2_32, in_split=xs, emit_split=(None, None, B.ACT_NONE), out=_f(N_OUT, 32),
              out_split=torch.zeros((N_OUT, 1, 2, 32), dtype=torch.float16)), {}),
        ("emit_empty", (x8, w32, _i(3, 0), 0), dict(split=m2_32, in_split=xs, emit_split=(None, None, B.ACT_NONE)), {}),
    ]
    # 27-offset maps: the dense-grid promise, row lists, windows (n_in == n_out for the grid)
    x20, w27, w27_64, nbr27 = _f(N_OUT, 8), _f(27, 8, 16), _f(27, 8, 64), _i(27, N_OUT)
    win = {"rows": _i(1, 27 * 128), "cnt": _i(1), "slots": torch.zeros((1, 27, 128), dtype=torch.int16), "stats": _i(4), "n_out": N_OUT}
    rl = {"in": _i(256), "out": _i(256), "tile_k": _i(2)}
    out += [
        ("grid", (x20, w27, nbr27, N_OUT), dict(split=be.split_weight_rows(w27), grid=((1, 2, 5, 2), (3, 3, 3))), {}),
        ("grid_without_map", (x20, w27, None, N_OUT), dict(split=be.split_weight_rows(w27), grid=((1, 2, 5, 2), (3, 3, 3))), {}),
        ("rowlist", (x8, w3, nbr3, N_OUT), dict(split=m2, in_split=xs, rowlist=rl), {}),
        ("win", (x20, w27, nbr27, N_OUT), dict(split=be.split_weight_rows(w27), win=win), {}),
        ("win_kvol3_ignored", (x8, w3, nbr3, N_OUT), dict(split=m2, in_split=xs, win=win), {}),
        ("win_64_on_cpu", (x20, w27_64, nbr27, N_OUT), dict(split=be.split_weight_rows(w27_64), win=win), {}),
        ("win_wfrag", (x20, w27_64, nbr27, N_OUT), dict(split=be.split_weight_rows(w27_64), win=win), {"serves_cuda": True}),
    ]
    # the split-K sizing rule on both sides of n_out * cout = 1 << 23, one offset and several: operand-only calls, no rows exist
    tiny = torch.zeros(N_IN * 2 * 32, dtype=torch.float16)                     # in_split of N_IN rows of 8 (padded to 32) channels
    wk1, wk2 = torch.zeros(64 * 2 * 32, dtype=torch.float16), torch.zeros(2 * 64 * 2 * 32, dtype=torch.float16)
    for name, rows, k, wsp in (("splitk_at_boundary_k1", BIG, 1, wk1), ("splitk_above_k1", BIG + 1, 1, wk1),
                               ("splitk_above_k2", BIG + 1, 2, wk2)):
        nbr = None if k == 1 else torch.empty((k, rows), dtype=torch.int32)
        out.append((name, (None, None, nbr, rows), dict(split=(wsp, 1.0), in_split=tiny, xshape=(N_IN, 8), wshape=(k, 8, 64)), {}))
    return out


def _addresses(args, kw):
    """address -> name of the argument tensor that starts there (tuples and dicts by member)."""
    named = dict(zip(("x", "weight", "nbr"), args), **kw)
    flat = {}
    for k, v in named.items():
        members = {k: v}
        if isinstance(v, (tuple, list)):
            members = {f"{k}[{i}]": m for i, m in enumerate(v)}
        elif isinstance(v, dict):
            members = {f"{k}[{i}]": m for i, m in v.items()}
        flat.update({m.data_ptr(): n for n, m in members.items() if isinstance(m, torch.Tensor) and m.numel()})
    return flat


def describe(d, args, kw):
    from pasco_amd.me.backend import ConvDesc
    row, given = {}, _addresses(args, kw)
    for name, typ in ConvDesc._fields_:
        v = getattr(d, name)
        if typ is C.c_void_p:
            row[name] = "null" if not v else given.get(v, "set")
        elif isinstance(v, C.Array):
            row[name] = [int(q) for q in v]
        else:
            row[name] = v
    return row


def record():
    """-> one row per call of `cases`, each made on a backend of its own."""
    from pasco_amd.me.backend import ConvDesc
    rows = []
    for i in range(len(cases(fresh_backend()))):
        be = fresh_backend()
        name, args, kw, how = cases(be)[i]
        seen, made, alive = [], [], []
        inner = be.split_rows

        def split_rows(*a, **k):                  # an operand conv_fwd makes itself: only the descriptor points to it
            t = inner(*a, **k)
            made.append(weakref.ref(t))
            return t

        def capture(ref, stream):
            seen.append(ConvDesc.from_buffer_copy(ref._obj))
            alive.extend(r() is not None for r in made)
            return 0

        be.fn["conv_fwd"], be.split_rows = capture, split_rows
        be._serves_cuda = bool(how.get("serves_cuda", False))
        with be.routing(how.get("route", 0)):
            ret = be.conv_fwd(*args, **kw)
        assert len(seen) <= 1
        rows.append({"name": name, "launched": bool(seen), "tuple": isinstance(ret, tuple), "made_operands_alive_at_launch": alive,
                     "desc": describe(seen[0], args, kw) if seen else None})
    return rows


ABOUT = ("ph_conv_desc per call of tests/golden/make_golden_convdesc.py::cases, recorded on the CPU oracle from the binding as it "
         "stood before conv_fwd was cut into named steps; win_wfrag with _serves_cuda patched true")


def main():
    out_path = os.path.join(HERE, "conv_desc.json")
    if "--out" in sys.argv:
        out_path = sys.argv[sys.argv.index("--out") + 1]
    rows = record()
    with open(out_path, "w") as f:
        f.write('{"about": %s,\n "calls": [\n' % json.dumps(ABOUT))
        f.write(",\n".join("  " + json.dumps(r) for r in rows))
        f.write("\n ]}\n")
    print(f"[convdesc] wrote {len(rows)} calls to {out_path}")


if __name__ == "__main__":
    main()
