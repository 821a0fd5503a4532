"""`pasco_amd.grad.optim.AdamW` on CPU parameters: the torch restatement of include/pasco_optim.h (pasco_amd/grad/host.py) behind
the same optimiser class, records and order as the kernels.  The checks are tests/optim_cases.py, the references
tests/optim_ref64.py; the GPU side is tests/test_hip_optim.py."""
import pytest
import torch

from pasco_amd.grad.optim import warmup_cosine
from tests import optim_cases as oc

CPU = torch.device("cpu")


@pytest.mark.parametrize("max_norm", [oc.CLIP, oc.NO_CLIP], ids=["clip_acts", "clip_idle"])
def test_three_steps_against_the_fp64_twin(max_norm):
    oc.check_accuracy(CPU, max_norm)


def test_sum_of_squares_and_equal_bits_on_a_repeat():
    oc.check_norm(CPU)


@pytest.mark.parametrize("name", list(oc.LONG_CASES))
def test_more_chunks_than_the_grid_and_more_tensors_than_a_workgroup(name):
    oc.check_long(CPU, name)


def test_grad_scale():
    oc.check_grad_scale(CPU)


def test_first_gradient_at_the_third_step():
    oc.check_late_gradient(CPU)


def test_nonfinite_propagates_like_torch():
    oc.check_nonfinite_propagate(CPU)


def test_nonfinite_skipped():
    oc.check_nonfinite_skip(CPU)


def test_state_dict_round_trips_with_torch():
    oc.check_state_dict_round_trips(CPU)


def test_versions_move_with_the_step():
    oc.check_versions(CPU)


def test_refusals():
    oc.check_refusals(CPU)


def test_non_contiguous_gradient_and_a_late_group():
    oc.check_non_contiguous_gradient(CPU)


def test_lambda_lr_drives_it():
    oc.check_scheduler_drives_it(CPU)


def test_warmup_cosine_factor():
    """The factor the reference's schedule returns: linear below `warmup_end`, 1.0 from there, 0.1 past iteration 60 000;
    `max_iter` and `factor_min` change nothing."""
    f = warmup_cosine(1000, 50000, 0.01)
    assert f(0) == 0.0 and f(250) == 0.25 and f(999) == 0.999 and f(1000) == 1.0 and f(1001) == 1.0
    assert f(60000) == 1.0 and f(60001) == 0.1 and f(10 ** 6) == 0.1
    g = warmup_cosine(0, 50000, 0.01)                # the reference's own arguments: no warm-up
    assert g(0) == 1.0 and g(60000) == 1.0 and g(60001) == 0.1
    assert [warmup_cosine(1000, 7, 0.5)(i) for i in (0, 500, 1000, 60001)] == [f(i) for i in (0, 500, 1000, 60001)]
    late = warmup_cosine(70000, 50000, 0.01)         # past 60 000 the drop wins over a warm-up still running
    assert late(35000) == 0.5 and late(60001) == 0.1


def test_tables_cover_every_element_once():
    """The chunk table the device path uploads: per tensor the starts 0, PO_CHUNK, ... below its element count, in tensor
    order; nothing for an empty tensor; the tensor records field for field."""
    from pasco_amd.grad.optim import build_tables
    from pasco_amd.grad.optimlib import PO_CHUNK
    sizes = [0, 1, PO_CHUNK - 1, PO_CHUNK, PO_CHUNK + 1, 0, 3 * PO_CHUNK + 5, 2 ** 31 - 1]
    entries = [(10 + i, i % 2, 1000 + 16 * i, 2000 + 16 * i, n) for i, n in enumerate(sizes)]
    tab, chunks = build_tables(entries, [3000 + i for i in range(len(sizes))], [4000 + i for i in range(len(sizes))])
    assert tab["n"].tolist() == sizes and tab["state"].tolist() == [10 + i for i in range(len(sizes))]
    assert tab["group"].tolist() == [i % 2 for i in range(len(sizes))] and tab["p"].tolist() == [1000 + 16 * i for i in range(len(sizes))]
    assert tab["g"][3] == 2048 and tab["m"][3] == 3003 and tab["v"][3] == 4003 and tab.tobytes()[48 * 3 + 32:48 * 3 + 40] == \
        (PO_CHUNK).to_bytes(8, "little")
    want = [(i, s) for i, n in enumerate(sizes[:-1]) for s in range(0, n, PO_CHUNK)]
    k = len(want)
    assert list(zip(chunks["tensor"][:k].tolist(), chunks["start"][:k].tolist())) == want
    last = chunks[k:]
    assert len(last) == 2 ** 31 // PO_CHUNK and set(last["tensor"].tolist()) == {len(sizes) - 1}
    assert last["start"][0] == 0 and last["start"][-1] == 2 ** 31 - PO_CHUNK and (last["start"][1:] - last["start"][:-1] == PO_CHUNK).all()


def test_binding_table_mirrors_the_prototypes():
    """Every `PO_FN(name)(...)` of the header is bound under that name with as many arguments, pointers as pointers, and the
    records have the header's sizes (the kernels' source asserts the same sizes on its side)."""
    import ctypes as C
    import os
    import re
    from pasco_amd.grad import optimlib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pasco_optim.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {m.group(1): [a.strip() for a in m.group(2).split(",")] for m in re.finditer(r"PO_FN\((\w+)\)\s*\(([^()]*)\)\s*;", text)}
    assert set(protos) == set(optimlib._SIGNATURES) and len(protos) == 6
    for name, args in protos.items():
        args = [] if args == ["void"] else args
        table = optimlib._SIGNATURES[name]
        assert len(table) == len(args), name
        for t, a in zip(table, args):
            assert ("*" in a) == (t is C.c_void_p), (name, a)
            if a.startswith("po_groups"):
                assert t is optimlib.Groups
            elif "*" not in a:
                assert t is {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[a.split()[0]], (name, a)
    assert C.sizeof(optimlib.Groups) == optimlib.PO_MAX_GROUPS * 5 * 8
    sizes = dict(re.findall(r"\}\s*(po_\w+);\s*/\*\s*(\d+) bytes", open(os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "include", "pasco_optim.h")).read()))
    assert {k: int(v) for k, v in sizes.items()} == {
        "po_tensor": optimlib.TENSOR_DTYPE.itemsize, "po_chunk": optimlib.CHUNK_DTYPE.itemsize, "po_state": optimlib.STATE_DTYPE.itemsize,
        "po_result": optimlib.RESULT_DTYPE.itemsize, "po_step": optimlib.STEP_DTYPE.itemsize, "po_scalars": 4 * len(optimlib.SCALAR_FIELDS)}


def test_library_binds_and_refuses_without_a_device(monkeypatch):
    """The built library exports the po_* family at this binding's version; another version is refused with a 'rebuild'
    message; the limits of a table are refused with their text - nothing here touches a GPU."""
    from pasco_amd.build import build_hip
    from pasco_amd.grad import optimlib
    path = build_hip(verbose=False)
    lib = optimlib.OptimLib(path)
    assert lib.lib.po_abi_version() == optimlib.PO_ABI_VERSION
    lib.table_check(349, 16056320, 126495889, 1)
    for args, text in (((5, 2 ** 31, 2 ** 31, 1), "fewer than 2\\^31 per tensor"), ((5, 7, 2 ** 40, 1), "fewer than 2\\^40"),
                       ((2 ** 31, 0, 0, 1), "tensors"), ((1, 1, 1, optimlib.PO_MAX_GROUPS + 1), "PO_MAX_GROUPS")):
        with pytest.raises(RuntimeError, match="po_table_check: table_check: .*" + text):
            lib.table_check(*args)
    monkeypatch.setattr(optimlib, "PO_ABI_VERSION", optimlib.PO_ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="rebuild"):
        optimlib.OptimLib(path)


def test_binding_constants_mirror_the_header():
    import os
    import re
    from pasco_amd.grad import host, optimlib
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pasco_optim.h")).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert const("PO_ABI_VERSION") == optimlib.PO_ABI_VERSION
    assert const("PO_CHUNK") == optimlib.PO_CHUNK == host.OPTIM_CHUNK
    assert const("PO_MAX_GROUPS") == optimlib.PO_MAX_GROUPS
    assert (const("PO_POLICY_PROPAGATE"), const("PO_POLICY_SKIP")) == (optimlib.PO_POLICY_PROPAGATE, optimlib.PO_POLICY_SKIP)
    assert tuple(re.search(r"float ([\w, ]+);\s*\} po_scalars", text).group(1).split(", ")) == optimlib.SCALAR_FIELDS == \
        host.OPTIM_SCALARS
