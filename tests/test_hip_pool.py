"""The pp_* kernels (include/pasco_pool.h) and the pooling / broadcast / channel-wise modules of pasco_amd.me on the MI355X: the
kernels against the formulas in fp64 at a-priori bounds, copies and selections bit for bit, the modules against torch's dense
operators, the autograd routes, and the family's contracts (the same bits from two runs and on a side stream, refusals with a
message).  The cases, the shared checks and the references are tests/pool_cases.py and tests/pool_ref64.py; the CPU side is
tests/test_pool_cpu.py."""
import pytest
import torch

from tests import pool_cases as pc
from tests import stream_cases as sc
from tests.pool_ref64 import POOL_STACK_M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.poollib import pool_lib
    return pool_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


@pytest.mark.parametrize("c", pc.SEG_CHANNELS)
@pytest.mark.parametrize("kind", pc.BATCH_KINDS)
def test_seg_reduce_channels_and_batches(kind, c, lib, dev):
    pc.check_seg(lib, dev, 2 * pc.R + 3, c, kind)


@pytest.mark.parametrize("n", pc.ROWS)
def test_seg_reduce_rows(n, lib, dev):
    for c, kind in ((33, "gap"), (256, "shuffled8")):
        pc.check_seg(lib, dev, n, c, kind)


def test_seg_reduce_misaligned_slice_and_max_edges(lib, dev):
    pc.check_seg(lib, dev, pc.R, 33, "gap", misalign=True)
    pc.check_seg(lib, dev, pc.R, 256, "gap", misalign=True)          # a multiple of four at a base 4 bytes past a boundary: scalar
    pc.check_seg_slice(lib, dev)
    pc.check_seg_max_edges(lib, dev)


def test_more_batch_indices_than_served_are_refused(lib, dev):
    n, c, B = 10, 4, pc.MAX_BATCH + 1
    x, coords = pc.values((n, c), 1, dev), pc.batch_coords("one", n, dev)[0]
    g = pc.values((B, c), 2, dev)
    with pytest.raises(ValueError, match="PP_MAX_BATCH"):
        lib.seg_reduce(x, coords, B, pc.SUM)
    with pytest.raises(ValueError, match="PP_MAX_BATCH"):
        lib.broadcast(x, g, coords, pc.ADD)
    with pytest.raises(ValueError, match="PP_MAX_BATCH"):
        lib.broadcast_mul_bwd(x, x, g, coords)
    with pytest.raises(TypeError, match="fp32"):
        lib.seg_reduce(x.double(), coords, 1, pc.SUM)
    with pytest.raises(RuntimeError, match=r"pool: K = 65 outside \[1, 64\]"):
        lib.pool(x, torch.full((65, 3), -1, dtype=torch.int32, device=dev), pc.SUM)


@pytest.mark.parametrize("c", pc.CHANNELS)
def test_broadcast(c, lib, dev):
    for n, kind in ((2 * pc.R + 3, "gap"), (pc.R, "shuffled8"), (1, "one"), (0, "max")):
        pc.check_broadcast(lib, dev, n, c, kind, cg=c + 1 if c % 2 else c)
    pc.check_broadcast(lib, dev, pc.R + 1, 33 if c % 2 else 32, "gap", misalign=True)
    if c == 256:
        pc.check_broadcast(lib, dev, pc.R + 1, 260, "max")
        pc.check_broadcast_batch_outside(lib, dev)


@pytest.mark.parametrize("c", pc.CHANNELS)
@pytest.mark.parametrize("kind", ["down", "same"])
def test_pool_and_chconv_channels(kind, c, lib, dev):
    pc.check_pool(lib, dev, kind, c)
    pc.check_chconv(lib, dev, kind, c, bias=c != 32)


@pytest.mark.parametrize("variant", pc.TABLE_VARIANTS[1:])
@pytest.mark.parametrize("kind", ["down", "same"])
def test_pool_and_chconv_tables(kind, variant, lib, dev):
    for c, mis in ((33, True), (32, False), (32, True)):
        pc.check_pool(lib, dev, kind, c, variant, misalign=mis)
        pc.check_chconv(lib, dev, kind, c, variant, misalign=mis)


@pytest.mark.parametrize("rows", pc.ROWS)
def test_chconv_wgrad_rows(rows, lib, dev):
    for c in (33, 256, 260):
        pc.check_chconv_wgrad_rows(lib, dev, rows, c)


def test_modules_against_the_dense_torch_operators(lib, dev):
    pc.check_dense_twins(dev, torch.float32)


@pytest.mark.parametrize("name", pc.MODULE_NAMES)
def test_module_modes(name, lib, dev):
    pc.check_module_modes(dev, name)


def test_module_gradients_against_the_host_restatement(lib, dev):
    """Every module's device gradients against the same module on the CPU in fp64 (pasco_amd/grad/host.py through the oracle's
    maps): 1e-4 of the largest entry covers the fp32 sums of a few hundred rows of O(1e4) values."""
    from tests.conftest import load_oracle
    from pasco_amd.me import backend
    backend.register_checker_backend(load_oracle())
    try:
        cpu = torch.device("cpu")
        for name in pc.MODULE_NAMES:
            grads = []
            for device, dtype in ((dev, torch.float32), (cpu, torch.float64)):
                _, build, run = next(t for t in pc.module_cases(device, 4) if t[0] == name)
                torch.manual_seed(6)
                mod = build().to(device=device, dtype=dtype)
                f = pc.values((pc.pool_map("same", device)["n_in"], 4), 33, device, dtype).requires_grad_(True)
                out = run(mod, f)
                out.backward(pc.values(tuple(out.shape), 34, device, dtype))
                grads.append([f.grad.double().cpu()] + [p.grad.double().cpu() for p in mod.parameters()])
            for g, w in zip(*grads):
                assert g.shape == w.shape and float((g - w).abs().max()) <= 1e-4 * float(w.abs().max()), name
    finally:
        backend.register_checker_backend(None)


def test_pending_prologue_state_dict_and_refusals(lib, dev):
    pc.check_prologue(dev)
    pc.check_state_dict()
    pc.check_refusals(dev)


def test_pool_stack_gradients_against_the_fp64_twin(lib, dev):
    ratios = pc.pool_stack_ratios(dev)
    print({k: round(v, 3) for k, v in ratios.items()})
    assert len(ratios) == 9 and "dw.kernel" in ratios and "x" in ratios
    for name, r in ratios.items():
        assert r <= POOL_STACK_M, f"{name}: max |g - g64| = {r:.2f} x max |g32 - g64|, bound {POOL_STACK_M}"


# ---- the stream contract -------------------------------------------------------------------------------------------------------
def _seg_make(mode):
    def make(seed, device):
        n, c = 2 * pc.R + 3, 260
        x = torch.randn(n, c, generator=sc._gen(seed)).to(device)
        coords, B = pc.batch_coords("shuffled8", n, device)
        return {"x": x, "coords": coords, "B": B, "mode": mode}
    return make


def _seg_run(d):
    from pasco_amd.grad.poollib import pool_lib
    out, cnt, arg = pool_lib().seg_reduce(d["x"], d["coords"], d["B"], d["mode"])
    if arg is None:
        return out, cnt
    return out, cnt, arg, pool_lib().seg_max_bwd(d["x"][:d["B"]].contiguous(), arg, d["x"].shape[0])


def _bc_make(seed, device):
    n, c = pc.R + 1, 32
    g = sc._gen(seed)
    coords, B = pc.batch_coords("gap", n, device)
    return {"x": torch.randn(n, c, generator=g).to(device), "g": torch.randn(B, c, generator=g).to(device),
            "dy": torch.randn(n, c, generator=g).to(device), "coords": coords}


def _bc_run(d):
    from pasco_amd.grad.poollib import pool_lib
    L = pool_lib()
    outs = [L.broadcast(None if m == pc.COPY else d["x"], d["g"], d["coords"], m) for m in (pc.ADD, pc.MUL, pc.CAT, pc.COPY)]
    return tuple(outs) + L.broadcast_mul_bwd(d["dy"], d["x"], d["g"], d["coords"])


def _win_make(seed, device):
    m = pc.pool_map("same", device)
    g = sc._gen(seed)
    c = 33
    from pasco_amd.grad import nbr_invert
    return {"x": torch.randn(m["n_in"], c, generator=g).to(device), "dy": torch.randn(m["n_out"], c, generator=g).to(device),
            "w": torch.randn(27, c, generator=g).to(device), "bias": torch.randn(c, generator=g).to(device), "nbr": m["nbr"],
            "inv": nbr_invert(m["nbr"], m["n_in"]), "n_in": m["n_in"]}


def _win_run(d):
    from pasco_amd.grad.poollib import pool_lib
    L = pool_lib()
    out, cnt = L.pool(d["x"], d["nbr"], pc.AVG)
    return (out, cnt, L.pool(d["x"], d["nbr"], pc.SUM)[0], L.pool_bwd(d["dy"], cnt, d["inv"], d["n_in"], pc.AVG),
            L.pool_bwd(d["dy"], None, d["inv"], d["n_in"], pc.SUM), L.chconv_fwd(d["x"], d["nbr"], d["w"], d["bias"]),
            L.chconv_wgrad(d["x"], d["dy"], d["nbr"]))


STREAM_ENTRIES = [
    sc.Entry("pp.seg_reduce/sum", "pp", ("seg_reduce",), _seg_make(pc.SUM), _seg_run),
    sc.Entry("pp.seg_reduce/avg", "pp", ("seg_reduce",), _seg_make(pc.AVG), _seg_run),
    sc.Entry("pp.seg_reduce/max", "pp", ("seg_reduce", "seg_max_bwd"), _seg_make(pc.MAX), _seg_run),
    sc.Entry("pp.broadcast", "pp", ("broadcast", "broadcast_mul_bwd"), _bc_make, _bc_run),
    sc.Entry("pp.windows", "pp", ("pool", "pool_bwd", "chconv_fwd", "chconv_wgrad"), _win_make, _win_run),
]


def test_stream_table_covers_every_launching_entry():
    from pasco_amd.grad import poollib
    launching = set(poollib._SIGNATURES) - {"abi_version", "last_error", "seg_workspace_bytes", "chconv_wgrad_workspace_bytes"}
    assert {n for e in STREAM_ENTRIES for n in e.covers} == launching


@pytest.fixture(scope="module")
def side(dev):
    producer = sc.Producer(dev)
    return producer, sc.SideStreams(dev, producer, want=1)


@pytest.mark.parametrize("entry", STREAM_ENTRIES, ids=[e.name for e in STREAM_ENTRIES])
def test_same_bits_on_a_side_stream_behind_a_pending_producer(entry, lib, dev, side):
    """tests/stream_cases.order_check: the call on a side stream that the null stream demonstrably overtakes, behind pending
    work, with nothing enqueued on the null stream, gives the bits of the null-stream run."""
    producer, streams = side
    report = sc.order_check(entry, dev, producer, stream=streams.one())
    assert not report.failures, report.failures
