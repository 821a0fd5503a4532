"""The pq_* kernels (include/pasco_field.h) and `TensorField`, the quantisation modes, `slice` and `MinkowskiInterpolation` of
pasco_amd.me on the MI355X: the grouping exactly, the sums against fp64 at a-priori bounds, selections and tables bit for bit,
the modules against the CPU route in fp64 and against a dense fp64 twin of a small network, and the family's contracts (the same
bits from two runs and on a side stream, refusals with a message).  The cases, the shared checks and the references are
tests/field_cases.py and tests/field_ref64.py; the CPU side is tests/test_field_cpu.py."""
import pytest
import torch

from tests import field_cases as fc
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu
U = fc.U


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.fieldlib import field_lib
    return field_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


@pytest.fixture()
def cpu_route():
    """CPU tensors served by the checker backend for the duration of one test (the fp64 side of the module checks)."""
    from tests.conftest import load_oracle
    from pasco_amd.me import backend
    backend.register_checker_backend(load_oracle())
    yield torch.device("cpu")
    backend.register_checker_backend(None)


@pytest.mark.parametrize("pattern", fc.GROUP_PATTERNS)
def test_group_exact(pattern, lib, dev):
    for n in fc.GROUP_N:
        fc.check_group(lib, dev, pattern, n)


@pytest.mark.parametrize("c", fc.SEG_CHANNELS)
def test_segment_sums_and_averages(c, lib, dev):
    fc.check_seg_sums(lib, dev, c)


def test_segment_sums_at_a_misaligned_base(lib, dev):
    fc.check_seg_sums(lib, dev, 33, misalign=True)
    fc.check_seg_sums(lib, dev, 256, misalign=True)          # a multiple of four 4 bytes past a boundary: scalar


def test_segment_max_with_arg_bit_for_bit(lib, dev):
    fc.check_seg_max(lib, dev)
    fc.check_seg_max(lib, dev, c=33)


@pytest.mark.parametrize("c", fc.SEG_CHANNELS)
def test_gather_w_bit_for_bit(c, lib, dev):
    fc.check_gather_w(lib, dev, c)
    if c in (33, 256):
        fc.check_gather_w(lib, dev, c, misalign=True)


@pytest.mark.parametrize("ts,batch,one", [(1, 0, False), (2, 3, False), (4, 0, False), (3, 0, False), (1, 3, True), (2, 0, True)])
def test_interpolation_map(ts, batch, one, lib, dev):
    fc.check_interp_map(lib, dev, ts, batch, one)


@pytest.mark.parametrize("c", fc.SEG_CHANNELS)
def test_interpolation_forward_and_backward(c, lib, dev):
    fc.check_interp_fwd(lib, dev, c)
    fc.check_interp_bwd(lib, dev, c)
    if c in (33, 256):
        fc.check_interp_fwd(lib, dev, c, misalign=True)


def test_python_level_refusals(lib, dev):
    x = fc.values((10, 4), 1, dev)
    keys = torch.zeros(10, dtype=torch.int32, device=dev)
    offsets, perm = lib.group(keys, 2)
    with pytest.raises(TypeError, match="fp32"):
        lib.seg_rows(x.double(), offsets, perm, fc.SUM)
    with pytest.raises(TypeError, match="fp32"):
        lib.gather_w(x.half(), keys, x[:, 0].contiguous())
    with pytest.raises(ValueError, match="2\\^31"):
        lib.group(keys, 1 << 31)
    with pytest.raises(RuntimeError, match="pq_seg_rows: seg_rows: mode = 7"):
        lib.seg_rows(x, offsets, perm, 7)
    with pytest.raises(RuntimeError, match="the maximum takes no weights"):
        lib.seg_rows(x, offsets, perm, fc.MAX, w=x[:, 0].contiguous())
    import pasco_amd.me as ME
    feats, coords = fc.cloud(n=50)
    with pytest.raises(TypeError, match="fp32 rows on the device"):
        ME.TensorField(feats.to(dev).double(), coords.to(dev)).sparse()
    with pytest.raises(TypeError, match="fp32 rows on the device"):
        st = ME.TensorField(feats.to(dev), coords.to(dev)).sparse()
        ME.SparseTensor(st.F.half(), coordinate_map_key=st.coordinate_map_key, coordinate_manager=st.coordinate_manager).slice(
            ME.TensorField(feats.to(dev), coords.to(dev), coordinate_manager=st.coordinate_manager))
    fc.check_refusals(dev)


# ---- the modules on the device ---------------------------------------------------------------------------------------------------
def test_sparse_in_every_mode_against_the_dense_twin(lib, dev):
    fc.check_sparse_against_dense(dev, torch.float32)
    fc.check_sparse_against_dense(dev, torch.float32, ts=2)


def test_slice_interpolation_and_existing_behaviour(lib, dev):
    fc.check_floor_below_boundaries(dev)
    fc.check_slice_and_interpolation(dev, torch.float32)
    fc.check_interpolation_against_grid_sample(dev, torch.float32)
    fc.check_existing_behaviour(dev)
    fc.check_prologue(dev)


@pytest.mark.parametrize("name", fc.MODULE_NAMES)
def test_module_modes_give_the_same_bits(name, lib, dev):
    fc.check_module_modes(dev, torch.float32, name)


@pytest.mark.parametrize("name", fc.MODULE_NAMES)
def test_modules_against_the_cpu_route_in_fp64(name, lib, dev, cpu_route):
    """Values: every route but the selections is linear in the features with non-negative coefficients, so the same route run
    on |features| in fp64 is the magnitude sum |w_j x_j| of every output element; a voxel of m points costs m + 1 roundings of
    it, the eight corners 16 more: (m_max + 17) u with m_max the fullest voxel of the cloud at tensor stride 2.  A zero
    magnitude (a row nothing contributes to) must be exactly zero.  Selections are exact.
    Gradients: within 1e-4 of the largest entry, the project's margin for a few hundred rows."""
    from tests.field_ref64 import dense_quantise
    out, grad = fc.module_gradients(dev, torch.float32, name)
    want, want_grad = fc.module_gradients(cpu_route, torch.float64, name)
    assert out.shape == want.shape and grad.shape == want_grad.shape
    if name in ("sparse_max_pool", "tensor_max_pool", "sparse_random_subsample"):
        assert torch.equal(out, want), name
    else:
        feats, runs = fc.module_runs(cpu_route, torch.float64)
        mag = runs[name](feats.abs()).double()
        m_max = float(dense_quantise(*fc.cloud(n=300), 2, "sum")[1].max())
        err = (out - want).abs()
        assert bool((err <= (m_max + 17) * U * mag).all()), f"{name}: {float((err / ((m_max + 17) * U * mag).clamp(min=1e-300)).max()):.2f} x the bound"
    assert float((grad - want_grad).abs().max()) <= 1e-4 * float(want_grad.abs().max()), name


def test_small_net_against_the_dense_fp64_twin(lib, dev):
    """points (3 000, batch 2) -> TensorField (average) -> sparse -> conv(4, 16, k = 3) -> BN -> ReLU -> slice -> Linear -> loss:
    every parameter's gradient and the input features' against the dense fp64 twin, 1e-4 of the largest entry; two runs give the
    same bits."""
    params, grads, (feats, coords, target) = fc.net_gradients(dev)
    twin = fc.net_twin_gradients(params, feats, coords, target)
    assert set(twin) == set(grads) and len(grads) == 6
    for k, g in grads.items():
        w = twin[k]
        err, top = float((g.double().cpu() - w).abs().max()), float(w.abs().max())
        print(f"{k}: max |g - g64| = {err:.3e}, max |g64| = {top:.3e}")
        assert g.shape == w.shape and err <= 1e-4 * top, k
    _, again, _ = fc.net_gradients(dev)
    for k, g in grads.items():
        assert torch.equal(g, again[k]), k


# ---- the stream contract -------------------------------------------------------------------------------------------------------
def _seg_make(seed, device):
    keys, n_seg, _ = fc.seg_case(device)
    keys = keys.clamp(min=0)                                 # every entry present: the whole of perm is specified
    n, c = keys.numel(), 260
    g = sc._gen(seed)
    return {"keys": keys.to(device), "n_seg": n_seg, "x": torch.randn(n, c, generator=g).to(device),
            "w": torch.randn(n, generator=g).to(device), "dy": torch.randn(n_seg, c, generator=g).to(device),
            "d": (torch.randint(0, 5, (n,), generator=g)).float().to(device)}


def _seg_run(d):
    from pasco_amd.grad.fieldlib import field_lib
    L = field_lib()
    offsets, perm = L.group(d["keys"], d["n_seg"])
    s, cnt, _ = L.seg_rows(d["x"], offsets, perm, fc.SUM, w=d["w"])
    a = L.seg_rows(d["x"], offsets, perm, fc.AVG)[0]
    m, _, arg = L.seg_rows(d["x"], offsets, perm, fc.MAX)
    return (offsets, perm, s, cnt, a, m, arg, L.seg_max_bwd(d["dy"], arg, d["x"].shape[0]),
            L.gather_w(d["x"], d["keys"], d["d"]))


def _interp_make(seed, device):
    mgr, key, vox = fc.voxel_map(device, 2, 0)
    g = sc._gen(seed)
    cmap = mgr._maps[key]
    pts = torch.cat([torch.zeros(300, 1), torch.rand(300, 3, generator=g) * 6 - 3], dim=1)
    return {"points": pts.to(device), "tkeys": cmap.tkeys.clone(), "tvals": cmap.tvals.clone(), "_ts": 2,
            "x": torch.randn(vox.shape[0], 33, generator=g).to(device), "dy": torch.randn(300, 33, generator=g).to(device)}


def _interp_run(d):
    from pasco_amd.grad.fieldlib import field_lib
    L = field_lib()
    rows, weights = L.interp_map(d["points"], d["tkeys"], d["tvals"], d["_ts"])
    out = L.interp_fwd(d["x"], rows, weights)
    offsets, perm = L.group(rows.reshape(-1), d["x"].shape[0])
    dx = L.seg_rows(d["dy"], offsets, perm, fc.SUM, w=weights.reshape(-1), src_mod=rows.shape[1])[0]
    return rows, weights, out, offsets, dx                  # (the tail of perm, behind the present entries, is unspecified)


STREAM_ENTRIES = [
    sc.Entry("pq.segments", "pq", ("group", "seg_rows", "seg_max_bwd", "gather_w"), _seg_make, _seg_run),
    sc.Entry("pq.interpolation", "pq", ("interp_map", "interp_fwd", "group", "seg_rows"), _interp_make, _interp_run),
]


def test_stream_table_covers_every_launching_entry():
    from pasco_amd.grad import fieldlib
    launching = set(fieldlib._SIGNATURES) - {"abi_version", "last_error", "group_workspace_bytes"}
    assert {n for e in STREAM_ENTRIES for n in e.covers} == launching


def _side_stream(dev, producer, tries: int = 32):
    """A side stream that the null stream demonstrably overtakes (tests/stream_cases.SideStreams' criterion), taken from torch's
    HIGH-priority pool: the default-priority pool, which the stream-choosing fixtures of the other modules draw from round
    robin, is not touched, so those modules are handed the streams they would be handed without this one."""
    null, seen = torch.cuda.default_stream(dev), set()
    for _ in range(tries):
        s = torch.cuda.Stream(dev, priority=-1)
        if s.cuda_stream in seen:
            continue
        seen.add(s.cuda_stream)
        if sc.overtakes(s, null, producer, dev):
            return s
    raise AssertionError(f"none of {len(seen)} side streams runs concurrently with the null stream: a mis-streamed launch cannot "
                         f"be seen here and the method is void")


@pytest.fixture(scope="module")
def side(dev, hip):
    producer = sc.Producer(dev)
    stream = _side_stream(dev, producer)
    yield producer, stream
    hip.release_stream(stream)               # (order_check releases after every call; nothing of this module stays keyed by the handle)


@pytest.mark.parametrize("entry", STREAM_ENTRIES, ids=[e.name for e in STREAM_ENTRIES])
def test_same_bits_on_a_side_stream_behind_a_pending_producer(entry, lib, dev, side):
    """tests/stream_cases.order_check: the call on a side stream that the null stream demonstrably overtakes, behind pending
    work, with nothing enqueued on the null stream, gives the bits of the null-stream run; and the per-stream scratch the
    family took ("field") is gone once the stream is released."""
    producer, stream = side
    report = sc.order_check(entry, dev, producer, stream=stream)
    assert not report.failures, report.failures
    from pasco_amd.me.backend import hip_backend
    assert hip_backend().scratch.held(stream) == set()
