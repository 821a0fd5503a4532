"""The pk_* kernels (include/pasco_knn.h) and `knn_up` of pasco_amd.grad.knn on the MI355X: the search bit for bit against the
literal all-pairs fp32 loop, weights / forward / backward against fp64 at the header's a-priori bounds, the drop-in module against
the fp64 restatement of the module it stands in for, the MinkUNet-shaped network against its dense fp64 twin, and the family's
contracts (the same bits from two runs and on a side stream, refusals with a message).  The cases, the shared checks and the
references are tests/knn_cases.py; the CPU side is tests/test_knn_cpu.py."""
import pytest
import torch

from tests import knn_cases as kc
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.knnlib import knn_lib
    return knn_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


@pytest.mark.parametrize("case", kc.sizes_cases(), ids=[c[0] for c in kc.sizes_cases()])
def test_search_sizes_bit_for_bit(case, lib, dev):
    name, cand, q, k, grid = case
    kc.check_search(dev, cand, q, k, grid, what=name)


@pytest.mark.parametrize("case", kc.edge_cases(), ids=[c[0] for c in kc.edge_cases()])
def test_search_edges_bit_for_bit(case, lib, dev):
    name, cand, q, k, grid = case
    kc.check_search(dev, cand, q, k, grid, what=name)


def test_search_edge_expectations(lib, dev):
    kc.check_edge_expectations(dev)


@pytest.mark.parametrize("k", kc.KS)
def test_search_through_a_column_view_of_batched_coordinates(k, lib, dev):
    """ldc = ldq = 4, both bases 4 bytes past a 16-byte boundary."""
    vox, q = kc.recipe()
    kc.check_search(dev, vox, q[:2 * kc.QB + 1], k, kc.grid_around(vox, 0.5), padded=True, what=f"padded k={k}")


def test_search_is_the_same_on_every_grid(lib, dev):
    """The cell edge decides the work, never the answer: a coarse grid, a fine one and a single cell."""
    vox, q = kc.recipe()
    first = None
    for h in (0.25, 0.5, 3.0, 100.0):
        idx, d2 = kc.search(dev, vox, q[:300], 8, kc.grid_around(vox, h))
        first = (idx, d2) if first is None else first
        assert torch.equal(idx, first[0]) and kc.same_bits(d2, first[1]), h
    kc.check_search(dev, vox, q[:300], 8, kc.grid_around(vox, 100.0), what="one cell")


def test_host_restatement_gives_the_same_answers(lib, dev):
    vox, q = kc.recipe()
    for k in kc.KS:
        a = kc.search(dev, vox, q, k)
        b = kc.search(torch.device("cpu"), vox, q, k)
        assert torch.equal(a[0], b[0]) and kc.same_bits(a[1], b[1]), k


@pytest.mark.parametrize("k", kc.KS)
def test_weights_against_fp64(k, lib, dev):
    kc.check_weights(dev, k)


@pytest.mark.parametrize("c", kc.CHANNELS)
def test_forward_against_fp64(c, lib, dev):
    kc.check_forward(dev, c)
    kc.check_forward(dev, c, k=16)


def test_forward_at_a_misaligned_base_and_with_one_neighbour(lib, dev):
    kc.check_forward(dev, 33, misalign=True)
    kc.check_forward(dev, 256, misalign=True)                # a multiple of four 4 bytes past a boundary: scalar
    kc.check_forward(dev, 4, k=1)


@pytest.mark.parametrize("c", (1, 4, 33, 256))
def test_backward_against_fp64_and_two_runs(c, lib, dev):
    kc.check_backward(dev, c)
    kc.check_backward(dev, c, k=16)


@pytest.mark.parametrize("k", kc.KS)
def test_knn_up_against_the_fp64_restatement(k, lib, dev):
    kc.check_knn_up(dev, k)


def test_grad_modes_give_the_same_bits(lib, dev):
    kc.check_grad_modes(dev)


def test_refusals(lib, dev):
    kc.check_refusals(dev)


def test_unet_gradients_against_the_dense_fp64_twin(lib, dev):
    """Fails without the feature at the first up-convolution: a transposed convolution onto the encoder's map."""
    grads = kc.check_net(dev)
    again = kc.net_gradients(dev)[1]
    for k, g in grads.items():
        assert torch.equal(g, again[k]), k


# ---- the stream contract -------------------------------------------------------------------------------------------------------
def _make(seed, device):
    vox, q = kc.recipe()
    g = sc._gen(seed)
    n, m, k = vox.shape[0], 300, 8
    return {"cand": torch.from_numpy(vox).to(device), "q": (torch.rand(m, 3, generator=g) * 8 - 1).to(device),
            "x": torch.randn(n, 33, generator=g).to(device), "dy": torch.randn(m, 33, generator=g).to(device), "_k": k}


def _run(d):
    from pasco_amd.grad.knnlib import knn_lib
    L = knn_lib()
    grid = kc.grid_around(kc.recipe()[0], 0.5)
    status = torch.zeros(1, dtype=torch.int32, device=d["cand"].device)
    start, order = L.csr(d["cand"], grid, status)
    idx, d2 = L.knn(d["cand"], start, order, grid, d["q"], d["_k"])
    w = L.weights(d2, idx)
    return idx, d2, w, L.interp_fwd(d["x"], idx, w), L.interp_bwd(d["dy"], idx, w, d["x"].shape[0]), status


STREAM_ENTRIES = [sc.Entry("pk.knn_up", "pk", ("knn", "weights", "interp_fwd"), _make, _run)]


def test_stream_table_covers_every_launching_entry():
    from pasco_amd.grad import knnlib
    launching = set(knnlib._SIGNATURES) - {"abi_version", "last_error"}
    assert {n for e in STREAM_ENTRIES for n in e.covers} == launching


def _side_stream(dev, producer, tries: int = 32):
    """A side stream that the null stream demonstrably overtakes, from torch's HIGH-priority pool (as tests/test_hip_field.py
    takes its own): the default-priority pool the other modules draw from is not touched."""
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
    hip.release_stream(stream)


@pytest.mark.parametrize("entry", STREAM_ENTRIES, ids=[e.name for e in STREAM_ENTRIES])
def test_same_bits_on_a_side_stream_behind_a_pending_producer(entry, lib, dev, side):
    producer, stream = side
    report = sc.order_check(entry, dev, producer, stream=stream)
    assert not report.failures, report.failures
    from pasco_amd.me.backend import hip_backend
    assert hip_backend().scratch.held(stream) == set()
