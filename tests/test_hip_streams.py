"""The stream contract of the eight training families (pg_*, pr_*, pa_*, pm_*, ps_*, pt_*, pn_*, po_*) off the null stream:
every launching entry point behind a pending producer on a side stream, the families with per-stream scratch on two streams
at once, every entry point captured and replayed, and the autograd layers over them on a side stream.  The table and the
harness are tests/stream_cases.py, the method DESIGN.md 4v.  Two planted fakes at the end show that the harness can fail."""
import pytest
import torch

from tests import stream_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def producer(dev):
    p = sc.Producer(dev)
    print(f"[streams] producer: {'torch.cuda._sleep' if p.sleep is not None else 'matmul chain'}, {p.units_per_ms:.0f} units per ms")
    return p


@pytest.fixture(scope="module")
def side(dev, producer):
    """Side streams that demonstrably run concurrently with the null stream and with each other."""
    st = sc.SideStreams(dev, producer)
    print(f"[streams] side streams: looked at {st.tried}, {st.shared} share a queue with the null stream or a chosen one, "
          f"chose {len(st.streams)}")
    return st


# ---- part 2: order behind a pending producer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sc.ENTRIES, ids=sc.ENTRY_IDS)
def test_order_behind_a_pending_producer(dev, producer, side, entry):
    """The call on a side stream, its operands copied in behind a producer that is still running when the call returns: the
    results are the bits of the default-stream run, not those of the operands' earlier values, and the call did not wait."""
    r = sc.order_check(entry, dev, producer, side.one())
    print(f"[streams] {r.name}: host {r.host_ms:.3f} ms, producer {r.producer_ms:.1f} ms, busy {r.busy}")
    assert not r.failures, "\n".join(r.failures)


# ---- part 3: two streams at once -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sc.PAIR_ENTRIES, ids=[e.name for e in sc.PAIR_ENTRIES])
def test_two_streams_at_once(dev, producer, side, entry):
    """Two streams released by one event issue the call alternately on different seeds: every result is that of its serial run,
    and the scratch each stream cached is found, once, by release_stream."""
    failures, first, second = sc.pair_check(entry, dev, producer, side.two())
    assert not failures, "\n".join(failures)
    if entry.caches_scratch:
        assert all(n > 0 for n in first), f"release_stream found no scratch of a stream that cached some: {first}"
    else:
        assert first == [0, 0], f"a per-call workspace was kept for the stream: {first}"
    assert second == [0, 0]


# ---- part 4: capture and replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", sc.ENTRIES, ids=sc.ENTRY_IDS)
def test_capture_and_replay(dev, side, entry):
    """One call captured on a side stream (single stream, linear), other values copied into its operands, one replay: the bits
    of an eager call on those values."""
    failures = sc.capture_check(entry, dev, side.one())
    assert not failures, "\n".join(failures)


# ---- the autograd layers on a side stream --------------------------------------------------------------------------------------
def _on_side_stream(dev, producer, s, fn):
    """fn() inside `with torch.cuda.stream(s)` behind the producer, then fn() on the default stream -> both results."""
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(s):
            producer.run(sc.FLOOR_MS)
            got = fn()
            s.synchronize()
    finally:
        sc.release(s)
    want = fn()
    torch.cuda.synchronize(dev)
    return got, want


@pytest.mark.parametrize("which", ["stack_gradients", "row_stack_gradients"])
def test_conv_stacks_on_a_side_stream(dev, producer, side, which):
    """Forward and backward of the two module stacks (convolutions, batch norm, pooling, dense and back) on a side stream: every
    gradient has the bits of the default-stream run.  The CoordinateManager synchronises by design, so nothing is asserted
    about the stream being busy."""
    from tests import grad_cases, rowgrad_cases
    fn = grad_cases.stack_gradients if which == "stack_gradients" else rowgrad_cases.row_stack_gradients
    got, want = _on_side_stream(dev, producer, side.one(), lambda: {k: v[0].clone() for k, v in fn(dev).items()})
    assert got.keys() == want.keys() and len(got) > 5
    for k in want:
        assert sc.bits_equal(got[k], want[k]), f"{which}: the gradient of {k} differs on a side stream"


def _leaf_run(dev, producer, s, make, forward):
    """`make(seed)` -> a dict of leaves and constants; forward(d) -> (outputs, output gradients).  The leaves hold seed B's
    values until copies queued behind the producer bring seed A's; forward and backward follow on the same stream."""
    def run(d):
        outs, gouts = forward(d)
        torch.autograd.backward(outs, gouts)
        return tuple(o.detach().clone() for o in outs) + tuple(v.grad.clone() for v in d.values()
                                                                if isinstance(v, torch.Tensor) and v.requires_grad)
    real, work, warm = make(sc.SEED_A), make(sc.SEED_B), make(sc.SEED_B)      # every host-to-device copy before the producer
    torch.cuda.synchronize(dev)
    try:
        with torch.cuda.stream(s):
            run(warm)                                 # the workspaces of this stream
            s.synchronize()
            producer.run(sc.FLOOR_MS)
            with torch.no_grad():
                for k, v in work.items():
                    if isinstance(v, torch.Tensor):
                        v.copy_(real[k], non_blocking=True)
            got = run(work)
            s.synchronize()
    finally:
        sc.release(s)
    want, other = run(make(sc.SEED_A)), run(make(sc.SEED_B))
    torch.cuda.synchronize(dev)
    assert sc.bits_equal(got, want), "the side-stream run differs from the default-stream run"
    assert not sc.bits_equal(want, other), "the two seeds give the same result"


def test_attention_function_on_a_side_stream(dev, producer, side):
    from pasco_amd.grad.attention import masked_cross_attention
    entry = sc._make_attn((2, 8, 100, 333))

    def make(seed):
        d = entry(seed, dev)
        d.pop("fwd")
        for k in ("q", "k", "v"):
            d[k].requires_grad_(True)
        return d
    _leaf_run(dev, producer, side.one(), make,
              lambda d: ((masked_cross_attention(d["q"], d["k"], d["v"], (d["bits"], d["any"])),), (d["dout"],)))


def test_mask_loss_function_on_a_side_stream(dev, producer, side):
    from pasco_amd.grad.criterion import MaskLossFunction
    src = torch.tensor([0, 2, 3], device=dev)

    def make(seed):
        d = sc._pm_operands(seed, dev)
        d = {k: d[k] for k in ("logits", "tbits", "flags")}
        d["logits"].requires_grad_(True)
        g = sc._gen(seed, 5)
        d["tgt"] = torch.randperm(sc.PM_T, generator=g)[:3].to(dev)
        d["weights"] = (torch.rand(3, generator=g) + 0.5).to(dev)
        d["g_mask"], d["g_dice"] = torch.randn(3, generator=g).to(dev), torch.randn(3, generator=g).to(dev)
        return d

    def forward(d):
        lm, ld = MaskLossFunction.apply(d["logits"], d["tbits"], d["flags"], src, d["tgt"], d["weights"], sc.PM_T)
        return (lm, ld), (d["g_mask"], d["g_dice"])
    _leaf_run(dev, producer, side.one(), make, forward)


def test_adamw_step_on_a_side_stream(dev, producer, side):
    """Two steps of `AdamW` on a side stream.  The first builds and uploads the tables and may wait; the second, on warm tables
    with its gradients copied in behind a pending producer, returns while the producer is still running, and parameters,
    moments and records have the bits of the default-stream run."""
    from pasco_amd.grad.optim import AdamW
    from tests import optim_cases as oc
    values, grads = oc.case_values(2, seed=sc.SEED_A)
    on_dev = [[g.to(dev) for g in step] for step in grads]
    filler = [[torch.zeros_like(g) + 0.5 for g in step] for step in on_dev]

    def two_steps(stream):
        ps = oc.make_params(values, dev, offset_last=False)
        opt = oc.make_optimizer(ps, max_norm=oc.CLIP)
        for p, g in zip(ps, on_dev[0]):
            p.grad = g.clone()
        torch.cuda.synchronize(dev)
        busy = None
        with torch.cuda.stream(stream):
            opt.step()
            stream.synchronize()
            for p, g in zip(ps, filler[1]):          # valid gradients that are not the second step's
                p.grad.copy_(g)
            torch.cuda.synchronize(dev)
            if stream is not torch.cuda.default_stream(dev):
                producer.run(sc.FLOOR_MS)
            for p, g in zip(ps, on_dev[1]):
                p.grad.copy_(g, non_blocking=True)
            opt.step()
            busy = not stream.query()
            stream.synchronize()
        st = oc.our_state(ps, opt)
        return busy, tuple(st["p"] + st["m"] + st["v"]) + (opt._buffers().states.clone(), opt._buffers().result.clone())

    busy, got = two_steps(side.one())
    _, want = two_steps(torch.cuda.default_stream(dev))
    assert sc.bits_equal(got, want), "two steps on a side stream differ from two steps on the default stream"
    assert busy, "the second step, on warm tables, waited for the device (or the producer was too short)"


# ---- the scratch table itself --------------------------------------------------------------------------------------------------
def test_scratch_table_is_per_stream(dev):
    """`StreamScratch` on two side streams of one device: every name has storage of its own per stream, `release` of one
    stream returns exactly the number of names it held and leaves the other stream's buffers and its status address alone.
    No launch of ours."""
    from pasco_amd._clib import StreamScratch
    table = StreamScratch()
    s0, s1 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    assert s0.cuda_stream != s1.cuda_stream
    held, ptr = {}, {}
    for s in (s0, s1):
        with torch.cuda.stream(s):
            assert StreamScratch.key(torch.device("cuda")) == StreamScratch.key(dev) == (dev, s.cuda_stream)
            held[s] = (table.bytes("ws", dev, 100, floor=1 << 20), table.bytes("attn", dev, 100), table.words("status", dev, 2))
            ptr[s] = table.status_ptr(dev)
            assert ptr[s] == held[s][2].data_ptr() and table.get("status", dev) is held[s][2]
    assert [t.numel() for t in held[s0]] == [1 << 20, 100, 2]
    for a, b in zip(held[s0], held[s1]):
        assert a.data_ptr() != b.data_ptr() and a.device == b.device == dev
    with torch.cuda.stream(s0):
        table.words("keep_any", dev, 1)
    assert table.held(s0) == {"ws", "attn", "status", "keep_any"} and table.held(s1) == {"ws", "attn", "status"}
    assert table.held(torch.cuda.default_stream(dev)) == set()
    assert table.release(s0) == 4 and table.held(s0) == set() and table.release(s0) == 0
    assert table.held(s1) == {"ws", "attn", "status"}
    with torch.cuda.stream(s1):
        assert table.status_ptr(dev) == ptr[s1] and table.words("status", dev, 2) is held[s1][2]
        assert table.bytes("ws", dev, 100, floor=1 << 20) is held[s1][0] and table.bytes("attn", dev, 100) is held[s1][1]
    assert table.release(s1.cuda_stream) == 3 and table.held() == set(), "a raw handle: the streams of the current device"


# ---- part 5: the harness can fail ----------------------------------------------------------------------------------------------
def _make_fake(seed, dev):
    return {"x": torch.randn(4099, generator=sc._gen(seed)).to(dev)}


def _run_mis_streamed(d):
    """Two ops, the first of them issued on the default stream whatever the current stream is."""
    with torch.cuda.stream(torch.cuda.default_stream(d["x"].device)):
        a = d["x"] * 3.0
    return (a + d["x"],)


def _run_hidden_read(d):
    y = d["x"] * 2.0
    y.sum().item()
    return (y,)


def test_harness_reports_a_mis_streamed_op(dev, producer, side):
    """If this passed with no mismatch reported, torch's side streams would block on the null stream here and the whole method
    would be void."""
    fake = sc.Entry("fake.mis_streamed", "fake", (), _make_fake, _run_mis_streamed)
    r = sc.order_check(fake, dev, producer, side.one())
    assert r.busy, "the producer had ended: the fake shows nothing"
    assert len(r.failures) == 1 and "differs from the default-stream run" in r.failures[0], r.failures


def test_harness_reports_a_hidden_read(dev, producer, side):
    fake = sc.Entry("fake.hidden_read", "fake", (), _make_fake, _run_hidden_read)
    r = sc.order_check(fake, dev, producer, side.one())
    assert not r.busy
    assert len(r.failures) == 1 and "had drained when the call returned" in r.failures[0], r.failures


def test_harness_passes_a_well_behaved_op(dev, producer, side):
    fake = sc.Entry("fake.plain", "fake", (), _make_fake, lambda d: (d["x"] * 3.0 + d["x"],))
    r = sc.order_check(fake, dev, producer, side.one())
    assert r.busy and not r.failures, r.failures
