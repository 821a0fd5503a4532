"""The attention backward on libpascohip.so (csrc/attn_grad.hip, include/pasco_attngrad.h): the cases of
tests/attn_grad_cases.py held to the fp64 gradients of tests/attn_grad_ref64.py by
    max |g - g64| <= ATTN_GRAD_M x max |g32 - g64|      (g32 = torch fp32 autograd of the materialised formulation, on the CPU)
then what only the device side has: bit-equal repeats, the declared workspace and its canary, refusals that launch nothing, NULL
outputs, the memory a backward takes.  Every launch gets a scratch of exactly pa_attn_bwd_workspace_bytes followed by a canary.
The CPU side is tests/test_attn_grad_cpu.py."""
import pytest
import torch

from tests import attn_grad_cases as ac
from tests import attn_grad_ref64 as gref
from tests.attn_edge_cases import DH, GUARD

pytestmark = pytest.mark.gpu

PATTERN = 7.0


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def raw_bwd(lib, q, k, v, bits, any_, out, dout, need_q=True, need_k=True, need_v=True, short=0, dh=DH, prefill=None):
    """pa_attn_cross_bwd with a scratch of exactly the declared size (minus `short`) and a canary behind it -> (dq, dk, dv, rc)."""
    B, H, Q, _ = q.shape
    N = k.shape[1]
    need = lib.workspace_bytes(N, B, H, Q)
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device=q.device)
    ws[need:] = 0x5A
    mk = (lambda t: torch.full_like(t, prefill)) if prefill is not None else torch.empty_like
    dq, dk, dv = (mk(t) if n else None for t, n in ((q, need_q), (k, need_k), (v, need_v)))
    rc = lib.lib.pa_attn_cross_bwd(_p(q), _p(k), _p(v), _p(bits), _p(any_), _p(out), _p(dout), _p(dq), _p(dk), _p(dv), N, B, H, Q, dh,
                                   ws.data_ptr(), need - short, _stream(q.device))
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "pa_attn_cross_bwd wrote past its declared workspace"
    return dq, dk, dv, rc


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.attnlib import attn_grad_lib
    return attn_grad_lib()


@pytest.fixture(scope="module")
def runner(hip, lib):
    def bwd(*a):
        dq, dk, dv, rc = raw_bwd(lib, *a)
        assert rc == 0, lib.lib.pa_last_error()
        return dq, dk, dv
    return ac.Runner(torch.device("cuda", 0), hip.attn_cross_fwd, bwd, gref.ATTN_GRAD_M, "hip")


@pytest.mark.parametrize("pattern", ac.PATTERNS)
@pytest.mark.parametrize("shape", ac.SHAPES, ids=lambda s: "B%d_H%d_Q%d_N%d" % s)
def test_hip_gradients_against_fp64(runner, shape, pattern):
    ac.check_precision(runner, shape, pattern)


def test_hip_unattended_keys_get_exact_zero_rows(runner):
    ac.check_unattended_keys(runner)


def test_hip_garbage_bits_beyond_q_change_nothing(runner):
    ac.check_garbage_bits(runner)


def test_hip_ranges_that_start_fully_masked(runner):
    ac.check_masked_range_start(runner)


@pytest.mark.parametrize("shape", [(1, 1, 16, 16), ac.MULTI], ids=["one_range", "multi_range"])
def test_hip_two_calls_return_the_same_bits(runner, shape):
    assert ac.bwd_geometry(*shape)["splits"] == (1 if shape != ac.MULTI else 86)
    x = ac.inputs(shape, "mask_any")
    a, b = runner.grads(x), runner.grads(x)
    for name, s, t in zip(("dq", "dk", "dv"), a, b):
        assert torch.equal(s, t), name


def test_hip_statistics_pass(hip, lib):
    """lse and delta of pa_attn_bwd_stats against fp64; +inf for the query with nothing allowed."""
    dev = torch.device("cuda", 0)
    shape = ac.MULTI
    B, H, Q, N = shape
    x = ac.inputs(shape, "mask_noany")
    bits, _ = x.words()
    q, k, v, dout, bits = (t.to(dev) for t in (x.q, x.k, x.v, x.dout, bits))
    out = hip.attn_cross_fwd(q, k, v, bits, None)
    lse, delta = lib.attn_bwd_stats(q, k, bits, None, out, dout)
    al, dead = gref.effective_allow(x.allow, False)
    s = torch.matmul(x.q.double(), x.k.double().view(B, N, H, DH).permute(0, 2, 3, 1)).masked_fill(~al[:, None], float("-inf"))
    lse64 = torch.logsumexp(s, dim=-1)
    lse64 = torch.where(dead[:, None].expand_as(lse64), torch.full_like(lse64, float("inf")), lse64)
    delta64 = (x.dout.double() * x.g64[3]).view(B, Q, H, DH).sum(-1).transpose(1, 2)
    live = ~dead[:, None].expand_as(lse64)
    assert bool(torch.isinf(lse.cpu()[~live]).all()) and bool((lse.cpu()[~live] > 0).all())
    err = float((lse.cpu().double()[live] - lse64[live]).abs().max())
    print(f"ATTN_GRAD_LSE max |lse - lse64| = {err:.3e}")
    assert err <= gref.LSE_ATOL
    derr = float((delta.cpu().double() - delta64).abs().max())
    print(f"ATTN_GRAD_DELTA max |delta - delta64| = {derr:.3e}")
    assert derr <= gref.LSE_ATOL
    assert not bool(delta.cpu()[~live].any())


def test_hip_refusals_launch_nothing(hip, lib):
    dev = torch.device("cuda", 0)
    x = ac.inputs((1, 2, 17, 15), "plain")
    q, k, v, dout = (t.to(dev) for t in (x.q, x.k, x.v, x.dout))
    out = hip.attn_cross_fwd(q, k, v)

    def refused(what, *a, **kw):
        dq, dk, dv, rc = raw_bwd(lib, *a, prefill=PATTERN, **kw)
        assert rc != 0, what
        assert lib.lib.pa_last_error(), what
        for t in (dq, dk, dv):
            assert t is None or bool((t == PATTERN).all()), what
        return lib.lib.pa_last_error().decode()

    assert "workspace" in refused("short workspace", q, k, v, None, None, out, dout, short=1)
    assert "head dim" in refused("another dh", q, k, v, None, None, out, dout, dh=32)
    for i, name in enumerate(("q", "k", "v", "bits", "any", "out", "dout")):
        if name in ("bits", "any"):
            continue
        args = [q, k, v, None, None, out, dout]
        args[i] = None
        B, H, Q, _ = q.shape
        N = k.shape[1]
        need = lib.workspace_bytes(N, B, H, Q)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        outs = [torch.full_like(t, PATTERN) for t in (q, k, v)]
        rc = lib.lib.pa_attn_cross_bwd(*[_p(t) for t in args], *[_p(t) for t in outs], N, B, H, Q, DH, ws.data_ptr(), need, _stream(dev))
        torch.cuda.synchronize()
        assert rc != 0 and b"null" in lib.lib.pa_last_error(), name
        assert all(bool((t == PATTERN).all()) for t in outs), name
    assert "no output" in refused("no output wanted", q, k, v, None, None, out, dout, need_q=False, need_k=False, need_v=False)
    q129 = torch.zeros(1, 2, 129, DH, device=dev)
    o129 = torch.zeros(1, 129, 2 * DH, device=dev)
    assert "129 queries" in refused("129 queries", q129, k, v, None, None, o129, o129)


def test_hip_null_outputs_leave_the_others_bit_for_bit(runner):
    x = ac.inputs(ac.MULTI, "mask_any")
    full = runner.grads(x)
    for i in range(3):
        part = runner.grads(x, need=tuple(j != i for j in range(3)))
        assert part[i] is None
        for j in range(3):
            assert j == i or torch.equal(part[j], full[j]), (i, j)
    only_v = runner.grads(x, need=(False, False, True))
    assert torch.equal(only_v[2], full[2])


def test_hip_masked_cross_attention_gradient_and_inference_route(hip):
    ac.check_autograd_route(hip, torch.device("cuda", 0), gref.ATTN_GRAD_M)


def test_hip_cross_attention_layer_against_the_multihead_attention_twin(hip):
    ac.check_layer(torch.device("cuda", 0), gref.ATTN_GRAD_M, "hip")


def test_hip_backward_memory_has_no_score_tensor(hip, lib):
    """B = 1, H = 8, Q = 100, N = 20 000: the score tensor alone would be 64 MB.  Across backward() the peak of
    torch.cuda.max_memory_allocated rises over the level before the call by at most the gradients, the declared workspace and
    1 MiB.

    The counter is the caching allocator's: it counts a large block WHOLE when the tail behind the request is at most 1 MiB, so
    dk and dv (30 720 000 bytes each) served from fresh 2 MiB-granular segments are counted as 31 457 280 each - 1.4 MiB that
    no tensor holds (measured so: rise 108 029 440 = gradients 61 593 600 + workspace 44 807 168 + dout 153 600 + 512 + those
    1 474 560).  So that the counter measures the requests, the cache is emptied and then given ONE large free block before the
    level is taken: every request of the backward is split off it at its own size (rounded to 512 bytes)."""
    from pasco_amd.grad.attention import masked_cross_attention
    dev = torch.device("cuda", 0)
    B, H, Q, N = 1, 8, 100, 20000
    g = torch.Generator(device=dev).manual_seed(20000)
    q = (torch.randn(B, H, Q, DH, device=dev, generator=g) * DH ** -0.5).requires_grad_(True)
    k = (torch.randn(B, N, H * DH, device=dev, generator=g) * 1.7).requires_grad_(True)
    v = torch.randn(B, N, H * DH, device=dev, generator=g).requires_grad_(True)
    allow = torch.rand(B * N, Q, device=dev, generator=g) < 0.3
    words = hip.attn_mask_pack(allow.float(), B, N)
    w = torch.randn(B, Q, H * DH, device=dev, generator=g)
    del allow
    loss = (masked_cross_attention(q, k, v, words) * w).sum()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    del_me = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    del del_me
    torch.cuda.reset_peak_memory_stats(dev)
    before = torch.cuda.memory_allocated(dev)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated(dev) - before
    grads = 4 * (q.numel() + k.numel() + v.numel())
    ws = lib.workspace_bytes(N, B, H, Q)
    print(f"ATTN_GRAD_MEMORY rise {rise} bytes; gradients {grads}, workspace {ws}, score tensor {4 * B * H * Q * N}")
    assert rise <= grads + ws + (1 << 20)
    assert all(bool(torch.isfinite(t.grad).all()) for t in (q, k, v))
