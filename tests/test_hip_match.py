"""The matcher and mask-loss family on libpascohip.so (csrc/match.hip, include/pasco_match.h): the cases of tests/match_cases.py
held to tests/match_ref64.py by the ratio rule with PM_M, then what only the device side has: bit-equal repeats, the declared
workspace and its canary, refusals that launch nothing, the memory a matcher + loss + backward takes.  The CPU side is
tests/test_match_cpu.py."""
import pytest
import torch

from tests import match_cases as mc
from tests import match_ref64 as mref

pytestmark = pytest.mark.gpu

PATTERN = 7.0
GUARD = 4096


def _p(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.matchlib import match_lib
    return match_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


def raw_pair_sums(lib, logits, tbits, flags, bit, t, short=0, q=None, prefill=None, null=None):
    """pm_pair_sums with a scratch of exactly the declared size (minus `short`) and a canary behind it -> (outputs, rc)."""
    n, q_real = logits.shape
    q = q_real if q is None else q
    d = logits.device
    need = lib.workspace_bytes(n, q_real, min(t, 128))
    ws = torch.empty(need + GUARD, dtype=torch.uint8, device=d)
    ws[need:] = 0x5A
    fill = 0.0 if prefill is None else prefill
    outs = [torch.full((q_real, min(t, 128)), fill, device=d), torch.full((q_real, min(t, 128)), fill, device=d),
            torch.full((q_real, min(t, 128), 3), fill, device=d), torch.full((1,), 77, dtype=torch.int32, device=d)]
    args = [logits, tbits, flags]
    ptrs = [_p(a) for a in args] + [bit, n, q, t] + [_p(o) for o in outs]
    if null is not None:
        ptrs[null] = None
    rc = lib.lib.pm_pair_sums(*ptrs, ws.data_ptr(), need - short, _stream(d))
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0x5A).all()), "pm_pair_sums wrote past its declared workspace"
    return outs, rc


@pytest.mark.parametrize("pattern", mc.PATTERNS)
@pytest.mark.parametrize("shape", mc.SHAPES, ids=lambda s: "Q%d_T%d_N%d" % s)
def test_hip_sums_losses_and_gradient_against_fp64(dev, shape, pattern):
    mc.check_precision(dev, mref.PM_M, "hip", shape, pattern)


@pytest.mark.parametrize("pattern", mc.PATTERNS)
@pytest.mark.parametrize("shape", [s for s in mc.SHAPES if s[1] >= 1], ids=lambda s: "Q%d_T%d_N%d" % s)
def test_hip_assignment_is_near_optimal_under_the_fp64_cost(dev, shape, pattern):
    mc.check_assignment(dev, mref.PM_M, "hip", shape, pattern)


def test_hip_indices_equal_the_fp64_optimum_on_the_seeded_cases(dev):
    mc.check_indices_equal(dev, mref.PM_M, "hip")


def test_hip_garbage_bits_beyond_t_change_nothing(dev):
    mc.check_garbage_bits(dev)


@pytest.mark.parametrize("t,with_unknown,n_outside", [(1, True, 0), (3, False, 0), (33, True, 6), (128, True, 3)])
def test_hip_target_pack_equals_a_numpy_gather(dev, t, with_unknown, n_outside):
    mc.check_target_pack(dev, t, with_unknown, n_outside)


@pytest.mark.parametrize("shape", mc.REPEAT_SHAPES, ids=["one_range", "multi_range", "three_target_tiles", "grown_ranges"])
def test_hip_two_calls_return_the_same_bits_within_the_declared_workspace(lib, dev, shape):
    from pasco_amd.grad.matchlib import geometry
    Q, T, N = shape
    assert geometry(N, Q, T)["ranges"] == lib.ranges(N, Q, T) == {(33, 33, 63): 1, mc.MULTI: 3, (5, 65, 129): 2, (7, 3, 32769): 205}[shape]
    x = mc.inputs(shape, "sparse")
    logits, tbits, flags = x.logits.to(dev), x.tbits.to(dev), x.flags.to(dev)
    for bit in (0, 1):
        a, rc = raw_pair_sums(lib, logits, tbits, flags, bit, T)
        assert rc == 0, lib.lib.pm_last_error()
        b, rc = raw_pair_sums(lib, logits, tbits, flags, bit, T)
        assert rc == 0
        for s, t_ in zip(a, b):
            assert torch.equal(s, t_)
        via = lib.pair_sums(logits, tbits, flags, bit, T)
        for s, t_ in zip(a, via):
            assert torch.equal(s, t_), "the binding's workspace table gives the same bits"
    tq = torch.full((Q,), -1, dtype=torch.int32)
    tq[x.optimum[0]] = x.optimum[1].to(torch.int32)
    coef = torch.randn(Q, 3, generator=torch.Generator().manual_seed(3))
    a = lib.mask_loss_bwd(logits, tbits, flags, tq.to(dev), coef.to(dev), T)
    b = lib.mask_loss_bwd(logits, tbits, flags, tq.to(dev), coef.to(dev), T)
    assert torch.equal(a, b)


def test_hip_refusals_launch_nothing(lib, dev):
    x = mc.inputs((33, 33, 63), "sparse")
    Q, T, N = x.shape
    logits, tbits, flags = x.logits.to(dev), x.tbits.to(dev), x.flags.to(dev)

    def untouched(outs):
        return all(bool((o == PATTERN).all()) for o in outs[:3]) and int(outs[3]) == 77

    def err():
        return lib.lib.pm_last_error().decode()

    outs, rc = raw_pair_sums(lib, logits, tbits, flags, 0, T, short=1, prefill=PATTERN)
    assert rc != 0 and "workspace" in err() and untouched(outs)
    outs, rc = raw_pair_sums(lib, logits, tbits, flags, 0, T, q=129, prefill=PATTERN)
    assert rc != 0 and "129 queries" in err() and untouched(outs)
    outs, rc = raw_pair_sums(lib, logits, tbits, flags, 0, 129, prefill=PATTERN)
    assert rc != 0 and "129 targets" in err() and untouched(outs)
    outs, rc = raw_pair_sums(lib, logits, tbits, flags, 2, T, prefill=PATTERN)
    assert rc != 0 and "flag_bit" in err() and untouched(outs)
    for null in (0, 1, 2, 7, 8, 9, 10):                # logits, tbits, flags, focal_sum, dice, stats, count
        outs, rc = raw_pair_sums(lib, logits, tbits, flags, 0, T, prefill=PATTERN, null=null)
        kept = [o for i, o in enumerate(outs) if 7 + i != null]
        assert rc != 0 and "null" in err(), null
        assert all(bool((o == (PATTERN if o.dtype != torch.int32 else 77)).all()) for o in kept), null

    # pm_mask_loss_bwd
    tq = torch.zeros(Q, dtype=torch.int32, device=dev)
    coef = torch.ones(Q, 3, device=dev)
    dl = torch.full_like(logits, PATTERN)
    args = [logits, tbits, flags, tq, coef]
    for q_, t_, text in ((129, T, "129 queries"), (Q, 129, "129 targets")):
        rc = lib.lib.pm_mask_loss_bwd(*[_p(a) for a in args], N, q_, t_, _p(dl), _stream(dev))
        torch.cuda.synchronize()
        assert rc != 0 and text in err() and bool((dl == PATTERN).all())
    for null in range(6):
        ptrs = [_p(a) for a in args] + [N, Q, T, _p(dl)]
        ptrs[null if null < 5 else 8] = None
        rc = lib.lib.pm_mask_loss_bwd(*ptrs, _stream(dev))
        torch.cuda.synchronize()
        assert rc != 0 and "null" in err() and bool((dl == PATTERN).all()), null

    # pm_target_pack
    masks, unknown, coords, _ = mc.pack_case(3)
    masks, coords = masks.to(dev), coords.to(dev)
    n = coords.shape[0]
    tb = torch.full((n, 4), 5, dtype=torch.int32, device=dev)
    fl = torch.full((n,), 5, dtype=torch.uint8, device=dev)
    oob = torch.full((1,), 5, dtype=torch.int32, device=dev)

    def pack(masks_p, coords_p, t, tb_p, fl_p, oob_p):
        rc = lib.lib.pm_target_pack(masks_p, None, coords_p, n, t, 5, 6, 7, 0, 0, 0, tb_p, fl_p, oob_p, _stream(dev))
        torch.cuda.synchronize()
        return rc

    assert pack(_p(masks), _p(coords), 129, _p(tb), _p(fl), _p(oob)) != 0 and "129 targets" in err()
    for i in range(5):
        ptrs = [_p(masks), _p(coords), 3, _p(tb), _p(fl), _p(oob)]
        ptrs[i if i < 2 else i + 1] = None
        assert pack(*ptrs) != 0 and "null" in err(), i
    assert bool((tb == 5).all()) and bool((fl == 5).all()) and int(oob) == 5


@pytest.mark.parametrize("scene", mc.GOLDEN_SCENES)
def test_hip_criterion_against_the_recorded_reference(dev, scene):
    mc.check_golden(dev, mref.PM_M, "hip", scene)


def test_hip_criterion_state_dict_and_ssc_terms(dev):
    mc.check_state_dict_and_ssc(dev)


def test_hip_matcher_loss_and_backward_hold_no_row_by_query_temporary(hip, lib, dev):
    """Q = 100, T = 30, N = 20 000: one [N, Q] fp32 tensor is 8 MB.  Across the forward (matcher + loss) the peak of
    torch.cuda.max_memory_allocated rises over the level before by at most the [Q, T] outputs of the two pair_sums calls, the
    declared workspace and 1 MiB (the words and flags are made before, once per batch element: they are counted with the
    packing, which this test also bounds); across backward() by at most the dlogits bytes, the workspace and 1 MiB.  The cache
    is emptied and then given one large free block before each level is taken, so that every request is split off it at its own
    size (as test_hip_backward_memory_has_no_score_tensor does)."""
    from pasco_amd.grad import criterion as crit
    Q, T, N = 100, 30, 20000
    g = torch.Generator(device=dev).manual_seed(20000)
    logits = torch.randn(N, Q, device=dev, generator=g).requires_grad_(True)
    dims = (64, 64, 8)
    masks = (torch.randint(0, T + 3, dims, device=dev, generator=g)[None] == torch.arange(T, device=dev)[:, None, None, None]).to(torch.uint8)
    unknown = (torch.rand(dims, device=dev, generator=g) < 0.1).to(torch.uint8)
    pick = torch.randperm(dims[0] * dims[1] * dims[2], device=dev, generator=g)[:N]
    coords = torch.stack([torch.zeros_like(pick), pick // (dims[1] * dims[2]), (pick // dims[2]) % dims[1], pick % dims[2]], dim=1).to(torch.int32)
    query_logits = torch.randn(Q, 21, device=dev, generator=g)
    labels = torch.randint(0, 20, (T,), device=dev, generator=g)
    class_weights = torch.rand(21, device=dev, generator=g) + 0.5
    ws = lib.workspace_bytes(N, Q, T)
    lib.pair_sums(logits.detach(), torch.zeros(N, 4, dtype=torch.int32, device=dev), torch.zeros(N, dtype=torch.uint8, device=dev), 0, T)
    matcher = crit.HungarianMatcher()

    def level():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        block = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
        del block
        torch.cuda.reset_peak_memory_stats(dev)
        return torch.cuda.memory_allocated(dev)

    before = level()
    packed = crit.pack_targets(masks, unknown, coords)
    torch.cuda.synchronize()
    rise_pack = torch.cuda.max_memory_allocated(dev) - before
    words = 16 * N + N + 4

    before = level()
    src, tgt = matcher.match_packed(logits, query_logits, labels, class_weights, packed)
    lm, ld = crit.mask_losses(logits, packed, src, tgt, class_weights[labels[tgt.to(dev)]])
    loss = lm.mean() + ld.mean()
    torch.cuda.synchronize()
    rise_fwd = torch.cuda.max_memory_allocated(dev) - before
    qt = 2 * (5 * 4 * Q * T + 4)

    before = level()
    loss.backward()
    torch.cuda.synchronize()
    rise_bwd = torch.cuda.max_memory_allocated(dev) - before
    print(f"PM_MEMORY pack {rise_pack} (words and flags {words}); forward {rise_fwd} ([Q,T] outputs {qt}, workspace {ws}); "
          f"backward {rise_bwd} (dlogits {4 * N * Q}); one [N, Q] tensor {4 * N * Q}")
    assert rise_pack <= words + (1 << 20)
    assert rise_fwd <= words + qt + ws + (1 << 20)
    assert rise_fwd < 4 * N * Q, "the forward holds less than one [N, Q] tensor"
    assert rise_bwd <= 4 * N * Q + ws + (1 << 20)
    assert bool(torch.isfinite(logits.grad).all()) and bool(logits.grad.any())
