"""The semantic completion loss kernels (pasco_amd/csrc/semloss.hip) on the MI355X against tests/sem_ref64.py, stage by stage:
rows and keys, the radix sort against numpy's stable order, the increments, values and gradients; the declared workspace and
its canary, refusals that launch nothing, repeated calls, the drop-in functions, the memory a forward takes.  The CPU side is
tests/test_semloss_cpu.py."""
import pytest
import torch

from tests import sem_cases as sc
from tests import sem_ref64 as sref
from tests import test_semloss_cpu as cpu

pytestmark = pytest.mark.gpu

GUARD = 4096


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


@pytest.fixture(scope="module")
def lib(hip):
    from pasco_amd.grad.semlib import sem_lib
    return sem_lib()


@pytest.fixture(scope="module")
def dev(hip):
    return torch.device("cuda", 0)


@pytest.mark.parametrize("shape,pattern", sc.CASES, ids=sc.CASE_IDS)
def test_hip_stages_values_and_gradients_against_fp64(hip, shape, pattern):
    sc.check_case("hip", sref.PS_M, shape, pattern)


@pytest.mark.parametrize("kind", cpu.SORT_KEYS)
@pytest.mark.parametrize("s", [1, 3, 32])
def test_hip_sort_is_numpys_stable_descending_order(lib, dev, kind, s):
    """No tolerance: a broken histogram, scan, rank or scatter cannot pass.  The scratch has exactly the declared bytes and a
    canary behind it; perm has a canary too."""
    T = sc.T
    for m in (1, 2, 63, 64, 65, 511, 513, T - 1, T, T + 1, 3 * T + 1) + ((sc.LONG_SHAPES[0][0],) if s == 3 else ()):      # 33 tiles
        keys = cpu.sort_keys(kind, s, m)
        need = lib.sort_workspace_bytes(s, m)
        ws = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
        perm = torch.full((s * m + 64,), -7, dtype=torch.int32, device=dev)
        kd = keys.to(dev)
        rc = lib.lib.ps_sort_desc(kd.data_ptr(), s, m, perm.data_ptr(), ws.data_ptr(), need, _stream(dev))
        torch.cuda.synchronize()
        assert rc == 0, lib.lib.ps_last_error()
        assert bool((ws[need:] == 0x5A).all()) and bool((perm[s * m:] == -7).all()), "ps_sort_desc wrote past its buffers"
        assert torch.equal(perm[:s * m].cpu().reshape(s, m), sc.stable_desc(keys)), (kind, s, m)


def test_hip_edges(hip):
    cpu.check_edges("hip")


def test_hip_dropins_mean_over_the_surviving_pairs(hip):
    cpu.check_dropin("hip", sref.PS_M)


def test_hip_head_receives_its_kernel_gradient(hip):
    cpu.check_head_gradient("hip", sref.PS_M)


def _forward_raw(lib, dev, case, ws_short=0, c_arg=None):
    """The three entry points on a scratch of exactly the declared bytes with a canary behind it -> (outputs, return codes)."""
    n, c = case["n"], case["c"]
    g = lib.geometry(n, c)
    ws = torch.full((g["workspace_bytes"] + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
    keys, perm, ws_sort, ws_rows, ws_lov = lib.parts(ws, n, c, g)
    box = torch.cat([case["min_C"], case["max_C"]]).to(device=dev, dtype=torch.int32)
    F, C, tgt, w = (case[k].to(dev) for k in ("logits", "coords", "target", "weights"))
    label = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    ce = torch.full((3,), 7.0, device=dev)
    cc = torch.full((c,), 77, dtype=torch.int32, device=dev)
    info = torch.full((4,), 77, dtype=torch.int32, device=dev)
    loss_c = torch.full((c,), 7.0, device=dev)
    coef = torch.full((n, c), 7.0, device=dev)
    lov = torch.full((1,), 7.0, device=dev)
    present = torch.full((1,), 77, dtype=torch.int32, device=dev)
    dl = torch.full((n, c), 7.0, device=dev)
    gg = torch.ones(2, device=dev)
    cq = c if c_arg is None else c_arg
    dx, dy, dz = case["target"].shape
    st = _stream(dev)
    refuse = bool(ws_short) or c_arg is not None      # then every call below is expected to be refused before it launches
    rcs = [lib.lib.ps_rows_fwd(F.data_ptr(), C.data_ptr(), tgt.data_ptr(), box.data_ptr(), case["scale"], w.data_ptr(), n, cq, dx, dy,
                               dz, label.data_ptr(), ce.data_ptr(), cc.data_ptr(), info.data_ptr(), keys.data_ptr(),
                               ws_rows.data_ptr(), g["rows_bytes"] - ws_short, st)]
    rcs.append(None if refuse else lib.lib.ps_sort_desc(keys.data_ptr(), c, n, perm.data_ptr(), ws_sort.data_ptr(),
                                                        g["sort_bytes"], st))
    rcs.append(lib.lib.ps_lovasz_fwd(perm.data_ptr(), label.data_ptr(), keys.data_ptr(), cc.data_ptr(), n, cq, loss_c.data_ptr(),
                                     coef.data_ptr(), lov.data_ptr(), present.data_ptr(), ws_lov.data_ptr(),
                                     g["lovasz_bytes"] - ws_short, st))
    rcs.append(None if ws_short else lib.lib.ps_loss_bwd(F.data_ptr(), label.data_ptr(), coef.data_ptr(), w.data_ptr(),
                                                         ce.data_ptr(), present.data_ptr(), gg.data_ptr(), n, cq, dl.data_ptr(), st))
    torch.cuda.synchronize()
    assert bool((ws[g["workspace_bytes"]:] == 0x5A).all()), "a stage wrote past the declared workspace"
    outs = {"label": label, "ce": ce, "class_count": cc, "info": info, "loss_c": loss_c, "coef": coef, "lovasz": lov,
            "present": present, "dlogits": dl, "keys": keys.clone(), "perm": perm.clone()}
    return {k: v.cpu() for k, v in outs.items()}, rcs


@pytest.mark.parametrize("shape", [(65, 20), (3 * sc.T + 1, 20), sc.LONG_SHAPES[0]], ids=lambda s: "N%d_C%d" % s)
def test_hip_declared_workspace_canary_and_repeatability(lib, dev, shape):
    """Exactly the declared bytes are enough, nothing is written behind them, and two calls give the same bits: one range,
    several, and ranges of two rows per thread over 33 tiles."""
    case = sc.make_case(shape, "ignore10", scale=2)
    a, rcs = _forward_raw(lib, dev, case)
    assert rcs == [0, 0, 0, 0], lib.lib.ps_last_error()
    b, _ = _forward_raw(lib, dev, case)
    for k in a:
        assert torch.equal(a[k], b[k]) or (k == "ce" and torch.equal(torch.isnan(a[k]), torch.isnan(b[k]))), k
    ref = sc.run_stages("hip", case)
    for k in ("label", "ce", "class_count", "loss_c", "coef", "lovasz", "present", "keys", "perm"):
        assert torch.equal(a[k], ref[k]), k
    assert bool(a["dlogits"].any()) and not bool((a["dlogits"] == 7.0).any())


def test_hip_refusals_leave_prefilled_outputs_untouched(lib, dev):
    case = sc.make_case((65, 20), "random", scale=1)
    for kw, text in ((dict(ws_short=4), b"workspace"), (dict(c_arg=33), b"33 classes")):
        out, rcs = _forward_raw(lib, dev, case, **kw)
        assert rcs[0] != 0 and rcs[2] != 0 and text in lib.lib.ps_last_error(), (rcs, lib.lib.ps_last_error())
        if "c_arg" in kw:
            assert rcs[3] != 0
            assert bool((out["dlogits"] == 7.0).all())
        assert bool((out["label"] == 77).all()) and bool((out["ce"] == 7.0).all()) and bool((out["class_count"] == 77).all())
        assert bool((out["info"] == 77).all()) and bool((out["loss_c"] == 7.0).all()) and bool((out["coef"] == 7.0).all())
        assert bool((out["lovasz"] == 7.0).all()) and bool((out["present"] == 77).all())
    n = 65
    perm = torch.full((n,), -7, dtype=torch.int32, device=dev)
    keys = torch.zeros(n, dtype=torch.int32, device=dev)
    ws = torch.zeros(lib.sort_workspace_bytes(1, n), dtype=torch.uint8, device=dev)
    for args in ((0, n, ws.numel()), (65536, n, ws.numel()), (1, (1 << 24) + 1, ws.numel()), (1, n, ws.numel() - 4)):
        rc = lib.lib.ps_sort_desc(keys.data_ptr(), args[0], args[1], perm.data_ptr(), ws.data_ptr(), args[2], _stream(dev))
        torch.cuda.synchronize()
        assert rc != 0 and bool((perm == -7).all()), args


def test_hip_forward_memory_is_the_declared_workspace(lib, dev):
    """At N = 20 000, C = 20 the forward's peak above its inputs is at most the declared workspace + coef (4 N C) + label (N) +
    1 MiB of small tensors, from the allocator's counters (as the pm_ memory test does); the backward adds dlogits."""
    from pasco_amd.grad.semloss import sem_compl_loss
    from pasco_amd.me.backend import hip_backend
    N, C = 20000, 20
    g = torch.Generator(device=dev).manual_seed(20000)
    dims = (64, 64, 8)
    F = torch.randn(N, C, device=dev, generator=g).requires_grad_(True)
    target = torch.randint(0, C, dims, device=dev, generator=g).to(torch.uint8)
    target[torch.rand(dims, device=dev, generator=g) < 0.1] = 255
    pick = torch.randperm(dims[0] * dims[1] * dims[2], device=dev, generator=g)[:N]
    coords = torch.stack([torch.zeros_like(pick), pick // (dims[1] * dims[2]), (pick // dims[2]) % dims[1], pick % dims[2]], dim=1).to(torch.int32)
    min_C, max_C = torch.zeros(3, dtype=torch.int32, device=dev), torch.tensor([62, 63, 7], dtype=torch.int32, device=dev)
    w = torch.rand(C, device=dev, generator=g) + 0.5
    need = lib.workspace_bytes(N, C)
    be = hip_backend()
    be.scratch.drop("semloss")

    def level():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        block = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
        del block
        torch.cuda.reset_peak_memory_stats(dev)
        return torch.cuda.memory_allocated(dev)

    before = level()
    ce, lov = sem_compl_loss(F, coords, target, min_C, max_C, 1, w)
    torch.cuda.synchronize()
    rise_fwd = torch.cuda.max_memory_allocated(dev) - before
    before = level()
    (ce + lov).backward()
    torch.cuda.synchronize()
    rise_bwd = torch.cuda.max_memory_allocated(dev) - before
    print(f"PS_MEMORY forward {rise_fwd} (workspace {need}, coef {4 * N * C}, label {N}); backward {rise_bwd} (dlogits {4 * N * C})")
    assert rise_fwd <= need + 4 * N * C + N + (1 << 20)
    assert rise_bwd <= 4 * N * C + (1 << 20)
    assert bool(torch.isfinite(F.grad).all()) and bool(F.grad.any())


@pytest.mark.parametrize("name", cpu.GOLDEN)
def test_hip_recorded_reference_scenes(hip, name):
    cpu.check_golden("hip", sref.PS_M, name)
