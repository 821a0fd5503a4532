"""`pasco_amd.grad.optim.AdamW` on the GPU: the po_* kernels of libpascohip.so (include/pasco_optim.h).  The checks are
tests/optim_cases.py (shared with tests/test_optim_cpu.py), the references tests/optim_ref64.py: the fp64 torch twin, torch's
own fp32 clip + AdamW on the same GPU as the yardstick of the error, and the host restatement, which the update has to equal
bit for bit.  The short case is nine tensors and a dozen chunks; the two long ones pass the grid cap of the table kernels."""
import os
import re

import pytest
import torch

import pasco_amd.me as ME
from pasco_amd.grad import host
from pasco_amd.grad.optim import AdamW
from tests import optim_cases as oc
from tests import optim_ref64 as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def test_binding_mirrors_the_header(dev):
    from pasco_amd.grad import optimlib
    lib = optimlib.optim_lib()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pasco_optim.h")).read()
    const = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert const("PO_ABI_VERSION") == optimlib.PO_ABI_VERSION == lib.lib.po_abi_version()
    assert const("PO_CHUNK") == optimlib.PO_CHUNK == host.OPTIM_CHUNK
    assert const("PO_MAX_GROUPS") == optimlib.PO_MAX_GROUPS


def test_ranges_are_refused_with_a_message(dev):
    """The limits of the header, at the entry points themselves: nothing is launched."""
    from pasco_amd.grad import optimlib
    lib = optimlib.optim_lib()
    lib.table_check(0, 0, 0, 1)
    lib.table_check(5, 2 ** 31 - 1, 2 ** 40 - 1, optimlib.PO_MAX_GROUPS)
    for args, text in (((5, 2 ** 31, 2 ** 31, 1), "fewer than 2\\^31 per tensor"), ((5, 7, 2 ** 40, 1), "fewer than 2\\^40"),
                       ((-1, 0, 0, 1), "tensors"), ((1, 1, 1, optimlib.PO_MAX_GROUPS + 1), "PO_MAX_GROUPS"), ((1, 1, 1, 0), "PO_MAX_GROUPS")):
        with pytest.raises(RuntimeError, match="po_table_check: table_check: .*" + text):
            lib.table_check(*args)
    rec = torch.zeros(3, dtype=torch.float64, device=dev)
    step = torch.zeros(2, dtype=torch.int32, device=dev)
    hyper = [(1e-3, 0.9, 0.999, 1e-8, 0.0)]
    with pytest.raises(RuntimeError, match="policy = 7"):
        lib.prepare(None, 0, None, 0, hyper, 0.5, 1.0, 7, None, None, rec, step)
    with pytest.raises(RuntimeError, match="grad_scale"):
        lib.prepare(None, 0, None, 0, hyper, 0.5, 0.0, 0, None, None, rec, step)
    with pytest.raises(RuntimeError, match="T = -1"):
        lib.prepare(None, -1, None, 0, hyper, 0.5, 1.0, 0, None, None, rec, step)
    with pytest.raises(ValueError, match="PO_MAX_GROUPS"):
        lib.prepare(None, 0, None, 0, hyper * 9, 0.5, 1.0, 0, None, None, rec, step)
    with pytest.raises(RuntimeError, match="chunks without a table"):
        lib.adamw(None, 0, None, 3, None, step)
    lib.prepare(None, 0, None, 0, hyper, 0.5, 1.0, 0, None, None, rec, step)       # an empty table is served: norm 0, s = 1
    assert rec.tolist() == [0.0, 0.0, 0.0] and step.tolist()[1] == 1 and float(step.view(torch.float32)[0]) == 1.0


@pytest.mark.parametrize("max_norm", [oc.CLIP, oc.NO_CLIP], ids=["clip_acts", "clip_idle"])
def test_three_steps_against_the_fp64_twin(dev, max_norm):
    oc.check_accuracy(dev, max_norm)


def test_sum_of_squares_and_equal_bits_on_a_repeat(dev):
    oc.check_norm(dev)


def test_grad_scale(dev):
    oc.check_grad_scale(dev)


@pytest.mark.parametrize("max_norm", [oc.CLIP, None], ids=["clip_acts", "no_clip"])
def test_update_equals_the_restatement_bit_for_bit(dev, max_norm):
    """Three steps on the device - one tensor getting its first gradient at the third; after each the sum of squares is read
    from the result record, the clip scale formed from it on the host by the same fp64 expression, and the restatement run
    on the host: p, m and v have to be the same bits (every operation is a correctly rounded fp32 one, contraction off), and so
    do the fp32 scalars and the state records po_prepare wrote."""
    values, grads = oc.case_values()
    steps = [(lr, [None if (i == 2 and k < 2) else g for i, g in enumerate(gs)]) for k, (lr, gs) in enumerate(zip(oc.LRS, grads))]
    ps = oc.make_params(values, dev)
    opt = oc.make_optimizer(ps, max_norm=max_norm)
    sums = []
    for lr, gs in steps:
        oc.set_lr(opt, lr), oc.set_grads(ps, gs, dev), opt.step()
        sums.append(float(opt.sum_of_squares))
        norm, s = host.optim_clip(sums[-1], 0.0 if max_norm is None else max_norm, 1.0)
        assert float(opt.grad_norm) == norm and float(opt._buffers().step.view(torch.float32)[0]) == s
    want = oc.restate_steps(values, steps, max_norm, sums)
    got = oc.our_state(ps, opt)
    report = []
    for k in ref.QUANTITIES:
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            diff = int((a.cpu().view(torch.int32) != b.view(torch.int32)).sum())
            if diff:
                report.append(f"{k} of tensor {i} ({a.numel()} elements): {diff} differ, max {float((a.cpu() - b).abs().max()):.3e}")
    print(f"[optim] kernel against restatement, max_norm = {max_norm}: {len(report)} of {3 * len(ps)} tensors differ")
    assert not report, "\n".join(report)
    records = oc.our_records(ps, opt)
    assert records["step"].tolist() == [3, 3, 1] + [3] * 6
    wd = {i: w for idx, w in oc.GROUPS for i in idx}
    scalars = opt._buffers().scalars.cpu()
    for i, at in enumerate(oc.slots(ps, opt)):
        b1p, b2p = 1.0, 1.0
        for _ in range(int(records["step"][i])):
            b1p, b2p = b1p * oc.BETAS[0], b2p * oc.BETAS[1]
        assert (records["beta1_pow"][i], records["beta2_pow"][i]) == (b1p, b2p)
        k = host.optim_scalars(oc.LRS[2], oc.BETAS[0], oc.BETAS[1], oc.EPS, wd[i], b1p, b2p)
        assert torch.equal(scalars[at].view(torch.int32), k.view(torch.int32)), (i, scalars[at].tolist(), k.tolist())


@pytest.mark.parametrize("name", list(oc.LONG_CASES))
def test_more_chunks_than_the_grid_and_more_tensors_than_a_workgroup(dev, name):
    """The cases of tests/optim_cases.py in which a workgroup of k_sqnorm / k_adamw takes a second chunk (of another tensor, or
    of the same one) and both loops of k_prepare take several trips: the checks of the shared table, then p, m, v, the state
    records and the fp32 scalars against the host restatement, bit for bit, under the case's own groups."""
    case, ps, opt, sums = oc.check_long(dev, name)
    values, steps = case.values()
    for sumsq in sums[-1:]:
        norm, s = host.optim_clip(sumsq, oc.CLIP, 1.0)
        assert float(opt.grad_norm) == norm and float(opt._buffers().step.view(torch.float32)[0]) == s
    want = oc.restate_steps(values, steps, oc.CLIP, sums, case.groups)
    got = oc.our_state(ps, opt)
    report = []
    for k in ref.QUANTITIES:
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            diff = int((a.cpu().view(torch.int32) != b.view(torch.int32)).sum())
            if diff:
                report.append(f"{k} of tensor {i} ({a.numel()} elements): {diff} differ, max {float((a.cpu() - b).abs().max()):.3e}")
    print(f"[optim] {name}: kernel against restatement: {len(report)} of {3 * len(ps)} tensors differ")
    assert not report, "\n".join(report[:20])
    records = oc.our_records(ps, opt)
    b1p, b2p = 1.0, 1.0
    for _ in range(case.n_steps):
        b1p, b2p = b1p * oc.BETAS[0], b2p * oc.BETAS[1]
    assert records["step"].tolist() == [case.n_steps] * len(ps)
    assert set(records["beta1_pow"].tolist()) == {b1p} and set(records["beta2_pow"].tolist()) == {b2p}
    wd = {i: w for idx, w in case.groups for i in idx}
    scalars = opt._buffers().scalars.cpu().view(torch.int32)
    lr = steps[-1][0]
    k_of = {w: host.optim_scalars(lr, oc.BETAS[0], oc.BETAS[1], oc.EPS, w, b1p, b2p).view(torch.int32) for w in set(wd.values())}
    for i, at in enumerate(oc.slots(ps, opt)):
        assert torch.equal(scalars[at], k_of[wd[i]]), (i, scalars[at].tolist(), k_of[wd[i]].tolist())


def test_first_gradient_at_the_third_step(dev):
    oc.check_late_gradient(dev)


def test_nonfinite_propagates_like_torch(dev):
    oc.check_nonfinite_propagate(dev)


def test_nonfinite_skipped(dev):
    oc.check_nonfinite_skip(dev)


def test_state_dict_round_trips_with_torch(dev):
    oc.check_state_dict_round_trips(dev)


def test_versions_move_with_the_step(dev):
    oc.check_versions(dev)


def test_refusals(dev):
    oc.check_refusals(dev)


def test_non_contiguous_gradient_and_a_late_group(dev):
    oc.check_non_contiguous_gradient(dev)


def test_lambda_lr_drives_it(dev):
    oc.check_scheduler_drives_it(dev)


def test_a_warm_convolution_sees_the_step(dev):
    """the module keeps the split of its kernel while the kernel's version counter stands.  The kernels write the
    weights through raw pointers; `step()` moves the counters, so the next forward is that of a cold module built from the
    stepped weights."""
    from tests.grad_cases import make_map, make_module
    m = make_map("same", dev)
    torch.manual_seed(7)
    mod = make_module("same", 32, 32).to(dev).eval()
    g = torch.Generator().manual_seed(8)
    feats = torch.randn(m["n_in"], 32, generator=g).to(dev)

    def forward(module):
        with torch.no_grad():
            return module(ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])).F.clone()

    warm = forward(mod)
    assert "_ph_me_split" in mod.__dict__, "the forward kept no split kernel: this test would show nothing"
    opt = AdamW(mod.parameters(), lr=1e-2, max_norm=0.5)
    for p in mod.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(dev)
    opt.step()
    stepped = forward(mod)
    cold = make_module("same", 32, 32).to(dev).eval()
    cold.load_state_dict({k: v.clone() for k, v in mod.state_dict().items()})
    assert "_ph_me_split" not in cold.__dict__
    want = forward(cold)
    assert not torch.equal(stepped, warm)
    assert torch.equal(stepped, want), f"a warm module differs from a cold one by {float((stepped - want).abs().max()):.3e}"


def test_stack_trains_for_five_steps(dev):
    """`Stack` of tests/grad_cases.py: five steps of forward, backward and `AdamW(max_norm=0.5).step()`, and the same with
    `clip_grad_norm_` + torch's fp32 AdamW from the same weights.  The loss is finite and lower at the end; the two sets of
    weights stay within the recorded difference (a smoke bound between two fp32 paths)."""
    from tests.grad_cases import Stack, box_coords
    coords = box_coords(5).to(dev)
    g = torch.Generator().manual_seed(11)
    feats = torch.randn(coords.shape[0], 3, generator=g).to(dev)
    torch.manual_seed(3)
    nets = [Stack().to(dev).train() for _ in range(2)]
    nets[1].load_state_dict(nets[0].state_dict())
    opts = [AdamW(nets[0].parameters(), lr=3e-3, weight_decay=0.01, max_norm=0.5),
            torch.optim.AdamW(nets[1].parameters(), lr=3e-3, weight_decay=0.01, foreach=False)]
    tgt, losses = None, ([], [])
    for step in range(5):
        for which, (net, opt) in enumerate(zip(nets, opts)):
            out = net(ME.SparseTensor(feats, coords))
            if tgt is None:
                tgt = torch.randn(out.F.shape, generator=g).to(dev)
            loss = (out.F - tgt).square().mean()
            opt.zero_grad()
            loss.backward()
            if which == 1:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5, foreach=False)
            opt.step()
            losses[which].append(float(loss.detach()))
    ours = losses[0]
    assert all(torch.isfinite(torch.tensor(ours))) and ours[-1] < ours[0], ours
    diff = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(nets[0].parameters(), nets[1].parameters()))
    print(f"[optim] Stack, five steps: loss {ours[0]:.6f} -> {ours[-1]:.6f} (torch's {losses[1][-1]:.6f}); largest parameter "
          f"difference {diff:.3e}, bound {ref.STACK_DIFF:.3e}")
    assert diff <= ref.STACK_DIFF
