"""Test helper: the cases and checks of `pasco_amd.grad.optim.AdamW`, shared by tests/test_optim_cpu.py (the host restatement)
and tests/test_hip_optim.py (the po_* kernels).  References and bounds: tests/optim_ref64.py.

One case is a handful of tensors in two parameter groups (with and without weight decay): 1, 3, 4, 5, PO_CHUNK - 1, PO_CHUNK,
PO_CHUNK + 1 and 3 PO_CHUNK + 5 elements - a lone element, the ragged quads, one chunk short of, at and past its end, several
chunks with a ragged last one - plus a parameter and a gradient that are views one element into their storage, whose addresses
are 4 bytes past a 16-byte boundary and force the 4-byte accesses."""
import math

import torch

from pasco_amd.grad import host
from pasco_amd.grad.optim import AdamW
from pasco_amd.grad.optimlib import PO_CHUNK
from tests import optim_ref64 as ref

SIZES = (1, 3, 4, 5, PO_CHUNK - 1, PO_CHUNK, PO_CHUNK + 1, 3 * PO_CHUNK + 5)
OFFSET_SHAPE = (293, 7)            # the views at storage offset 1 (2-d: several quads and a ragged end)
DECAY, NO_DECAY = 0.1, 0.0
BETAS, EPS = (0.9, 0.999), 1e-8
LRS = (1e-3, 5e-4, 2e-3)             # the schedule moves the learning rate between the steps
CLIP, NO_CLIP = 0.5, 1e9             # the reference's gradient_clip_val; a max_norm too large to act


def offset_view(t: torch.Tensor) -> torch.Tensor:
    """The same values as a contiguous view one element into a flat buffer."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.storage_offset() == 1 and out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def case_values(n_steps: int = 3, seed: int = 0):
    """-> (initial parameter values, [gradient values per step]) on the host: the SIZES, then the offset tensor (a 2-d one)."""
    g = torch.Generator().manual_seed(seed)
    shapes = [(n,) for n in SIZES] + [OFFSET_SHAPE]
    params = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) * (0.03 * (1 + i % 4)) for i, s in enumerate(shapes)] for _ in range(n_steps)]
    return params, grads


GROUPS = ([0, 2, 4, 6, 8], DECAY), ([1, 3, 5, 7], NO_DECAY)      # indices into the case's tensors


# ---- past the first trip of the loops ----------------------------------------------------------------------------------------
# The case above is 9 tensors and 14 chunks: no workgroup of k_sqnorm / k_adamw takes a second chunk and neither loop of
# k_prepare a second trip.  A net is thousands of tensors and of chunks.
MAX_GRID, BLOCK = 2048, 256                  # csrc/optim.hip: the grid cap of the table kernels, the threads of a workgroup


class LongCase:
    """sizes: the elements of every tensor; even tensors decay, odd ones do not; `n_steps` steps with the clip acting."""

    def __init__(self, name, sizes, n_steps, seed):
        self.name, self.sizes, self.n_steps, self.seed = name, tuple(sizes), n_steps, seed
        self.groups = tuple((idx, wd) for idx, wd in ((list(range(0, len(sizes), 2)), DECAY), (list(range(1, len(sizes), 2)), NO_DECAY))
                            if idx)
        self._values = None

    def values(self):
        """-> (initial parameter values, [(lr, gradient values)] per step) on the host, made once and never written to."""
        if self._values is None:
            g = torch.Generator().manual_seed(self.seed)
            total = sum(self.sizes)
            flat = torch.randn(total, generator=g)
            scale = torch.repeat_interleave(torch.tensor([0.03 * (1 + i % 4) for i in range(len(self.sizes))]), torch.tensor(self.sizes))
            grads = [torch.randn(total, generator=g) * scale for _ in range(self.n_steps)]
            split = lambda t: [x.clone() for x in t.split(self.sizes)]
            self._values = split(flat), [(lr, split(gr)) for lr, gr in zip(LRS, grads)]
        return self._values


LONG_CASES = {c.name: c for c in (
    LongCase("many_tensors", [1 + i % 9 for i in range(2100)] + [3 * PO_CHUNK + 5], 2, 21),
    LongCase("one_long_tensor", [2049 * PO_CHUNK + 3], 1, 22),
)}


# !! `table_geometry` restates the launch arithmetic of pasco_amd/csrc/optim.hip over the chunk table the optimiser uploads (its
# !! tensors group by group).  It is used to CHOOSE the sizes and to assert, at import, that the cases reach the classes below -
# !! never to form an expected value: those come from tests/optim_ref64.py, math.fsum and the host restatement.
def table_geometry(case: LongCase):
    order = [i for idx, _ in case.groups for i in idx]
    tensor_of = [i for i in order for _ in range(-(-case.sizes[i] // PO_CHUNK))]
    C, T = len(tensor_of), len(order)
    grid = min(C, MAX_GRID)
    second = [(tensor_of[b], tensor_of[b + grid]) for b in range(grid) if b + grid < C]
    last = case.sizes[tensor_of[-1]] % PO_CHUNK
    return dict(T=T, C=C, grid=grid, second_trips=len(second), changes_tensor=sum(1 for a, b in second if a != b),
                keeps_tensor=sum(1 for a, b in second if a == b), partial_trips=-(-C // BLOCK), tensor_trips=-(-T // BLOCK),
                last_chunk=last or PO_CHUNK)


def _check_long_cases():
    small = [(n,) for n in SIZES] + [OFFSET_SHAPE]
    assert sum(-(-math.prod(s) // PO_CHUNK) for s in small) < MAX_GRID and len(small) < BLOCK, "the short case: one trip everywhere"
    g = table_geometry(LONG_CASES["many_tensors"])
    assert (g["T"], g["C"]) == (2101, 2104) and g["grid"] == MAX_GRID
    assert g["second_trips"] == g["changes_tensor"] == 56, "a workgroup changes its tensor between two trips"
    assert g["partial_trips"] > 1 and g["tensor_trips"] > 1, "k_prepare: both loops take several trips"
    assert len(LONG_CASES["many_tensors"].groups) == 2 and LONG_CASES["many_tensors"].n_steps == 2
    g = table_geometry(LONG_CASES["one_long_tensor"])
    assert (g["T"], g["C"]) == (1, 2050) and g["second_trips"] == g["keeps_tensor"] == 2, "a second trip that changes the chunk alone"
    assert g["last_chunk"] == 3, "the last chunk is ragged"


_check_long_cases()


def make_params(values, device, offset_last: bool = True):
    if not offset_last:
        return [torch.nn.Parameter(v.to(device).clone()) for v in values]
    ps = [torch.nn.Parameter(v.to(device).clone()) for v in values[:-1]]
    ps.append(torch.nn.Parameter(offset_view(values[-1].to(device))))
    assert ps[-1].storage_offset() == 1 and ps[-1].data_ptr() % 16 == 4
    return ps


def make_optimizer(ps, groups=GROUPS, **kw):
    return AdamW([{"params": [ps[i] for i in idx], "weight_decay": wd} for idx, wd in groups], lr=LRS[0], betas=BETAS, eps=EPS, **kw)


def set_grads(ps, grads, device, offset_last: bool = True):
    for i, (p, g) in enumerate(zip(ps, grads)):
        if g is None:
            p.grad = None
            continue
        g = g.to(device).clone()
        p.grad = offset_view(g) if (offset_last and i == len(ps) - 1) else g


def set_lr(opt, lr):
    for group in opt.param_groups:
        group["lr"] = lr


def slots(ps, opt):
    """The optimiser numbers its parameters group by group: -> for each tensor of the case its index there (the index of its
    moments, of its state record and of its entry in a state dict)."""
    order = {id(p): i for i, p in enumerate(opt._params())}
    return [order[id(p)] for p in ps]


def our_state(ps, opt):
    buf, at = opt._buffers(), slots(ps, opt)
    return {"p": [p.detach().clone() for p in ps], "m": [buf.m[i].clone() for i in at], "v": [buf.v[i].clone() for i in at]}


def our_records(ps, opt):
    """The state records (step, beta1^step, beta2^step) in the order of the case's tensors."""
    return opt._buffers().get_states()[slots(ps, opt)]


def our_run(values, steps, device, groups=GROUPS, offset_last: bool = True, sums=None, **kw):
    """steps: (lr, grads) per step -> (parameters, optimiser) after the last; the sum of squares of every step is appended to
    `sums` where a list is given."""
    ps = make_params(values, device, offset_last)
    opt = make_optimizer(ps, groups, **kw)
    for lr, grads in steps:
        set_lr(opt, lr)
        set_grads(ps, grads, device, offset_last)
        opt.step()
        if sums is not None:
            sums.append(float(opt.sum_of_squares))
    return ps, opt


def bits_equal(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def assert_within(got, v32, v64, what):
    r = ref.ratios(got, v32, v64)
    print(f"[optim] {what}: " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()) + f"  (worst {max(r.values()):.3f})")
    bad = {k: v for k, v in r.items() if not v <= ref.OPT_M}
    assert not bad, f"{what}: ratio over OPT_M = {ref.OPT_M}: {bad}"


def twins(values, steps, max_norm, device, groups=GROUPS):
    """-> (v32 on `device`, v64 on the host)."""
    v32 = ref.twin_run([v.to(device) for v in values], groups, BETAS, EPS, steps, max_norm, torch.float32)
    v64 = ref.twin_run(values, groups, BETAS, EPS, steps, max_norm, torch.float64)
    return v32, v64


# ---- the checks -------------------------------------------------------------------------------------------------------------
def check_accuracy(device, max_norm):
    """Three steps with a changing learning rate against the fp64 twin, relative to torch's own fp32 error."""
    values, grads = case_values()
    steps = list(zip(LRS, grads))
    ps, opt = our_run(values, steps, device, max_norm=max_norm)
    v32, v64 = twins(values, steps, max_norm, device)
    norm = float(opt.grad_norm)
    assert (norm > max_norm) == (max_norm == CLIP), f"the clip is {'not ' if max_norm == CLIP else ''}meant to act: norm {norm}"
    assert_within(our_state(ps, opt), v32, v64, f"3 steps, max_norm = {max_norm:g}, {device}")


def check_norm(device):
    """The summed squares against math.fsum of the exact squares: any order of a sum of n non-negative terms is within
    n 2^-53 of it, relatively.  And a second run gives the same bits, in the record and in every tensor."""
    values, grads = case_values(1)
    runs = [our_run(values, [(LRS[0], grads[0])], device, max_norm=CLIP) for _ in range(2)]
    n = sum(g.numel() for g in grads[0])
    exact = ref.exact_sum_of_squares(grads[0])
    got = float(runs[0][1].sum_of_squares)
    rel = abs(got - exact) / exact
    print(f"[optim] sum of squares over {n} elements: relative error {rel:.3e}, bound {n * 2.0 ** -53:.3e}")
    assert rel <= n * 2.0 ** -53
    assert float(runs[0][1].grad_norm) == math.sqrt(got)
    assert torch.equal(runs[0][1]._buffers().result.view(torch.int64), runs[1][1]._buffers().result.view(torch.int64))
    a, b = our_state(*runs[0]), our_state(*runs[1])
    assert all(bits_equal(a[k], b[k]) for k in ref.QUANTITIES)


def check_grad_scale(device):
    """grad_scale = 1 / 4 on gradients four times as large: the same norm and the same step (scaling by a power of two is
    exact), with and without the clip acting."""
    values, grads = case_values(1)
    for max_norm in (CLIP, NO_CLIP):
        a = our_run(values, [(LRS[0], grads[0])], device, max_norm=max_norm)
        b = our_run(values, [(LRS[0], [4 * g for g in grads[0]])], device, max_norm=max_norm, grad_scale=0.25)
        assert float(a[1].grad_norm) == float(b[1].grad_norm) and float(b[1].sum_of_squares) == 16 * float(a[1].sum_of_squares)
        sa, sb = our_state(*a), our_state(*b)
        assert all(bits_equal(sa[k], sb[k]) for k in ref.QUANTITIES)


def check_late_gradient(device):
    """A parameter without a gradient for two steps keeps its bits, its state and its version; its first step is step 1."""
    values, grads = case_values()
    late = 7                                            # the 3 PO_CHUNK + 5 tensor
    steps = [(lr, [None if (i == late and k < 2) else g for i, g in enumerate(gs)]) for k, (lr, gs) in enumerate(zip(LRS, grads))]
    ps = make_params(values, device)
    opt = make_optimizer(ps, max_norm=CLIP)
    before = ps[late].detach().clone()
    for k, (lr, gs) in enumerate(steps):
        set_lr(opt, lr)
        set_grads(ps, gs, device)
        versions = [p._version for p in ps]
        opt.step()
        moved = [p._version > v for p, v in zip(ps, versions)]
        assert moved == [gs[i] is not None for i in range(len(ps))], (k, moved)
        records, state = our_records(ps, opt), our_state(ps, opt)
        if k < 2:
            assert bits_equal([ps[late].detach()], [before]) and tuple(records[late]) == (0, 1.0, 1.0)
            assert not state["m"][late].any() and not state["v"][late].any()
    assert records["step"].tolist() == [3] * late + [1] + [3] * (len(ps) - late - 1)
    assert records["beta1_pow"][late] == BETAS[0] and records["beta1_pow"][0] == BETAS[0] * BETAS[0] * BETAS[0]
    v32, v64 = twins(values, steps, CLIP, device)
    assert_within(our_state(ps, opt), v32, v64, f"first gradient at step 3, {device}")
    sd = opt.state_dict()["state"]
    at = slots(ps, opt)
    assert float(sd[at[late]]["step"]) == 1.0 and float(sd[at[0]]["step"]) == 3.0


def bad_gradients(grads):
    out = [g.clone() for g in grads]
    out[5][17] = float("nan")
    out[5][PO_CHUNK - 1] = float("inf")
    return out


def check_nonfinite_propagate(device):
    """One NaN and one inf in one gradient, the default policy: non-finite wherever the twin is."""
    values, grads = case_values(2)
    for max_norm in (CLIP, None):
        steps = [(LRS[0], grads[0]), (LRS[1], bad_gradients(grads[1]))]
        ps, opt = our_run(values, steps, device, max_norm=max_norm)
        got = our_state(ps, opt)
        v32 = ref.twin_run([v.to(device) for v in values], GROUPS, BETAS, EPS, steps, max_norm, torch.float32)
        for k in ref.QUANTITIES:
            for i, (a, t) in enumerate(zip(got[k], v32[k])):
                assert torch.equal(torch.isfinite(a), torch.isfinite(t)), (k, i, max_norm)
                assert torch.equal(torch.isnan(a), torch.isnan(t)), (k, i, max_norm)
        assert not math.isfinite(float(opt.grad_norm)) and int(opt.skipped_steps) == 0
        assert opt._buffers().get_states()["step"].tolist() == [2] * len(ps)
        if max_norm is None:      # without the clip the damage stays in the elements that were bad
            assert sum(int((~torch.isfinite(a)).sum()) for a in got["p"]) == 2
        else:                     # a NaN norm makes the clip coefficient NaN: every weight
            assert all(bool(torch.isnan(a).all()) for a in got["p"])


def check_nonfinite_skip(device):
    """The skip policy: the bad step changes no bit of p, m, v or the state records and is counted; the next finite step is
    the one of a run that never saw the bad one."""
    values, grads = case_values(3)
    ps = make_params(values, device)
    opt = make_optimizer(ps, max_norm=CLIP, on_nonfinite="skip")
    set_lr(opt, LRS[0]), set_grads(ps, grads[0], device), opt.step()
    before, records = our_state(ps, opt), opt._buffers().get_states()
    set_lr(opt, LRS[1]), set_grads(ps, bad_gradients(grads[1]), device), opt.step()
    after = our_state(ps, opt)
    assert all(bits_equal(before[k], after[k]) for k in ref.QUANTITIES)
    assert opt._buffers().get_states().tobytes() == records.tobytes()
    assert int(opt.skipped_steps) == 1 and not math.isfinite(float(opt.grad_norm))
    set_lr(opt, LRS[2]), set_grads(ps, grads[2], device), opt.step()
    clean = our_run(values, [(LRS[0], grads[0]), (LRS[2], grads[2])], device, max_norm=CLIP, on_nonfinite="skip")
    a, b = our_state(ps, opt), our_state(*clean)
    assert all(bits_equal(a[k], b[k]) for k in ref.QUANTITIES)
    assert int(opt.skipped_steps) == 1 and int(clean[1].skipped_steps) == 0 and math.isfinite(float(opt.grad_norm))
    assert opt._buffers().get_states().tobytes() == clean[1]._buffers().get_states().tobytes()


def check_state_dict_round_trips(device):
    """Two steps with ours, loaded into torch for two more; the same the other way round; both against four uninterrupted
    steps of the twin."""
    values, grads = case_values(4)
    lrs = LRS + (1e-3,)
    steps = list(zip(lrs, grads))
    v32, v64 = twins(values, steps, CLIP, device)

    ps, opt = our_run(values, steps[:2], device, max_norm=CLIP)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(len(ps))) and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    tps, topt = ref.twin_optimizer([p.detach() for p in ps], GROUPS, BETAS, EPS, torch.float32)
    topt.load_state_dict(sd)
    for lr, gs in steps[2:]:
        ref.twin_step(tps, topt, [g.to(device) for g in gs], lr, CLIP)
    assert_within(ref.twin_state(tps, topt), v32, v64, f"ours (2 steps) -> torch (2 steps), {device}")

    tps, topt = ref.twin_optimizer([v.to(device) for v in values], GROUPS, BETAS, EPS, torch.float32)
    for lr, gs in steps[:2]:
        ref.twin_step(tps, topt, [g.to(device) for g in gs], lr, CLIP)
    ps = make_params([p.detach() for p in tps], device)
    opt = make_optimizer(ps, max_norm=CLIP)
    opt.load_state_dict(topt.state_dict())
    records = opt._buffers().get_states()
    assert records["step"].tolist() == [2] * len(ps) and records["beta2_pow"][0] == math.pow(BETAS[1], 2)
    for lr, gs in steps[2:]:
        set_lr(opt, lr), set_grads(ps, gs, device), opt.step()
    assert_within(our_state(ps, opt), v32, v64, f"torch (2 steps) -> ours (2 steps), {device}")
    again = opt.state_dict()
    assert [float(again["state"][i]["step"]) for i in range(len(ps))] == [4.0] * len(ps)
    assert again["param_groups"][0]["weight_decay"] == DECAY and again["param_groups"][1]["params"] == [5, 6, 7, 8]


def check_versions(device):
    values, grads = case_values(1)
    ps = make_params(values, device)
    opt = make_optimizer(ps)
    set_grads(ps, [None if i == 2 else g for i, g in enumerate(grads[0])], device)
    versions = [p._version for p in ps]
    opt.step()
    assert [p._version > v for p, v in zip(ps, versions)] == [i != 2 for i in range(len(ps))]


def check_refusals(device):
    """More groups than PO_MAX_GROUPS, an fp16 parameter, amsgrad, maximize, a non-contiguous parameter, a sparse gradient:
    each raises with a message before anything is launched."""
    import pytest
    from pasco_amd.grad.optimlib import PO_MAX_GROUPS
    mk = lambda *s, dtype=torch.float32: torch.nn.Parameter(torch.zeros(*s, dtype=dtype, device=device))
    with pytest.raises(ValueError, match="PO_MAX_GROUPS"):
        AdamW([{"params": [mk(3)]} for _ in range(PO_MAX_GROUPS + 1)])
    AdamW([{"params": [mk(3)]} for _ in range(PO_MAX_GROUPS)])
    with pytest.raises(TypeError, match="fp32 only"):
        AdamW([mk(3, dtype=torch.float16)])
    with pytest.raises(TypeError, match="amsgrad"):
        AdamW([mk(3)], amsgrad=True)
    with pytest.raises(TypeError, match="maximize"):
        AdamW([mk(3)], maximize=True)
    with pytest.raises(TypeError, match="non-contiguous"):
        AdamW([torch.nn.Parameter(torch.zeros(4, 6, device=device).t())])
    with pytest.raises(ValueError, match="on_nonfinite"):
        AdamW([mk(3)], on_nonfinite="ignore")
    p = mk(4, 3)
    opt = AdamW([p])
    p.grad = torch.zeros(4, 3, device=device).to_sparse()
    with pytest.raises(TypeError, match="sparse"):
        opt.step()
    opt = AdamW([mk(3)])
    opt.add_param_group({"params": [mk(2)], "weight_decay": 0.0})
    assert len(opt.param_groups) == 2
    with pytest.raises(TypeError, match="amsgrad"):
        opt.add_param_group({"params": [mk(2)], "amsgrad": True})
    assert len(opt.param_groups) == 2


def check_non_contiguous_gradient(device):
    """A transposed gradient is read from a contiguous copy; a group added after the first step joins with step 0."""
    g = torch.Generator().manual_seed(5)
    w0, g0, w1, g1 = (torch.randn(s, generator=g) for s in ((6, 5), (5, 6), (9,), (9,)))
    runs = []
    for transposed in (True, False):
        p = torch.nn.Parameter(w0.to(device).clone())
        opt = AdamW([p], lr=1e-2, max_norm=CLIP)
        p.grad = g0.to(device).t() if transposed else g0.t().contiguous().to(device)
        assert p.grad.is_contiguous() != transposed
        opt.step()
        q = torch.nn.Parameter(w1.to(device).clone())
        opt.add_param_group({"params": [q], "weight_decay": 0.0})
        p.grad, q.grad = g0.to(device).t().contiguous(), g1.to(device)
        opt.step()
        assert opt._buffers().get_states()["step"].tolist() == [2, 1]
        runs.append([p.detach().clone(), q.detach().clone()] + [t.clone() for t in opt._buffers().m + opt._buffers().v])
    assert bits_equal(runs[0], runs[1])


def check_scheduler_drives_it(device):
    """LambdaLR(warmup_cosine) sets the learning rate the step uses."""
    from pasco_amd.grad.optim import warmup_cosine
    p = torch.nn.Parameter(torch.ones(5, device=device))
    opt = AdamW([p], lr=0.5, weight_decay=0.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_cosine(4, 100, 0.01))
    seen = []
    for _ in range(6):
        p.grad = torch.ones(5, device=device)
        before = p.detach().clone()
        opt.step()
        sched.step()
        seen.append(float((before - p.detach()).abs().max()))
    want = [0.0, 0.125, 0.25, 0.375, 0.5, 0.5]          # Adam's step on a constant gradient is lr
    assert all(abs(a - b) <= 1e-6 for a, b in zip(seen, want)), seen
    opt.zero_grad()
    assert p.grad is None


def restate_steps(values, steps, max_norm, sums, groups=GROUPS):
    """The steps again on the host with the restatement of pasco_amd/grad/host.py: `sums[k]` is the sum of squares the device
    found at step k (read from its result record), from which the clip scale is formed by the same fp64 expression; the
    powers of beta by the same repeated fp64 products.  -> {"p", "m", "v"} on the host."""
    ps = [v.clone() for v in values]
    ms, vs = [torch.zeros_like(v) for v in values], [torch.zeros_like(v) for v in values]
    pows = [[1.0, 1.0] for _ in values]
    wd = {i: w for idx, w in groups for i in idx}
    for (lr, gs), sumsq in zip(steps, sums):
        _, s = host.optim_clip(sumsq, 0.0 if max_norm is None else max_norm, 1.0)
        for i, g in enumerate(gs):
            if g is None:
                continue
            pows[i][0] *= BETAS[0]
            pows[i][1] *= BETAS[1]
            k = host.optim_scalars(lr, BETAS[0], BETAS[1], EPS, wd[i], pows[i][0], pows[i][1])
            host.optim_adamw_(ps[i], g, ms[i], vs[i], s, k)
    return {"p": ps, "m": ms, "v": vs}


def check_long(device, name):
    """A LONG_CASE: its steps against the twins, the first step's sum of squares against math.fsum, a repeat run bit for bit.
    -> (case, parameters, optimiser, the sums of squares per step) for what the GPU side adds."""
    case = LONG_CASES[name]
    values, steps = case.values()
    sums = []
    ps, opt = our_run(values, steps, device, case.groups, False, sums, max_norm=CLIP)
    again = our_run(values, steps, device, case.groups, False, max_norm=CLIP)
    a, b = our_state(ps, opt), our_state(*again)
    assert all(bits_equal(a[k], b[k]) for k in ref.QUANTITIES), f"{name}: a repeat run gives other bits"
    assert torch.equal(opt._buffers().result.view(torch.int64), again[1]._buffers().result.view(torch.int64))
    assert opt._buffers().get_states().tobytes() == again[1]._buffers().get_states().tobytes()
    assert our_records(ps, opt)["step"].tolist() == [case.n_steps] * len(ps)
    assert float(opt.grad_norm) > CLIP, "the clip is meant to act"
    n = sum(case.sizes)
    exact = ref.exact_sum_of_squares(steps[0][1])
    rel = abs(sums[0] - exact) / exact
    print(f"[optim] {name}: sum of squares over {n} elements: relative error {rel:.3e}, bound {n * 2.0 ** -53:.3e}")
    assert rel <= n * 2.0 ** -53
    v32, v64 = twins(values, steps, CLIP, device, case.groups)
    assert_within(a, v32, v64, f"{name}, {case.n_steps} steps, {device}")
    return case, ps, opt, sums
