"""Test helper: the cases of the train / eval boundary tests (tests/test_modes_cpu.py on the CPU oracle, tests/test_hip_modes.py on
the MI355X).  Every check crosses from one mode to the other: a module in `.train()` or `.eval()`, parameters and features that do
or do not require grad, autograd enabled or not, and an input that is either plain or carries the pending prologue of an
eval-mode `MinkowskiBatchNorm -> activation` run under `torch.no_grad()`.

Maps: the 12 x 12 x 6 boxes of tests/grad_cases.py (a few hundred rows); channel counts are multiples of 8, so the device takes
the split-precision route wherever the module's state allows it.  References are fp64 twins written from the formulas
(tests/grad_ref64.py, tests/conv_ref64.py); each function returns a list of failure lines (empty = passed), so that one run shows
every cell of a matrix that is wrong."""
import itertools

import torch
import torch.nn as nn
import torch.nn.functional as F

import pasco_amd.me as ME
from pasco_amd.me import modules as M
from tests.conv_ref64 import act64, gather_sum64, violations
from tests.grad_cases import KINDS, box_coords, make_map, make_module  # noqa: F401
from tests.grad_ref64 import C_WGRAD, STACK_M, conv_twin, invert_torch, sum_cap, wgrad64
from tests.test_me_guarded_conv import _scene

CIN, COUT = 16, 24
INPUTS = ("plain", "relu", "leaky")
ACT_OF = {"relu": 1, "leaky": 2}
LEAKY_SLOPE = 0.2


# ---- building blocks --------------------------------------------------------------------------------------------------------
def randomise_bn(bn, seed):
    g = torch.Generator().manual_seed(seed)
    c = bn.bn.num_features
    with torch.no_grad():
        bn.bn.running_mean.copy_(torch.randn(c, generator=g) * 0.3)
        bn.bn.running_var.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bn.weight.copy_(torch.rand(c, generator=g) + 0.5)
        bn.bn.bias.copy_(torch.randn(c, generator=g) * 0.1)
    return bn


def fold64(bn):
    """(scale, shift) of the eval-mode normalisation in fp64, from the module's buffers."""
    m = bn.bn
    scale = m.weight.detach().double() / torch.sqrt(m.running_var.double() + m.eps)
    return scale, m.bias.detach().double() - m.running_mean.double() * scale


def operand64(raw, bn, act, slope):
    """-> (h, dh_draw) fp64: h = act(raw * scale + shift) and its derivative with respect to raw, element-wise.  No element may
    sit within rounding of the activation's kink, where the fp32 and the fp64 derivative could differ."""
    scale, shift = fold64(bn)
    pre = raw.detach().double() * scale + shift
    room = 1e-5 * ((raw.detach().double() * scale).abs() + shift.abs())
    assert bool((pre.abs() > room).all()), "an element at the activation's kink: choose another seed"
    slope_d = torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.0 if act == 1 else slope))
    return act64(pre, act, slope), slope_d * scale


def front(inp, device, seed=21):
    """The eval-mode BatchNorm -> activation in front of the convolution under test (None, None for a plain input)."""
    if inp == "plain":
        return None, None
    bn = randomise_bn(ME.MinkowskiBatchNorm(CIN), seed).to(device).eval()
    act = ME.MinkowskiReLU() if inp == "relu" else ME.MinkowskiLeakyReLU(LEAKY_SLOPE)
    return bn, act.eval()


def tensor_on(m, feats):
    return ME.SparseTensor(feats, coordinate_map_key=m["in_key"], coordinate_manager=m["mgr"])


def conv_grads64(h64, dh_draw, kernel, dy, m):
    """The three gradients of sum_k h[nbr[k]] @ W[k] + b for the upstream gradient dy, in fp64, with the magnitudes of the
    element-wise bounds: dict(w = (ref, A), b = (ref, bound), x = (ref, mag)); the input gradient is the one of the RAW rows
    (d_h * dh_draw; dh_draw None = the operand is the input itself)."""
    ref_w, a_w = wgrad64(h64, dy, m["nbr"])
    ref_b = dy.double().sum(0)
    bound_b = sum_cap(m["n_out"]) * dy.double().abs().sum(0) + 1e-30
    inv = invert_torch(m["nbr"], m["n_in"])
    w_t = kernel.detach().transpose(1, 2).contiguous()
    acc, mag = gather_sum64(dy, w_t, inv, torch.arange(m["n_in"], device=dy.device))
    if dh_draw is not None:
        acc, mag = acc * dh_draw, mag * dh_draw.abs()
    return dict(w=(ref_w, a_w), b=(ref_b, bound_b), x=(acc, mag))


def check_grads(ref, kernel_grad, bias_grad, feats_grad, what):
    """Element-wise: the weight gradient by C_WGRAD * A, the bias gradient by sum_cap(n_out) * sum |dy|, the input gradient by
    conv_ref64.violations.  A None gradient is not checked here."""
    bad = []
    if kernel_grad is not None:
        r, a = ref["w"]
        err = (kernel_grad.double().reshape(r.shape) - r).abs()
        if not bool((err <= C_WGRAD * a + 1e-30).all()):
            bad.append(f"{what}: weight gradient, worst err / A = {float((err / (a + 1e-300)).max()):.3e} > C_WGRAD = {C_WGRAD:.3e}")
    if bias_grad is not None:
        r, b = ref["b"]
        err = (bias_grad.double().reshape(-1) - r).abs()
        if not bool((err <= b).all()):
            bad.append(f"{what}: bias gradient, worst err / bound = {float((err / b).max()):.3e}")
    if feats_grad is not None:
        r, mag = ref["x"]
        v = violations(feats_grad, r, mag, r.abs())
        if bool(v.any()):
            bad.append(f"{what}: input gradient, {int(v.sum())} elements outside the bound")
    return bad


# ---- (a) the mode matrix of one convolution -------------------------------------------------------------------------------
def mode_matrix(kind, inp, device, be):
    """Every cell of {train, eval} x {kernel, bias, features require grad or not} x {autograd enabled, no_grad} for one
    convolution of `kind` behind the input `inp`.  -> failure lines."""
    m = make_map(kind, device)
    torch.manual_seed(7)
    mod = make_module(kind, CIN, COUT).to(device)
    bn, act = front(inp, device)
    g = torch.Generator().manual_seed(31)
    raw0 = torch.randn(m["n_in"], CIN, generator=g).to(device)
    dy = torch.randn(m["n_out"], COUT, generator=g).to(device)
    if inp == "plain":
        ref = conv_grads64(raw0.double(), None, mod.kernel, dy, m)
    else:
        h64, dh = operand64(raw0, bn, ACT_OF[inp], LEAKY_SLOPE)
        ref = conv_grads64(h64, dh, mod.kernel, dy, m)

    def the_input(raw):
        if inp == "plain":
            return tensor_on(m, raw)
        with torch.no_grad():
            h = act(bn(tensor_on(m, raw)))
        assert h._pending is not None and h._pending[2] == ACT_OF[inp], "the front did not defer"
        return h

    bad = []
    for training, kreq, breq, freq, grad_on in itertools.product((True, False), repeat=5):
        what = (f"{kind} / {inp}: {'train' if training else 'eval'}, kernel {int(kreq)}, bias {int(breq)}, features {int(freq)}, "
                f"{'autograd' if grad_on else 'no_grad'}")
        mod.train(training)
        mod.kernel.requires_grad_(kreq)
        mod.bias.requires_grad_(breq)
        mod.kernel.grad = mod.bias.grad = None
        raw = raw0.clone().requires_grad_(freq)
        with torch.set_grad_enabled(grad_on):
            out = mod(the_input(raw)).F
        # grad_fn: exactly when autograd is enabled and something asks, whatever is pending
        wants = grad_on and (kreq or breq or freq)
        if (out.grad_fn is not None) != wants or out.requires_grad != wants:
            bad.append(f"{what}: grad_fn {out.grad_fn}, requires_grad {out.requires_grad}, expected {'one' if wants else 'none'}")
            continue
        # forward values: a plain input against the module's own launch for this state (the exact route for a training-mode
        # kernel that requires grad, the guarded one otherwise), bit for bit; a pending input against the same call on the
        # materialised tensor
        if inp == "plain":
            exact = grad_on and kreq and training
            want = mod._launch(be, raw0, m["nbr"], m["n_out"], m["mgr"], None, exact)
            if not torch.equal(out.detach(), want):
                bad.append(f"{what}: forward differs from _launch(exact={exact}) by {float((out.detach() - want).abs().max()):.3e}")
        else:
            h = the_input(raw0)
            h.F
            assert h._pending is None
            with torch.set_grad_enabled(grad_on):
                want = mod(h).F.detach()
            if not torch.allclose(out.detach(), want, rtol=1e-5, atol=1e-6):
                bad.append(f"{what}: forward differs from the materialised call by {float((out.detach() - want).abs().max()):.3e}")
        if not wants:
            continue
        out.backward(dy)
        got = (mod.kernel.grad, mod.bias.grad, raw.grad)
        for name, t, req, shape in (("kernel", got[0], kreq, mod.kernel.shape), ("bias", got[1], breq, mod.bias.shape),
                                    ("features", got[2], freq, raw.shape)):
            if (t is not None) != req:
                bad.append(f"{what}: {name}.grad is {'missing' if req else 'present'}")
            elif req and t.shape != shape:
                bad.append(f"{what}: {name}.grad has shape {tuple(t.shape)}, the tensor {tuple(shape)}")
        bad += check_grads(ref, *got, what)
    mod.kernel.requires_grad_(True)
    return bad


# ---- (b) a frozen body and a trainable head -------------------------------------------------------------------------------
class Body(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = ME.MinkowskiConvolution(CIN, 32, kernel_size=3, bias=True, dimension=3)
        self.bn = ME.MinkowskiBatchNorm(32)
        self.relu = ME.MinkowskiReLU()

    def forward(self, x):
        return self.relu(self.bn(self.conv(x)))


def frozen_body(device, be, body_autograd):
    """body (conv -> BN -> ReLU, eval) and a head convolution with bias (train, autograd enabled).  `body_autograd` False: the
    body runs under no_grad (its output carries a pending prologue).  True: the body's parameters are frozen, it runs with autograd
    enabled and the input features require grad - the guarded forward inside ConvFunction.  -> failure lines."""
    m = make_map("same", device)
    torch.manual_seed(9)
    body, head = Body().to(device).eval(), make_module("same", 32, COUT).to(device).train()
    randomise_bn(body.bn, 23)
    g = torch.Generator().manual_seed(33)
    feats = torch.randn(m["n_in"], CIN, generator=g).to(device)
    tgt = torch.randn(m["n_out"], COUT, generator=g).to(device)
    bad = []
    if body_autograd:
        body.requires_grad_(False)
        feats.requires_grad_(True)
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)          # "eval-mode modules called with autograd enabled": said once
            h = body(tensor_on(m, feats))
        if h.F.grad_fn is None:
            bad.append("frozen body under autograd: the body's output has no grad_fn")
        want = body.conv._launch(be, feats.detach(), m["nbr"], m["n_out"], m["mgr"], None, False)
        with torch.no_grad():
            y = body.conv(tensor_on(m, feats.detach())).F
        if not torch.equal(y, want):
            bad.append("frozen body under autograd: the convolution's values differ from the guarded launch")
    else:
        with torch.no_grad():
            h = body(tensor_on(m, feats))
        assert h._pending is not None and h._pending[2] == 1, "the body did not defer"
    raw = h._F.detach().clone()                                      # what the pending operations (if any) apply to
    out = head(h)
    if out.F.grad_fn is None:
        mode = "autograd" if body_autograd else "no_grad"
        return bad + [f"frozen body ({mode}): the head's output has no grad_fn - it never trains"]
    loss = (out.F * tgt).sum()
    loss.backward()
    if head.kernel.grad is None or head.bias.grad is None:
        return bad + ["frozen body: the head's kernel.grad / bias.grad is None"]
    if any(p.grad is not None for p in body.parameters()):
        bad.append("frozen body: a parameter of the body received a gradient")
    h64 = raw.double() if body_autograd else operand64(raw, body.bn, 1, 0.0)[0]
    ref = conv_grads64(h64, None, head.kernel, tgt, m)
    bad += check_grads(ref, head.kernel.grad, head.bias.grad, None, "frozen body, head")
    if body_autograd:                                # the input gradient through the whole chain: the stack's criterion
        if feats.grad is None:
            return bad + ["frozen body under autograd: the input features received no gradient"]
        twins = {}
        for dt in (torch.float32, torch.float64):
            x = feats.detach().to(dt).requires_grad_(True)
            bnm = body.bn.bn
            t = conv_twin(x, body.conv.kernel.detach().to(dt), m["nbr"], body.conv.bias.detach().to(dt))
            t = F.batch_norm(t, bnm.running_mean.to(dt), bnm.running_var.to(dt), bnm.weight.detach().to(dt),
                             bnm.bias.detach().to(dt), False, 0.0, bnm.eps)
            t = conv_twin(torch.relu(t), head.kernel.detach().to(dt), m["nbr"], head.bias.detach().to(dt))
            (t * tgt.to(dt)).sum().backward()
            twins[dt] = x.grad.double()
        e = float((feats.grad.double() - twins[torch.float64]).abs().max())
        e32 = float((twins[torch.float32] - twins[torch.float64]).abs().max())
        print(f"frozen body under autograd: input gradient max |g - g64| = {e:.3e} = {e / e32:.2f} x max |g32 - g64|")
        if not e <= STACK_M * e32:
            bad.append(f"frozen body under autograd: input gradient {e / e32:.2f} x the fp32 twin's error, bound {STACK_M}")
    return bad


# ---- (c) train / validate cycles ----------------------------------------------------------------------------------------------
class Small(nn.Module):
    """conv -> BN -> ReLU -> conv."""

    def __init__(self, momentum=0.1):
        super().__init__()
        self.c1 = ME.MinkowskiConvolution(CIN, 32, kernel_size=3, bias=True, dimension=3)
        self.bn = ME.MinkowskiBatchNorm(32, momentum=momentum)
        self.relu = ME.MinkowskiReLU()
        self.c2 = ME.MinkowskiConvolution(32, COUT, kernel_size=3, bias=True, dimension=3)

    def forward(self, x):
        return self.c2(self.relu(self.bn(self.c1(x))))


def _validate(model, momentum, m, feats, device, what):
    """The warm model's eval output against a freshly constructed model with the same state; the fresh model's deferred BatchNorm
    against F.batch_norm with the current buffers.  -> failure lines."""
    bad = []
    model.eval()
    fresh = Small(momentum).to(device)
    fresh.load_state_dict(model.state_dict())
    fresh.eval()
    with torch.no_grad():
        got, want = model(tensor_on(m, feats)).F, fresh(tensor_on(m, feats)).F
        y = fresh.c1(tensor_on(m, feats))
        d = fresh.bn(y)
        assert d._pending is not None, "the eval-mode BatchNorm did not defer"
        bn = fresh.bn.bn
        ref = F.batch_norm(y.F, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        e = float((d.F - ref).abs().max())
    if not e <= 1e-6:
        bad.append(f"{what}: a fresh model's deferred BatchNorm differs from F.batch_norm by {e:.3e}")
    if not torch.equal(got, want):
        e = float((got - want).abs().max())
        bad.append(f"{what}: eval output differs from a fresh model with the same state_dict by {e:.3e}")
    return bad


def train_validate_cycles(device, momentum=0.1, affine_trains=True):
    """`affine_trains` False: the BatchNorm's weight and bias are frozen, so a training step moves nothing of the BatchNorm but
    its running statistics (an optimiser step on the affine parameters would move their version counters and hide a cache that
    misses the statistics).  Three rounds of (training step, validation), then a statistics recalibration (training-mode forward
    under no_grad), a load_state_dict into the warm model, an in-place kernel update under no_grad, and a `.data` write followed
    by the in-place operation INTEGRATION.md 3c prescribes; a validation after each.  -> failure lines."""
    m = make_map("same", device)
    torch.manual_seed(13)
    model = Small(momentum).to(device)
    g = torch.Generator().manual_seed(35)
    feats = (torch.randn(m["n_in"], CIN, generator=g) * 1.5 + 0.3).to(device)
    tgt = torch.randn(m["n_out"], COUT, generator=g).to(device)
    model.bn.requires_grad_(affine_trains)
    opt = torch.optim.SGD([p for p in model.parameters() if p.requires_grad], lr=0.05)
    bad = _validate(model, momentum, m, feats, device, "before training")
    for r in range(3):
        model.train()
        opt.zero_grad()
        (model(tensor_on(m, feats)).F - tgt).square().mean().backward()
        opt.step()
        bad += _validate(model, momentum, m, feats, device, f"round {r + 1}")
    model.train()
    with torch.no_grad():
        model(tensor_on(m, feats * 2.0 - 1.0))
    bad += _validate(model, momentum, m, feats, device, "recalibration under no_grad")
    torch.manual_seed(14)
    other = Small(momentum).to(device)
    randomise_bn(other.bn, 25)
    model.load_state_dict(other.state_dict())
    bad += _validate(model, momentum, m, feats, device, "load_state_dict into a warm model")
    with torch.no_grad():
        model.c1.kernel.mul_(1.5)
        model.c2.kernel.mul_(0.5)
    bad += _validate(model, momentum, m, feats, device, "kernel.mul_() under no_grad")
    model.c2.kernel.data.mul_(1.5)
    with torch.no_grad():
        model.c2.kernel.add_(0)                      # moves the version counter a .data write leaves alone
    bad += _validate(model, momentum, m, feats, device, ".data write, then add_(0)")
    return bad


def _fold_close(got, bn):
    s64, b64 = fold64(bn)
    return torch.allclose(got[0].double(), s64, rtol=1e-6, atol=1e-7) and torch.allclose(got[1].double(), b64, rtol=1e-6, atol=1e-7)


def fused_fold_after_training_forward(device):
    """`fused.fold_bn` after a training-mode forward of the same BatchNorm: through the ME module and through the bare
    nn.BatchNorm1d (which only advances num_batches_tracked).  -> failure lines."""
    from pasco_amd.graph import fused
    bad = []
    m = make_map("same", device)
    g = torch.Generator().manual_seed(37)
    feats = (torch.randn(m["n_in"], 32, generator=g) * 2.0 + 1.0).to(device)
    for through in ("module", "bare"):
        bn = randomise_bn(ME.MinkowskiBatchNorm(32), 27).to(device).eval()
        if not _fold_close(fused.fold_bn(bn), bn):
            bad.append(f"fold_bn ({through}): the first fold is not the fold of the buffers")
        bn.train()
        with torch.no_grad():
            bn(tensor_on(m, feats)) if through == "module" else bn.bn(feats)
        bn.eval()
        if not _fold_close(fused.fold_bn(bn), bn):
            bad.append(f"fold_bn ({through}): after a training-mode forward the fold is not the fold of the current buffers")
    return bad


def decoder_resize_after_training_forward(device, monkeypatch):
    """The decoder's absorbed `resize` (BatchNorm folded into the 1x1 convolution's weights, cached as `_ph_resize`) after a
    training-mode forward of its BatchNorm: the entry is rebuilt and the output is the one of a fresh block with the same state.
    The tall-operand threshold is lowered for the test: the cache, not the threshold, is the subject.  -> failure lines."""
    from pasco_amd.graph import fused
    from pasco_amd.graph.decoder import DecoderBlock
    monkeypatch.setattr(fused, "MIN_ROWS_LINEAR", 1)
    m = make_map("gen", device)
    g = torch.Generator().manual_seed(39)
    feats = torch.randn(m["n_in"], 32, generator=g).to(device)
    stats = (torch.randn(m["n_out"], 35, generator=g) * 2.0 + 1.0).to(device)

    def block(seed):
        torch.manual_seed(seed)
        return DecoderBlock(32, 32, n_heads=1, compl_head_dim=4, heavy_decoder=False).to(device).eval()

    def run(blk):
        with torch.no_grad():
            out = blk._resize_absorbed(tensor_on(m, feats), m["out_key"], m["nbr"])
        assert out is not None and "_ph_resize" in blk.__dict__, "the absorbed resize did not apply"
        return out.F

    blk = block(1)
    randomise_bn(blk.resize[0], 29)
    run(blk)
    first = blk.__dict__["_ph_resize"]
    bn = blk.resize[0]
    bn.train()
    with torch.no_grad():
        bn.bn(stats)
    bn.eval()
    got = run(blk)
    fresh = block(2)
    fresh.load_state_dict(blk.state_dict())
    want = run(fresh)
    bad = []
    if blk.__dict__["_ph_resize"] is first:
        bad.append("decoder resize: the _ph_resize entry was not rebuilt after a training-mode BatchNorm forward")
    if not torch.equal(got, want):
        bad.append(f"decoder resize: output differs from a fresh block with the same state by {float((got - want).abs().max()):.3e}")
    return bad


# ---- (d) the guarded forward under autograd ---------------------------------------------------------------------------------
GUARDED = [("plain", dict()), ("big", dict(big=5000.0)), ("tiny", dict(gain=1e-8))]


def guarded_under_autograd(device, be, n=4000, extent=(24, 24, 10), variants=GUARDED):
    """The 64 -> 64, 27-offset scene of tests/test_me_guarded_conv.py with a frozen kernel and features that require grad: the
    output is the no_grad guarded output bit for bit (the exact route's where the guard fires: one activation at 5000, a tensor
    of 1e-8), and the input gradient meets fp64.  -> failure lines."""
    bad = []
    torch.manual_seed(3)
    conv = ME.MinkowskiConvolution(64, 64, kernel_size=3, bias=True, dimension=3).to(device).train()
    conv.kernel.requires_grad_(False)
    conv.bias.requires_grad_(False)
    for name, kw in variants:
        coords, feats = _scene(n=n, extent=extent, **kw)
        coords, feats = coords.to(device), feats.to(device).requires_grad_(True)
        x = ME.SparseTensor(feats, coords)
        out = conv(x).F
        if out.grad_fn is None:
            bad.append(f"guarded under autograd ({name}, {n} rows): no grad_fn")
            continue
        with torch.no_grad():
            quiet = conv(ME.SparseTensor(feats.detach(), coordinate_map_key=x.coordinate_map_key,
                                         coordinate_manager=x.coordinate_manager)).F
        if not torch.equal(out.detach(), quiet):
            bad.append(f"guarded under autograd ({name}, {n} rows): differs from the no_grad guarded output")
        M.set_me_conv("exact")
        try:
            with torch.no_grad():
                exact = conv(ME.SparseTensor(feats.detach(), coordinate_map_key=x.coordinate_map_key,
                                             coordinate_manager=x.coordinate_manager)).F
        finally:
            M.set_me_conv("guarded")
        if name == "plain":
            if torch.equal(out.detach(), exact) and device.type == "cuda":
                bad.append(f"guarded under autograd ({name}, {n} rows): the split kernel did not do the work")
        elif not torch.equal(out.detach(), exact):
            bad.append(f"guarded under autograd ({name}, {n} rows): the guard fired but the output is not the exact route's")
        g = torch.Generator().manual_seed(41)
        dy = torch.randn(out.shape, generator=g).to(device)
        out.backward(dy)
        mgr = x.coordinate_manager
        nbr = mgr.kernel_map(x.coordinate_map_key, x.coordinate_map_key, 3)
        inv = invert_torch(nbr, n)
        acc, mag = gather_sum64(dy, conv.kernel.detach().transpose(1, 2).contiguous(), inv, torch.arange(n, device=device))
        v = violations(feats.grad, acc, mag, acc.abs())
        if bool(v.any()):
            bad.append(f"guarded under autograd ({name}, {n} rows): input gradient, {int(v.sum())} elements outside the bound")
        if conv.kernel.grad is not None or conv.bias.grad is not None:
            bad.append(f"guarded under autograd ({name}, {n} rows): a frozen parameter received a gradient")
    be.check_status(device)
    return bad
