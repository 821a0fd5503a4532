"""AdamW with the global-norm gradient clip folded in (include/pasco_optim.h, the `po_*` kernels) - the optimiser of the
reference's `configure_optimizers` under Lightning's `gradient_clip_val`, as one object:

    opt = AdamW(net.parameters(), lr=1e-4, weight_decay=0.0, max_norm=0.5)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, warmup_cosine(0, 50000, 0.01))
    loss.backward(); opt.step(); sched.step(); opt.zero_grad()

A step is three launches whatever the number of parameter tensors: the squared gradient norm per chunk in fp64, one small
kernel that sums the partials in a fixed order, forms the clip scale and advances the per-tensor step records, and the update,
which multiplies every gradient element by the clip scale as it reads it - the gradients are never rewritten.  Nothing is read
back: `grad_norm` and `skipped_steps` are 0-d views of the device's result record, and reading them is the caller's
synchronisation.  The same inputs give the same bits on every run.

`on_nonfinite="skip"` leaves every weight, moment and step count as it is when a gradient element is inf or NaN and counts the
step in `skipped_steps`; "propagate" (the default) is torch's behaviour.  `grad_scale` multiplies every gradient (1 / k after k
accumulated backward passes); the norm is that of the scaled gradients.

The kernels write the weights through raw pointers, which moves no version counter, so `step()` moves the counters itself
(`torch.autograd.graph.increment_version`): every tensor derived from a weight sees the step.

CPU parameters run the restatement of pasco_amd/grad/host.py with the same expression order.  All parameters of one optimiser
live on one device."""
from __future__ import annotations

import math
from typing import Callable

import numpy as np
import torch

from . import host
from .optimlib import (CHUNK_DTYPE, PO_CHUNK, PO_MAX_GROUPS, PO_POLICY_PROPAGATE, PO_POLICY_SKIP, STATE_DTYPE, TENSOR_DTYPE,
                       optim_lib)

_f4, _f8 = torch.float32, torch.float64


def warmup_cosine(warmup_end: int, max_iter: int, factor_min: float) -> Callable[[int], float]:
    """The learning-rate factor of the reference's schedule as it runs (for `LambdaLR`): it rises linearly from 0 over the first
    `warmup_end` iterations, is 1.0 from there on and 0.1 past iteration 60 000.  The name and the two unused arguments are
    the reference's: its cosine branch is switched off, so `max_iter` and `factor_min` change nothing."""
    def factor(iteration: int) -> float:
        if iteration > 60000:
            return 0.1
        if iteration < warmup_end:
            return min(iteration / warmup_end, 1.0)
        return 1.0
    return factor


def build_tables(entries, m_ptrs, v_ptrs):
    """The two tables of include/pasco_optim.h as record arrays.  entries: (state index, group, address of p, address of g,
    elements) per tensor; m_ptrs / v_ptrs: the addresses of its moments.  A tensor of n elements gets ceil(n / PO_CHUNK) chunks
    at the starts 0, PO_CHUNK, 2 PO_CHUNK, ...; a tensor without elements gets none."""
    n = np.array([e[4] for e in entries], dtype=np.int64)
    tab = np.zeros(len(entries), dtype=TENSOR_DTYPE)
    tab["p"], tab["g"], tab["n"] = [e[2] for e in entries], [e[3] for e in entries], n
    tab["m"], tab["v"] = m_ptrs, v_ptrs
    tab["group"], tab["state"] = [e[1] for e in entries], [e[0] for e in entries]
    per = (n + PO_CHUNK - 1) // PO_CHUNK
    chunks = np.zeros(int(per.sum()), dtype=CHUNK_DTYPE)
    chunks["tensor"] = np.repeat(np.arange(len(entries), dtype=np.int32), per)
    chunks["start"] = (np.arange(len(chunks), dtype=np.int64) - np.repeat(np.cumsum(per) - per, per)) * PO_CHUNK
    return tab, chunks


def _upload(arr: np.ndarray, device) -> torch.Tensor:
    """The bytes of a record array as a device buffer (at least one byte long, so that it has an address)."""
    raw = np.frombuffer(arr.tobytes() or b"\0", dtype=np.uint8).copy()
    return torch.from_numpy(raw).to(device)


class _Buffers:
    """What one optimiser keeps on its device: the two moments of every parameter as 16-byte-aligned slices of one flat
    buffer, the state records, the scalars, the result and step records, and the tables of the last step."""

    def __init__(self, params, device):
        self.device = device
        self.ids = tuple(id(p) for p in params)
        offsets, total = [], 0
        for p in params:
            offsets.append(total)
            total += (p.numel() + 3) // 4 * 4
        self.flat = torch.zeros(2 * total, dtype=_f4, device=device)
        self.m = [self.flat[o:o + p.numel()].view(p.shape) for o, p in zip(offsets, params)]
        self.v = [self.flat[total + o:total + o + p.numel()].view(p.shape) for o, p in zip(offsets, params)]
        assert all(t.data_ptr() % 16 == 0 for t in self.m + self.v if t.numel())
        self.set_states(np.array([(0, 1.0, 1.0)] * len(params), dtype=STATE_DTYPE))
        self.scalars = torch.zeros((max(len(params), 1), 8), dtype=_f4, device=device)
        self.result = torch.zeros(3, dtype=_f8, device=device)
        self.step = torch.zeros(2, dtype=torch.int32, device=device)
        self.key, self.tensors, self.chunks, self.partials, self.n_chunks = None, None, None, None, 0

    def set_states(self, records: np.ndarray):
        raw = np.frombuffer(records.tobytes(), dtype=np.float64).reshape(-1, 3).copy()      # the step's bits ride along
        self.states = torch.from_numpy(raw).to(self.device) if len(raw) else torch.zeros((1, 3), dtype=_f8, device=self.device)

    def get_states(self) -> np.ndarray:
        return np.frombuffer(self.states.cpu().numpy().tobytes(), dtype=STATE_DTYPE)[:len(self.ids)].copy()


class AdamW(torch.optim.Optimizer):
    """`torch.optim.AdamW(params, lr, betas, eps, weight_decay)` with `torch.nn.utils.clip_grad_norm_(params, max_norm)` in
    front of it, on the po_* kernels.  `param_groups`, `zero_grad`, `add_param_group`, `state_dict` and `load_state_dict` are
    torch's in behaviour and format, so schedulers and trainers drive it unchanged and checkpoints go both ways."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_norm=None, grad_scale: float = 1.0, on_nonfinite: str = "propagate", amsgrad: bool = False,
                 maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if on_nonfinite not in ("propagate", "skip"):
            raise ValueError(f"on_nonfinite = {on_nonfinite!r}: 'propagate' or 'skip'")
        if not (grad_scale > 0 and math.isfinite(grad_scale)):
            raise ValueError(f"grad_scale = {grad_scale}: positive and finite")
        self.max_norm = max_norm
        self.grad_scale = float(grad_scale)
        self.on_nonfinite = on_nonfinite
        self._buf = None
        # torch.optim.AdamW's group keys, so that a state dict of either loads into the other
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    # ---- what is served -------------------------------------------------------------------------------------------------
    def _check_groups(self):
        if len(self.param_groups) > PO_MAX_GROUPS:
            raise ValueError(f"{len(self.param_groups)} parameter groups; at most PO_MAX_GROUPS = {PO_MAX_GROUPS} are served")
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise TypeError("pasco_amd.grad.optim.AdamW serves neither amsgrad nor maximize")
            if group.get("decoupled_weight_decay", True) is False:
                raise TypeError("pasco_amd.grad.optim.AdamW decays the weights decoupled from the gradient (AdamW, not Adam)")
            for p in group["params"]:
                if p.dtype != _f4:
                    raise TypeError(f"a {p.dtype} parameter of shape {tuple(p.shape)}: fp32 only")
                if not p.is_contiguous():
                    raise TypeError(f"a non-contiguous parameter of shape {tuple(p.shape)}")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        try:
            self._check_groups()
        except (TypeError, ValueError):
            self.param_groups.pop()
            raise

    def _params(self):
        return [p for group in self.param_groups for p in group["params"]]

    def _buffers(self) -> _Buffers:
        """The buffers of the current parameter list on the parameters' device; what an earlier list or device held is carried
        over (`add_param_group`, `net.cuda()` after construction)."""
        params = self._params()
        devices = {p.device for p in params}
        if len(devices) != 1:
            raise ValueError(f"the parameters of one optimiser live on one device, these are on {sorted(map(str, devices))}")
        device = devices.pop()
        old = self._buf
        if old is not None and old.device == device and old.ids == tuple(id(p) for p in params):
            return old
        new = _Buffers(params, device)
        if old is not None:
            slot = {pid: i for i, pid in enumerate(old.ids)}
            records, had = new.get_states(), old.get_states()
            for i, p in enumerate(params):
                j = slot.get(id(p))
                if j is not None:
                    new.m[i].copy_(old.m[j]), new.v[i].copy_(old.v[j])
                    records[i] = had[j]
            new.set_states(records)
            new.result.copy_(old.result)
        self._buf = new
        return new

    # ---- the result record ----------------------------------------------------------------------------------------------
    @property
    def grad_norm(self) -> torch.Tensor:
        """The global L2 norm of the (scaled) gradients of the last step, before the clip: a 0-d fp64 view on the device."""
        return self._buffers().result[1]

    @property
    def sum_of_squares(self) -> torch.Tensor:
        return self._buffers().result[0]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """How many steps `on_nonfinite="skip"` has skipped: a 0-d int64 view on the device."""
        return self._buffers().result.view(torch.int64)[2]

    # ---- the step -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._check_groups()
        buf = self._buffers()
        listed, slot = [], 0          # (state index, group, parameter, gradient)
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                g = p.grad
                if g is not None:
                    if g.is_sparse:
                        raise TypeError("a sparse gradient is not served")
                    if g.dtype != _f4 or g.device != p.device:
                        raise TypeError(f"a {g.dtype} gradient on {g.device} of a {p.dtype} parameter on {p.device}")
                    listed.append((slot, gi, p, g if g.is_contiguous() else g.contiguous()))
                slot += 1
        if not listed:
            return loss
        hyper = [(g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]) for g in self.param_groups]
        max_norm = 0.0 if self.max_norm is None else float(self.max_norm)
        skip = self.on_nonfinite == "skip"
        if buf.device.type == "cuda":
            self._step_device(buf, listed, hyper, max_norm, skip)
            torch.autograd.graph.increment_version([p for _, _, p, _ in listed])
        else:
            self._step_host(buf, listed, hyper, max_norm, skip)
        return loss

    def _step_device(self, buf: _Buffers, listed, hyper, max_norm: float, skip: bool):
        lib = optim_lib()
        key = tuple((i, gi, p.data_ptr(), g.data_ptr(), p.numel()) for i, gi, p, g in listed)
        if key != buf.key:
            n = [k[4] for k in key]
            lib.table_check(len(key), max(n), sum(n), len(hyper))
            tab, chunks = build_tables(key, [buf.m[k[0]].data_ptr() for k in key], [buf.v[k[0]].data_ptr() for k in key])
            buf.tensors, buf.chunks, buf.n_chunks = _upload(tab, buf.device), _upload(chunks, buf.device), len(chunks)
            buf.partials = torch.empty(max(len(chunks), 1), dtype=_f8, device=buf.device)
            buf.key = key
        with torch.cuda.device(buf.device):
            T, C = len(key), buf.n_chunks
            lib.sqnorm(buf.tensors, T, buf.chunks, C, buf.partials)
            lib.prepare(buf.tensors, T, buf.partials, C, hyper, max_norm, self.grad_scale,
                        PO_POLICY_SKIP if skip else PO_POLICY_PROPAGATE, buf.states, buf.scalars, buf.result, buf.step)
            lib.adamw(buf.tensors, T, buf.chunks, C, buf.scalars, buf.step)

    def _step_host(self, buf: _Buffers, listed, hyper, max_norm: float, skip: bool):
        partials = host.optim_sqnorm([g for _, _, _, g in listed])
        host.optim_prepare(partials, [(gi, i) for i, gi, _, _ in listed], hyper, max_norm, self.grad_scale, skip, buf.states,
                           buf.scalars, buf.result, buf.step)
        if int(buf.step[1]) == 0:
            return
        s = float(buf.step.view(_f4)[0])
        for i, _, p, g in listed:
            host.optim_adamw_(p, g, buf.m[i], buf.v[i], s, buf.scalars[i])

    # ---- torch.optim.AdamW's state dict ---------------------------------------------------------------------------------
    def state_dict(self):
        """`{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [...]}` as `torch.optim.AdamW` writes it: an entry
        for every parameter that has taken a step, the moments as copies.  Reads the step counts back (a synchronisation)."""
        buf = self._buffers()
        records = buf.get_states()
        self.state.clear()
        for i, p in enumerate(self._params()):
            if records["step"][i] > 0:
                self.state[p] = {"step": torch.tensor(float(records["step"][i])), "exp_avg": buf.m[i].clone(),
                                 "exp_avg_sq": buf.v[i].clone()}
        try:
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict):
        """Takes a state dict of this class or of `torch.optim.AdamW` (a reference checkpoint's `optimizer_states[0]`): the
        moments are copied into the flat buffer, beta^step is formed with fp64 `pow` on the host."""
        super().load_state_dict(state_dict)
        try:
            self._check_groups()
            self._buf = None
            buf = self._buffers()
            records = buf.get_states()
            slot = 0
            for group in self.param_groups:
                b1, b2 = group["betas"]
                for p in group["params"]:
                    st = self.state.get(p)
                    if st:
                        step = int(round(float(st["step"])))
                        buf.m[slot].copy_(st["exp_avg"]), buf.v[slot].copy_(st["exp_avg_sq"])
                        records[slot] = (step, math.pow(b1, step), math.pow(b2, step))
                    slot += 1
            buf.set_states(records)
        finally:
            self.state.clear()
