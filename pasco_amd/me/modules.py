"""MinkowskiEngine-named nn.Modules served by the HIP library (SURVEY.md 8(b) census).

Parameter names/shapes follow upstream so reference checkpoints load: convolution `kernel`
[kvol, cin, cout] ([cin, cout] when kvol == 1) and `bias` [1, cout]; batch norm under `.bn.*`.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn

from . import backend as B
from .. import settings
from ..grad import field_ops, pool_ops
from ..grad.host import POOL_AVG, POOL_BC_ADD, POOL_BC_CAT, POOL_BC_COPY, POOL_BC_MUL, POOL_MAX, POOL_SUM
from ..grad.poollib import PP_MAX_BATCH, PP_MAX_KVOL
from .autograd import (BroadcastFunction, ChannelwiseConvFunction, ConvFunction, GatherRowsFunction, InterpolationFunction,
                       MaxPoolFunction, PoolFunction, PoolTransposeFunction, SegReduceFunction, gather_parents, wants_grad)
from .core import CoordinateManager, CoordinateMapKey, SparseTensor, TensorField, _triple, apply_prologue, derived


class MinkowskiModuleBase(nn.Module):
    pass


def _kvol(kernel_size) -> int:
    k = _triple(kernel_size)
    return k[0] * k[1] * k[2]


ME_MIN_ROWS_WINDOWS = 16384     # 3x3x3 maps with at least this many rows get window tables (as pasco_amd.graph.fused does)


def set_me_conv(mode: str) -> None:
    """"guarded" (default): the plain convolution modules run on the split-precision kernels with the exact fp32 kernel as a
    device-side fallback; "exact": the exact fp32 kernel only."""
    settings.replace(me_conv=mode)


def set_me_norm(mode: str) -> None:
    """"torch" (default): a training-mode `MinkowskiBatchNorm` is torch's batch_norm; "device": on fp32 GPU rows it is
    `pasco_amd.grad.norm.batch_norm_rows` (the pn_* kernels: fixed-order statistics).  `MinkowskiSyncBatchNorm`
    in a process group of more than one rank takes the pn_* route under either setting."""
    settings.replace(me_norm=mode)


class _ConvBase(MinkowskiModuleBase):
    is_transpose = False

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__()
        assert dimension == 3, "dimension=3 is the served case"
        assert kernel_generator is None, "custom kernel generators are not served"
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _triple(kernel_size)
        self.stride = _triple(stride)
        self.dilation = _triple(dilation)
        self.expand_coordinates = expand_coordinates
        self.kernel_volume = _kvol(kernel_size)
        self.dimension = dimension
        self.use_mm = self.kernel_volume == 1 and self.stride == (1, 1, 1)
        shape = (in_channels, out_channels) if self.kernel_volume == 1 else (self.kernel_volume, in_channels, out_channels)
        self.kernel = nn.Parameter(torch.empty(shape, dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty((1, out_channels), dtype=torch.float32)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():
            n = (self.out_channels if self.is_transpose else self.in_channels) * self.kernel_volume
            stdv = 1.0 / math.sqrt(n)
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    # out key + neighbour table for an input tensor
    def _maps(self, x: SparseTensor, coordinates=None):
        mgr = x.coordinate_manager
        in_key = x.coordinate_map_key
        assert coordinates is None or self.is_transpose, "explicit output coordinates are not served"
        if self.use_mm:
            assert coordinates is None, "explicit output coordinates are not served"
            return in_key, None
        if self.is_transpose and self.expand_coordinates:
            if coordinates is not None:
                raise ValueError("coordinates= names the existing map a transposed convolution lands on; with "
                                 "expand_coordinates=True the module generates its own output map")
            assert self.kernel_size == (2, 2, 2) and self.stride == (2, 2, 2), \
                "generative transposed convolution is served for kernel 2 / stride 2"
            out_key = mgr.expand(in_key, self.stride)
            nbr = mgr.kernel_map(in_key, out_key, self.kernel_size, self.dilation, transposed=True)
        elif self.is_transpose:
            if not (self.kernel_size == self.stride == (2, 2, 2)):
                raise ValueError(f"a transposed convolution onto an existing map (expand_coordinates=False) is served for "
                                 f"kernel_size == stride == 2, got kernel {list(self.kernel_size)}, stride {list(self.stride)}: "
                                 f"kernel != stride is not served")
            out_key = self._target(x, coordinates)
            # a child at parent + o_k * ts_out uses kernel[k], as the generative route; a target row without a parent has an
            # all-absent column (a zero row + bias), a parent without a child in the target appears in no column
            nbr = mgr.kernel_map(in_key, out_key, self.kernel_size, self.dilation, transposed=True)
        else:
            if self.stride != (1, 1, 1):
                assert self.kernel_size == self.stride, "strided convolution is served for kernel == stride"
            out_key = mgr.stride(in_key, self.stride)
            nbr = mgr.kernel_map(in_key, out_key, self.kernel_size, self.dilation, transposed=False)
        return out_key, nbr

    def _target(self, x: SparseTensor, coordinates) -> CoordinateMapKey:
        """The existing map a non-expanding transposed convolution writes: `coordinates` (a key of x's manager or a SparseTensor
        on it, at tensor stride in / stride) where given, else the map x's map was strided from."""
        mgr, in_key = x.coordinate_manager, x.coordinate_map_key
        if coordinates is None:
            return mgr.transposed_target(in_key, self.stride)
        key = coordinates
        if isinstance(coordinates, SparseTensor):
            if coordinates.coordinate_manager is not mgr:
                raise ValueError("coordinates=: the target tensor belongs to another coordinate manager than the input")
            key = coordinates.coordinate_map_key
        elif torch.is_tensor(coordinates):
            raise ValueError("coordinates=: a coordinate tensor is not served, pass the CoordinateMapKey of a map of the input's "
                             "manager or a SparseTensor on it")
        if not isinstance(key, CoordinateMapKey) or key not in mgr._maps:
            raise ValueError(f"coordinates=: {key!r} is no coordinate map of the input's manager (a key of another manager?)")
        want = tuple(t // a if t % a == 0 else -1 for t, a in zip(in_key.tensor_stride, self.stride))
        if tuple(key.tensor_stride) != want:
            raise ValueError(f"coordinates=: the target has tensor stride {list(key.tensor_stride)}, a stride-{list(self.stride)} "
                             f"transposed convolution of tensor stride {list(in_key.tensor_stride)} lands on {list(want)}")
        return key

    def forward(self, x: SparseTensor, coordinates=None) -> SparseTensor:
        assert isinstance(x, SparseTensor)
        out_key, nbr = self._maps(x, coordinates)
        mgr = x.coordinate_manager
        raw, pending = x.take_prologue()
        if pending is not None and wants_grad(raw, self.kernel, self.bias):
            raw, pending = x.F, None          # the backward needs the operand itself: apply what is pending, once, on the tensor
        out = self.conv_rows(mgr.backend(), raw, nbr, mgr.size(out_key), mgr=mgr, prologue=pending)
        return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=mgr)

    def conv_rows(self, be, feats: torch.Tensor, nbr, n_out: int, mgr=None, prologue=None) -> torch.Tensor:
        """The module's own launch(es): exact fp32 results, as upstream's.  Where the split-precision kernels apply (GPU,
        cin % 8 == 0) the products run on them GUARDED: the operand split reports an f16 range overflow (|x| > 2047) into a
        word of this call, and the exact fp32 kernel is launched behind the split one with that word as its predicate
        (`ph_conv_desc.exact_if`): it replaces the result exactly when it has to and costs an empty launch otherwise.  No
        host read, nothing for the caller to check - a maintainer who only swaps the import gets the fast kernels (round 5:
        the exact fp32 MFMA runs at 1 / 16 of the f16 rate and was ~85 % of the unfused route's time).
        `settings.me_conv == "exact"` (`PASCO_ME_CONV=exact` or `set_me_conv("exact")`): the exact kernel only.
        `prologue` = (scale, shift, act, slope) of a deferred BatchNorm / activation in front (SparseTensor.deferred): applied
        to the gathered rows by the launch itself instead of by separate passes over the tensor.
        With autograd enabled and features, kernel or bias requiring grad the same launches run inside
        `autograd.ConvFunction`, which gives the result its `grad_fn` (backward: include/pasco_grad.h).  A pending prologue
        is then applied first (torch operations, differentiable down to the raw rows): the weight gradient needs the operand
        the products saw, not the raw rows."""
        if torch.is_grad_enabled():
            exact = self.kernel.requires_grad and self.training
            if wants_grad(feats, self.kernel, self.bias):
                if prologue is not None:
                    feats = apply_prologue(feats, prologue)
                return ConvFunction.apply(feats, self.kernel, self.bias,
                                          lambda f: self._launch(be, f, nbr, n_out, mgr, None, exact), be, nbr, n_out, mgr)
            return self._launch(be, feats, nbr, n_out, mgr, prologue, exact)
        return self._launch(be, feats, nbr, n_out, mgr, prologue, False)

    def _launch(self, be, feats: torch.Tensor, nbr, n_out: int, mgr, prologue, exact: bool) -> torch.Tensor:
        """The launches of `conv_rows` on detached parameters; `exact` = a training-mode kernel that requires grad, seen with
        autograd enabled: the exact fp32 route only."""
        feats = feats.contiguous()
        kernel = self.kernel.detach().contiguous()
        bias = self.bias.detach().reshape(-1).contiguous() if self.bias is not None else None
        pro = {}
        if prologue is not None:
            ps, pb, pact, pslope = prologue
            pro = dict(pro_scale=ps, pro_shift=pb, pro_act=pact, slope=pslope)
        if n_out == 0 or settings.current().me_conv != "guarded" or not be.split_supported(self.in_channels, self.out_channels) or exact:
            return be.conv_fwd(feats, kernel, nbr, n_out, bias=bias, **pro)
        # the same cache, under the same rule, as the fused graph's entries (`derived`: valid while the kernel is the same
        # object at the same version counter); a kernel made under torch.inference_mode() has no counter: split every call
        w_split = derived(self, "_ph_me_split", (self.kernel,), None, lambda: be.split_weight_rows(kernel), identity_suffices=False)
        flag = torch.zeros(1, dtype=torch.int32, device=feats.device)
        xs = be.split_rows(feats, status=flag, **pro)
        win = None
        if mgr is not None and nbr is not None and nbr.shape[0] == 27 and 33 <= self.out_channels <= 64 and \
                n_out >= ME_MIN_ROWS_WINDOWS and be.device_type == "cuda":
            win = mgr.kernel_windows(nbr)       # LDS-window tables of the map (cached by the manager): k_conv_wop2
        out = be.conv_fwd(feats, kernel, nbr, n_out, bias=bias, split=w_split, in_split=xs, status=flag, win=win)
        be.conv_fwd(feats, kernel, nbr, n_out, bias=bias, out=out, exact_if=flag, **pro)
        return out

    def extra_repr(self):
        return (f"in={self.in_channels}, out={self.out_channels}, kernel_size={list(self.kernel_size)}, "
                f"stride={list(self.stride)}, dilation={list(self.dilation)}")


class MinkowskiConvolution(_ConvBase):
    """reference: mink.py:509-511,625-638; encoder_v2.py:109-111; decoder_v3.py:103-105,133-135,267-282"""
    is_transpose = False


class MinkowskiConvolutionTranspose(_ConvBase):
    """reference: mink.py:524-527 (kernel 2, stride 2, expand_coordinates=True) and mink.py:537-543 (kernel 2, stride 2 onto the
    encoder's map: without expand_coordinates the output lands on the map the input's map was strided from, or on the map
    `forward(x, coordinates=key | tensor on it)` names; out[child] = x[parent] @ kernel[k] + bias for the child at
    parent + o_k * ts_out, the generative module's convention)"""
    is_transpose = True

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, kernel_generator,
                         expand_coordinates, convolution_mode, dimension)


class MinkowskiGenerativeConvolutionTranspose(MinkowskiConvolutionTranspose):
    def __init__(self, *a, **kw):
        kw["expand_coordinates"] = True
        super().__init__(*a, **kw)


# ---- normalisation / activations: wrappers over torch.nn on F, same key -------------
def _same_map(x: SparseTensor, feats: torch.Tensor) -> SparseTensor:
    return SparseTensor(feats, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)


_GRAD_MODE_WARNED = False


def _warn_grad_mode_once() -> None:
    """An eval-mode module called with autograd ENABLED takes the module-by-module route (separate BatchNorm / activation passes,
    exact fp32 products where a parameter requires grad): the results are the same, the speed is not ('a caller who
    forgets torch.no_grad() silently gets the slow route').  Said once per process."""
    global _GRAD_MODE_WARNED
    if not _GRAD_MODE_WARNED:
        _GRAD_MODE_WARNED = True
        import warnings
        warnings.warn("pasco_amd.me: eval-mode modules called with autograd enabled - the fused inference route (deferred BatchNorm / "
                      "activations, split-precision convolutions) needs torch.no_grad() / torch.inference_mode(); running the "
                      "module-by-module route", RuntimeWarning, stacklevel=3)


class MinkowskiBatchNorm(nn.Module):
    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)

    def folded(self):
        """(scale, shift) of the eval-mode normalisation, y = x * scale + shift; cached per parameter version."""
        m = self.bn
        bufs, pars = m._buffers, m._parameters
        rm, rv, w, b = bufs["running_mean"], bufs["running_var"], pars.get("weight"), pars.get("bias")
        # a training-mode forward updates the running statistics inside the op without moving their version counters; the
        # module advances num_batches_tracked itself (an in-place add_), so its counter stands for them
        def build():
            with torch.no_grad():
                scale = torch.rsqrt(rv.float() + m.eps) * (w.float() if w is not None else 1.0)
                shift = (b.float() if b is not None else 0.0) - rm.float() * scale
                return scale.contiguous(), shift.contiguous()

        # inference tensors have no counter: fold every call
        return derived(self, "_ph_me_folded", (rm, rv, w, b, bufs.get("num_batches_tracked")), None, build, identity_suffices=False)

    def forward(self, x: SparseTensor) -> SparseTensor:
        m, defer = self.bn, settings.current().me_defer
        if defer and not m.training and torch.is_grad_enabled():
            _warn_grad_mode_once()
        if defer and not m.training and m.track_running_stats and m._buffers.get("running_mean") is not None \
                and not torch.is_grad_enabled() and x._F.dtype == torch.float32:
            if x._pending is not None:
                x.F                        # an activation is pending: it has to be applied before this affine
            scale, shift = self.folded()
            return SparseTensor.deferred(x, scale, shift, B.ACT_NONE, 0.01)
        if m.training:                     # the running statistics move: no fold made before this call stands for them
            self.__dict__.pop("_ph_me_folded", None)
            m.__dict__.pop("_ph_folded", None)
            use, gather = self._rows_route(x.F)
            if use:
                from ..grad.norm import batch_norm_rows
                return _same_map(x, batch_norm_rows(x.F, m.weight, m.bias, m.running_mean, m.running_var, m.num_batches_tracked,
                                                    m.momentum, m.eps, gather=gather))
        return _same_map(x, self.bn(x.F))

    def _rows_route(self, feats: torch.Tensor):
        """-> (a training-mode forward goes through `batch_norm_rows`, its `gather`)."""
        return settings.current().me_norm == "device" and feats.is_cuda and feats.dtype == torch.float32, None


class MinkowskiSyncBatchNorm(MinkowskiBatchNorm):
    """Batch normalisation whose training-mode mean and variance are taken over the rows of ALL ranks of `process_group`
    (reference: unet3d_sparse_v2.py:172-175 converts the whole encoder and decoder and trains with one scene per GPU).  Same
    state-dict keys as `MinkowskiBatchNorm`.

    In training mode, with torch.distributed initialised and more than one rank in the group (torch.nn.SyncBatchNorm's own
    condition), the forward is `pasco_amd.grad.norm.batch_norm_rows` with `group_gather(process_group)`: one all-gather of the
    moments record per forward, one of the gradient sums per backward, the same statistics bit for bit on every rank.  EVERY
    rank has to call the module (a rank without rows passes its `[0, c]` tensor).  Otherwise - eval mode, no process group, one
    rank - it is `MinkowskiBatchNorm`."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, process_group=None):
        super().__init__(num_features, eps, momentum, affine, track_running_stats)
        self.process_group = process_group

    def _rows_route(self, feats: torch.Tensor):
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1:
            from ..grad.norm import group_gather
            return True, group_gather(self.process_group)
        return super()._rows_route(feats)

    @classmethod
    def convert_sync_batchnorm(cls, module, process_group=None):
        out = module
        if isinstance(module, MinkowskiBatchNorm) and not isinstance(module, MinkowskiSyncBatchNorm):
            out = cls(module.bn.num_features, module.bn.eps, module.bn.momentum, module.bn.affine,
                      module.bn.track_running_stats, process_group)
            out.bn.load_state_dict(module.bn.state_dict())
            out.train(module.training)
        for name, child in module.named_children():
            out.add_module(name, cls.convert_sync_batchnorm(child, process_group))
        return out


class _Elementwise(MinkowskiModuleBase):
    MODULE = None

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.module = self.MODULE(*args, **kwargs)

    def forward(self, x: SparseTensor) -> SparseTensor:
        return _same_map(x, self.module(x.F))


class _DeferredAct(_Elementwise):
    """ReLU / LeakyReLU: in inference the activation is recorded on the returned tensor (SparseTensor.deferred) and applied
    by the next convolution's operand prologue, or the first time anything else reads the values."""
    ACT = B.ACT_NONE

    def forward(self, x: SparseTensor) -> SparseTensor:
        if settings.current().me_defer and not torch.is_grad_enabled() and x._F.dtype == torch.float32:
            slope = float(getattr(self.module, "negative_slope", 0.01))
            if x._pending is not None and x._pending[2] == B.ACT_NONE:      # behind a deferred BatchNorm: one prologue
                raw, (scale, shift, _, _) = x.take_prologue()
                src = SparseTensor(raw, coordinate_map_key=x.coordinate_map_key, coordinate_manager=x.coordinate_manager)
                return SparseTensor.deferred(src, scale, shift, self.ACT, slope)
            x.F                                                             # (materialises whatever else is pending)
            return SparseTensor.deferred(x, None, None, self.ACT, slope)
        return _same_map(x, self.module(x.F))


class MinkowskiReLU(_DeferredAct):
    MODULE = nn.ReLU
    ACT = B.ACT_RELU


class MinkowskiLeakyReLU(_DeferredAct):
    MODULE = nn.LeakyReLU
    ACT = B.ACT_LEAKY


class MinkowskiSigmoid(_Elementwise):
    MODULE = nn.Sigmoid


class MinkowskiSoftmax(_Elementwise):
    MODULE = nn.Softmax


class MinkowskiELU(_Elementwise):
    MODULE = nn.ELU


class MinkowskiDropout(_Elementwise):
    MODULE = nn.Dropout


class MinkowskiLinear(MinkowskiModuleBase):
    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, x: SparseTensor) -> SparseTensor:
        return _same_map(x, self.linear(x.F))


# ---- pruning / pooling -------------------------------------------------------------------------
class MinkowskiPruning(MinkowskiModuleBase):
    """reference: decoder_v3.py:127,159,285,421-432,496-497; misc.py:17,26"""

    def forward(self, x: SparseTensor, mask: torch.Tensor) -> SparseTensor:
        assert isinstance(x, SparseTensor)
        assert mask.dim() == 1 and mask.shape[0] == x.F.shape[0], "mask must be [N]"
        if mask.dtype != torch.bool:
            mask = mask != 0
        mgr = x.coordinate_manager
        out_key, keep = mgr.prune(x.coordinate_map_key, mask.to(x.device))
        if wants_grad(x.F):
            feats = GatherRowsFunction.apply(x.F, keep, mgr.backend())
        else:
            feats = mgr.backend().gather_rows(x.F.contiguous(), keep)
        return SparseTensor(feats, coordinate_map_key=out_key, coordinate_manager=mgr)


class MinkowskiMaxPooling(MinkowskiModuleBase):
    """reference: transformer_predictor_v2.py:100-102,234-236 (kernel == stride)"""

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None):
        super().__init__()
        assert dimension == 3 and kernel_generator is None
        self.kernel_size = _triple(kernel_size)
        self.stride = _triple(stride)
        self.dilation = _triple(dilation)
        assert self.kernel_size[0] ** 3 <= B.MAX_KVOL, "pooling window too large"

    def forward(self, x: SparseTensor) -> SparseTensor:
        mgr = x.coordinate_manager
        out_key = mgr.stride(x.coordinate_map_key, self.stride)
        nbr = mgr.kernel_map(x.coordinate_map_key, out_key, self.kernel_size, self.dilation)
        if wants_grad(x.F):
            out = MaxPoolFunction.apply(x.F, nbr, mgr.backend(), mgr)
        else:
            out = mgr.backend().maxpool_fwd(x.F.contiguous(), nbr)
        return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=mgr)


# ---- pooling, broadcast and channel-wise operators (include/pasco_pool.h) -------------------------------------------------------
def _served_pool_kernel(name: str, kernel_size, stride, dilation, kernel_generator, dimension):
    """The sizes of a pooling / channel-wise module as triples, refused outside the served range (that of `MinkowskiMaxPooling`
    and `MinkowskiConvolution`: dimension 3, no kernel generator, a cubic kernel of at most PP_MAX_KVOL offsets, stride 1 with an
    odd kernel or kernel == stride)."""
    if dimension != 3:
        raise ValueError(f"{name}: dimension=3 is the served case, got {dimension}")
    if kernel_generator is not None:
        raise ValueError(f"{name}: custom kernel generators are not served")
    ks, st, dl = _triple(kernel_size), _triple(stride), _triple(dilation)
    if not (ks[0] == ks[1] == ks[2] and st[0] == st[1] == st[2]):
        raise ValueError(f"{name}: cubic kernels and isotropic strides are served, got kernel {list(ks)}, stride {list(st)}")
    if _kvol(ks) > PP_MAX_KVOL:
        raise ValueError(f"{name}: a window of {_kvol(ks)} offsets, at most {PP_MAX_KVOL} (PP_MAX_KVOL) are served")
    if st == (1, 1, 1):
        if ks[0] % 2 == 0:
            raise ValueError(f"{name}: a stride-1 kernel must be odd, got {list(ks)}")
    elif ks != st:
        raise ValueError(f"{name}: a strided kernel is served for kernel == stride, got kernel {list(ks)}, stride {list(st)}")
    return ks, st, dl


def _pool_rows(x: SparseTensor) -> torch.Tensor:
    """The features a pooling / broadcast module works on: a pending prologue is applied by reading `x.F`; on the device
    anything but fp32 is refused."""
    feats = x.F
    if feats.is_cuda and feats.dtype != torch.float32:
        raise TypeError(f"pasco_amd.me serves fp32 rows on the device, got {feats.dtype}")
    return feats


class _GlobalPooling(MinkowskiModuleBase):
    """[n, c] rows -> one row per batch index 0 .. B - 1 (B = the largest batch index + 1) on the origin map of the input's
    map: coordinates (b, 0, 0, 0), tensor stride [0, 0, 0].  A batch index without rows gives a zero row."""
    MODE = POOL_AVG

    def __init__(self, mode=None):          # upstream's PoolingMode argument: the served arithmetic does not depend on it
        super().__init__()

    def forward(self, x: SparseTensor, coordinates=None) -> SparseTensor:
        assert isinstance(x, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not served"
        mgr = x.coordinate_manager
        out_key, nb = mgr.origin(x.coordinate_map_key)
        if nb > PP_MAX_BATCH:
            raise ValueError(f"{type(self).__name__}: {nb} batch indices, at most {PP_MAX_BATCH} (PP_MAX_BATCH) are served")
        feats = _pool_rows(x)
        if wants_grad(feats):
            out = SegReduceFunction.apply(feats, x.C, nb, self.MODE)
        else:
            out = pool_ops(feats).seg_reduce(feats.contiguous(), x.C, nb, self.MODE)[0]
        return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=mgr)


class MinkowskiGlobalSumPooling(_GlobalPooling):
    MODE = POOL_SUM


class MinkowskiGlobalAvgPooling(_GlobalPooling):
    """reference: mink.py:27,40-42,53-75 (ASPP, SELayer); decoder_v3.py:46-74"""
    MODE = POOL_AVG


class MinkowskiGlobalMaxPooling(_GlobalPooling):
    MODE = POOL_MAX


class MinkowskiGlobalPooling(MinkowskiGlobalAvgPooling):
    """Upstream's default global pooling: the average."""


class _Broadcast(MinkowskiModuleBase):
    """forward(x, g): `g` holds one row per batch index (a global pooling's output); the result lives on x's map."""
    MODE = POOL_BC_COPY

    def forward(self, x: SparseTensor, g: SparseTensor) -> SparseTensor:
        assert isinstance(x, SparseTensor) and isinstance(g, SparseTensor)
        mgr = x.coordinate_manager
        feats, glob = _pool_rows(x), _pool_rows(g)
        nb = glob.shape[0]
        if nb > PP_MAX_BATCH:
            raise ValueError(f"{type(self).__name__}: {nb} batch indices, at most {PP_MAX_BATCH} (PP_MAX_BATCH) are served")
        have = mgr.batch_count(x.coordinate_map_key)
        if x.F.shape[0] and have > nb:
            raise ValueError(f"{type(self).__name__}: the input has batch index {have - 1}, the global tensor has {nb} rows")
        if self.MODE in (POOL_BC_ADD, POOL_BC_MUL) and glob.shape[1] != feats.shape[1]:
            raise ValueError(f"{type(self).__name__}: {feats.shape[1]} channels against {glob.shape[1]} of the global tensor")
        rows = None if self.MODE == POOL_BC_COPY else feats
        if wants_grad(rows, glob):
            out = BroadcastFunction.apply(rows, glob, x.C, self.MODE)
        else:
            out = pool_ops(glob).broadcast(None if rows is None else rows.contiguous(), glob.contiguous(), x.C, self.MODE)
        return _same_map(x, out)


class MinkowskiBroadcast(_Broadcast):
    MODE = POOL_BC_COPY


class MinkowskiBroadcastAddition(_Broadcast):
    MODE = POOL_BC_ADD


class MinkowskiBroadcastMultiplication(_Broadcast):
    """reference: mink.py:53-75 (SELayer); decoder_v3.py:46-74"""
    MODE = POOL_BC_MUL


class MinkowskiBroadcastConcatenation(_Broadcast):
    MODE = POOL_BC_CAT


class _LocalPooling(MinkowskiModuleBase):
    """Sum / average over the maps and tables of `MinkowskiMaxPooling`.  The average divides by the number of neighbours that
    EXIST (upstream's definition), not by the kernel volume."""
    MODE = POOL_SUM

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None):
        super().__init__()
        self.kernel_size, self.stride, self.dilation = _served_pool_kernel(type(self).__name__, kernel_size, stride, dilation,
                                                                           kernel_generator, dimension)

    def forward(self, x: SparseTensor, coordinates=None) -> SparseTensor:
        assert isinstance(x, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not served"
        mgr = x.coordinate_manager
        out_key = mgr.stride(x.coordinate_map_key, self.stride)
        nbr = mgr.kernel_map(x.coordinate_map_key, out_key, self.kernel_size, self.dilation)
        feats = _pool_rows(x)
        if wants_grad(feats):
            out = PoolFunction.apply(feats, nbr, self.MODE, mgr)
        else:
            out = pool_ops(feats).pool(feats.contiguous(), nbr, self.MODE)[0]
        return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=mgr)


class MinkowskiSumPooling(_LocalPooling):
    MODE = POOL_SUM


class MinkowskiAvgPooling(_LocalPooling):
    MODE = POOL_AVG


class MinkowskiPoolingTranspose(MinkowskiModuleBase):
    """reference: layers.py:264-276 (DepthwiseUpsample).  Served like the transposed convolutions: kernel 2, stride 2,
    expand_coordinates=True, onto `mgr.expand(in_key, 2)`.  Every child then has exactly one parent and upstream's division by
    the number of contributors is a division by one: out[child] = x[parent]."""

    def __init__(self, kernel_size, stride, dilation=1, kernel_generator=None, expand_coordinates=False, dimension=None):
        super().__init__()
        if dimension != 3:
            raise ValueError(f"MinkowskiPoolingTranspose: dimension=3 is the served case, got {dimension}")
        if kernel_generator is not None:
            raise ValueError("MinkowskiPoolingTranspose: custom kernel generators are not served")
        if not expand_coordinates:
            raise ValueError("MinkowskiPoolingTranspose: pooling transpose is served with expand_coordinates=True")
        self.kernel_size, self.stride, self.dilation = _triple(kernel_size), _triple(stride), _triple(dilation)
        if self.kernel_size != (2, 2, 2) or self.stride != (2, 2, 2):
            raise ValueError(f"MinkowskiPoolingTranspose: pooling transpose is served for kernel 2 / stride 2, got kernel "
                             f"{list(self.kernel_size)}, stride {list(self.stride)}")

    def forward(self, x: SparseTensor, coordinates=None) -> SparseTensor:
        assert isinstance(x, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not served"
        mgr = x.coordinate_manager
        in_key = x.coordinate_map_key
        out_key = mgr.__dict__.setdefault("_expand_cache", {}).get(in_key)
        if out_key is None:                     # one child map per parent map, as a strided map is cached per input map
            out_key = mgr.__dict__["_expand_cache"][in_key] = mgr.expand(in_key, self.stride)
        nbr = mgr.kernel_map(in_key, out_key, self.kernel_size, self.dilation, transposed=True)
        parent = mgr.transpose_parents(nbr)
        feats = _pool_rows(x)
        if wants_grad(feats):
            out = PoolTransposeFunction.apply(feats, parent, nbr, mgr.backend(), mgr)
        else:
            out = gather_parents(feats.contiguous(), parent, mgr.backend())
        return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=mgr)


class MinkowskiChannelwiseConvolution(MinkowskiModuleBase):
    """reference: layers.py:178-191 (DepthwiseSeparableConvMultiheads).  out[o][ch] = sum_k x[nbr[k][o]][ch] * kernel[k][ch]
    (+ bias[ch]) over the maps of `MinkowskiConvolution`; parameters `kernel` [kvol, C] and `bias` [1, C] as upstream's."""

    def __init__(self, in_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None, dimension=None):
        super().__init__()
        self.kernel_size, self.stride, self.dilation = _served_pool_kernel("MinkowskiChannelwiseConvolution", kernel_size, stride,
                                                                           dilation, kernel_generator, dimension)
        self.in_channels = self.out_channels = in_channels
        self.kernel_volume = _kvol(self.kernel_size)
        self.dimension = dimension
        self.kernel = nn.Parameter(torch.empty((self.kernel_volume, in_channels), dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty((1, in_channels), dtype=torch.float32)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        with torch.no_grad():           # as `_ConvBase.reset_parameters`
            stdv = 1.0 / math.sqrt(self.in_channels * self.kernel_volume)
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def forward(self, x: SparseTensor, coordinates=None) -> SparseTensor:
        assert isinstance(x, SparseTensor)
        assert coordinates is None, "explicit output coordinates are not served"
        mgr = x.coordinate_manager
        out_key = mgr.stride(x.coordinate_map_key, self.stride)
        nbr = mgr.kernel_map(x.coordinate_map_key, out_key, self.kernel_size, self.dilation)
        feats = _pool_rows(x)
        if feats.shape[1] != self.in_channels:
            raise ValueError(f"MinkowskiChannelwiseConvolution: {feats.shape[1]} channels, the kernel has {self.in_channels}")
        if wants_grad(feats, self.kernel, self.bias):
            out = ChannelwiseConvFunction.apply(feats, self.kernel, self.bias, nbr, mgr)
        else:
            bias = None if self.bias is None else self.bias.detach().reshape(-1).contiguous()
            out = pool_ops(feats).chconv_fwd(feats.contiguous(), nbr, self.kernel.detach().contiguous(), bias)
        return SparseTensor(out, coordinate_map_key=out_key, coordinate_manager=mgr)

    def extra_repr(self):
        return (f"channels={self.in_channels}, kernel_size={list(self.kernel_size)}, stride={list(self.stride)}, "
                f"dilation={list(self.dilation)}")


class MinkowskiInterpolation(MinkowskiModuleBase):
    """forward(input, tfield): the features of `input` at the points `tfield` [M, 4] = (b, x, y, z), linearly interpolated over the
    eight voxels around each point -> [M, C] (a plain tensor, as upstream).  The weights are not renormalised over the corners
    that exist: a point next to missing voxels gets a smaller row, a point with none a zero row.  `return_kernel_map` /
    `return_weights` add the corner rows int32 [8, M] (-1: absent) / the weights [8, M] to the result."""

    def __init__(self, return_kernel_map=False, return_weights=False):
        super().__init__()
        self.return_kernel_map, self.return_weights = bool(return_kernel_map), bool(return_weights)

    def forward(self, input: SparseTensor, tfield: torch.Tensor):
        assert isinstance(input, SparseTensor)
        assert isinstance(tfield, torch.Tensor) and tfield.dim() == 2 and tfield.shape[1] == 4, "tfield must be [M, 4] (b,x,y,z)"
        mgr, key = input.coordinate_manager, input.coordinate_map_key
        ts = key.tensor_stride
        if not (ts[0] == ts[1] == ts[2] and ts[0] >= 1):
            raise ValueError(f"MinkowskiInterpolation: isotropic tensor strides >= 1 are served, got {list(ts)}")
        feats = _pool_rows(input)
        ops = field_ops(feats)
        cmap = mgr._maps[key]
        points = tfield.to(device=feats.device, dtype=feats.dtype).contiguous()
        rows, weights = ops.interp_map(points, cmap.tkeys, cmap.tvals, ts[0])
        if wants_grad(feats):
            out = InterpolationFunction.apply(feats, rows, weights)
        else:
            out = ops.interp_fwd(feats.contiguous(), rows, weights)
        extra = ((rows,) if self.return_kernel_map else ()) + ((weights,) if self.return_weights else ())
        return (out,) + extra if extra else out


def cat(*tensors):
    """Channel concat of sparse tensors sharing one coordinate map."""
    if len(tensors) == 1 and isinstance(tensors[0], (list, tuple)):
        tensors = tuple(tensors[0])
    k0 = tensors[0].coordinate_map_key
    assert all(t.coordinate_map_key == k0 for t in tensors), "cat needs one shared coordinate map"
    return _same_map(tensors[0], torch.cat([t.F for t in tensors], dim=1))
