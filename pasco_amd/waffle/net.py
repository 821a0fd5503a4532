"""The WaffleIron segmenter (Puy et al., ICCV 2023) for inference on the pw_* kernels and the ph_conv_fwd product route.

`WaffleNet.load` takes the published checkpoint as it is (`ckpt["net"]`, with or without a `module.` prefix): the parameter
tree below carries exactly the reference's key names, and loading is strict - no missing and no unexpected key.

One layer is    tokens += s_sp * Inflate(DW3x3(ReLU(DW3x3(Flatten(BN(tokens))))))          pw_flatten, 2 x pw_dwconv3x3, pw_inflate
                tokens += s_ch * (W2 ReLU(W1 BN(tokens) + b1) + b2)                        two launches of the product route
with the eval-mode BatchNorms folded to scale / shift (`fused.fold_bn`).  The embedding's neighbourhood branch is built in
chunks of `EMBED_CHUNK` points: pw_neigh_rows writes [chunk * k, C] rows (both BatchNorms and the 5 -> C product folded into
one affine map), the C x C product over them runs on the product route, pw_group_max takes the maximum over the k rows of a
point.  Workspace of the embedding: two fp32 buffers of EMBED_CHUNK * k * C entries (2 x 128 MiB at k = 16, C = 256)."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
import torch.nn as nn

from ..graph import fused
from ..me.backend import ACT_NONE, ACT_RELU
from . import host

EMBED_CHUNK = 8192


class _Embedding(nn.Module):
    def __init__(self, cin: int, C: int):
        super().__init__()
        self.norm = nn.BatchNorm1d(cin)
        self.conv1 = nn.Conv1d(cin, C, 1)
        self.conv2 = nn.Sequential(nn.BatchNorm2d(cin), nn.Conv2d(cin, C, 1, bias=False), nn.BatchNorm2d(C),
                                   nn.ReLU(inplace=True), nn.Conv2d(C, C, 1, bias=False))
        self.final = nn.Conv1d(2 * C, C, 1)


class _ChannelMix(nn.Module):
    def __init__(self, C: int):
        super().__init__()
        self.norm = nn.BatchNorm1d(C)
        self.mlp = nn.Sequential(nn.Conv1d(C, C, 1), nn.ReLU(inplace=True), nn.Conv1d(C, C, 1))
        self.scale = nn.Conv1d(C, C, 1, bias=False, groups=C)


class _SpatialMix(nn.Module):
    def __init__(self, C: int):
        super().__init__()
        self.norm = nn.BatchNorm1d(C)
        self.ffn = nn.Sequential(nn.Conv2d(C, C, 3, padding=1, groups=C), nn.ReLU(inplace=True),
                                 nn.Conv2d(C, C, 3, padding=1, groups=C))
        self.scale = nn.Conv1d(C, C, 1, bias=False, groups=C)


class _Backbone(nn.Module):
    def __init__(self, C: int, depth: int):
        super().__init__()
        self.channel_mix = nn.ModuleList([_ChannelMix(C) for _ in range(depth)])
        self.spatial_mix = nn.ModuleList([_SpatialMix(C) for _ in range(depth)])


class _Segmenter(nn.Module):
    """Parameter tree with the reference's key names; it is never called as a module."""

    def __init__(self, cin: int, C: int, classes: int, depth: int):
        super().__init__()
        self.embed = _Embedding(cin, C)
        self.waffleiron = _Backbone(C, depth)
        self.classif = nn.Conv1d(C, classes, 1)


class _Lin:
    """One [cin] -> [cout] product: its fp32 weight both ways and, made on first use per device, its split operand."""

    def __init__(self, w: torch.Tensor, b: Optional[torch.Tensor]):
        self.w = w.detach().float().contiguous()               # [cout, cin]
        self.wt = self.w.t().contiguous()                      # [cin, cout]
        self.b = None if b is None else b.detach().float().contiguous()
        self._split = None

    def split(self, be):
        if self._split is None:
            self._split = fused._split_of(self.wt, be)
            fused.publish(self.wt)
        return self._split


def linear(x: torch.Tensor, lin: _Lin, *, pro=None, act: int = ACT_NONE, epi_scale: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, min_rows: Optional[int] = None,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """residual + epi_scale * act(lin(x * pro[0] + pro[1])) for a tall [N, cin] operand: one ph_conv_fwd launch (identity
    map, split-precision products where the shape allows them) from `fused.MIN_ROWS_LINEAR` rows up on the GPU, torch below
    that and on the CPU - the rule `fused.linear_bn_act` follows, with the epilogue scale and the residual it does not take."""
    n = x.shape[0]
    min_rows = fused.MIN_ROWS_LINEAR if min_rows is None else min_rows
    if not (fused.fusion() and fused._kernel_device(x.device) and n >= min_rows):
        y = x if pro is None else x * pro[0] + pro[1]
        y = torch.nn.functional.linear(y, lin.w, lin.b)
        y = torch.relu(y) if act == ACT_RELU else y
        y = y if epi_scale is None else y * epi_scale
        y = y if residual is None else y + residual
        if out is not None:
            out.copy_(y)
            y = out
        return y
    from ..me.backend import backend_for
    be = backend_for(x.device)
    cout, cin = lin.w.shape
    split = lin.split(be) if (fused.conv_precision() == "f16x3" and be.split_supported(cin, cout)) else None
    return be.conv_fwd(x.contiguous(), lin.wt, None, n, bias=lin.b, pro_scale=None if pro is None else pro[0],
                       pro_shift=None if pro is None else pro[1], epi_scale=epi_scale, epi_act=act, residual=residual,
                       split=split, out=out)


class WaffleNet:
    def __init__(self, state: dict, grids: Sequence[Sequence[int]], device="cuda"):
        state = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in state.items()}
        C, cin = (int(v) for v in state["embed.conv1.weight"].shape[:2])
        depth = 1 + max(int(k.split(".")[2]) for k in state if k.startswith("waffleiron.channel_mix."))
        classes = int(state["classif.weight"].shape[0])
        tree = _Segmenter(cin, C, classes, depth)
        missing, unexpected = tree.load_state_dict(state, strict=False)
        if missing or unexpected:
            raise KeyError(f"WaffleIron checkpoint: missing keys {list(missing)}, unexpected keys {list(unexpected)}")
        self.device = torch.device(device)
        self.modules_ = tree.float().eval().to(self.device)
        for p in self.modules_.parameters():
            p.requires_grad_(False)
        self.C, self.cin, self.depth, self.classes = C, cin, depth, classes
        self.grids = [tuple(int(v) for v in g) for g in grids]
        self._fold()

    @staticmethod
    def load(ckpt_path: str, grids, device="cuda") -> "WaffleNet":
        ckpt = torch.load(ckpt_path, map_location="cpu", weights_only=True)
        return WaffleNet(ckpt["net"] if "net" in ckpt else ckpt, grids, device)

    def _fold(self):
        m = self.modules_
        e = m.embed
        with torch.no_grad():
            s0, t0 = fused.fold_bn(e.norm)
            s1, t1 = fused.fold_bn(e.conv2[0])
            s2, t2 = fused.fold_bn(e.conv2[2])
            w1 = e.conv2[1].weight[:, :, 0, 0]                              # [C, F]
            # rows = ReLU(BN2(W1 BN1(BN0(x_j) - BN0(x_i)))) = ReLU(A^T (x_j - x_i) + b): BN0's shift cancels in the difference
            self.neigh_A = (w1 * (s1 * s0)[None] * s2[:, None]).t().contiguous()          # [F, C]
            self.neigh_b = (s2 * (w1 @ t1) + t2).contiguous()
            self.embed_norm = (s0, t0)
            self.conv1 = _Lin(e.conv1.weight[:, :, 0], e.conv1.bias)
            self.neigh_lin = _Lin(e.conv2[4].weight[:, :, 0, 0], None)
            self.final = _Lin(e.final.weight[:, :, 0], e.final.bias)
            self.classif = _Lin(m.classif.weight[:, :, 0], m.classif.bias)
            self.layers = []
            for sm, cm in zip(m.waffleiron.spatial_mix, m.waffleiron.channel_mix):
                self.layers.append({
                    "sp_norm": fused.fold_bn(sm.norm),
                    "w_a": sm.ffn[0].weight.reshape(self.C, 9).t().contiguous(), "b_a": sm.ffn[0].bias.contiguous(),
                    "w_b": sm.ffn[2].weight.reshape(self.C, 9).t().contiguous(), "b_b": sm.ffn[2].bias.contiguous(),
                    "sp_scale": sm.scale.weight.reshape(self.C).contiguous(),
                    "ch_norm": fused.fold_bn(cm.norm),
                    "mlp_a": _Lin(cm.mlp[0].weight[:, :, 0], cm.mlp[0].bias),
                    "mlp_b": _Lin(cm.mlp[2].weight[:, :, 0], cm.mlp[2].bias),
                    "ch_scale": cm.scale.weight.reshape(self.C).contiguous()})

    # ---- stages (tools/waffle_time.py times them one by one) -------------------------------------------------------------
    def embedding(self, feat: torch.Tensor, knn: torch.Tensor, status: torch.Tensor, min_rows=None) -> torch.Tensor:
        from .lib import waffle_lib
        L = waffle_lib()
        N, k, C = int(feat.shape[0]), int(knn.shape[1]), self.C
        both = torch.empty((N, 2 * C), dtype=torch.float32, device=feat.device)
        both[:, :C] = linear(feat, self.conv1, pro=self.embed_norm, min_rows=min_rows)
        chunk = min(N, EMBED_CHUNK)
        rows = torch.empty((chunk * k, C), dtype=torch.float32, device=feat.device)
        prod = torch.empty((chunk * k, C), dtype=torch.float32, device=feat.device)
        for p0 in range(0, N, chunk):
            n = min(chunk, N - p0)
            L.neigh_rows(feat, knn, p0, n, self.neigh_A, self.neigh_b, status, out=rows)
            y = linear(rows[:n * k], self.neigh_lin, min_rows=min_rows, out=prod[:n * k])
            L.group_max(y, n, k, both[p0:p0 + n, C:])
        return linear(both, self.final, min_rows=min_rows)

    def spatial_mix(self, tokens: torch.Tensor, layer: dict, csr, status: torch.Tensor, bufs) -> torch.Tensor:
        from .lib import waffle_lib
        L = waffle_lib()
        cell, start, order, (H, W) = csr
        ga, gb = bufs[0][:H * W], bufs[1][:H * W]
        L.flatten(tokens, layer["sp_norm"][0], layer["sp_norm"][1], start, order, H * W, status, out=ga)
        L.dwconv3x3(ga, H, W, layer["w_a"], layer["b_a"], True, out=gb)
        L.dwconv3x3(gb, H, W, layer["w_b"], layer["b_b"], False, out=ga)
        return L.inflate(tokens, layer["sp_scale"], ga, cell, status, out=tokens)

    def channel_mix(self, tokens: torch.Tensor, layer: dict, min_rows=None) -> torch.Tensor:
        hidden = linear(tokens, layer["mlp_a"], pro=layer["ch_norm"], act=ACT_RELU, min_rows=min_rows)
        return linear(hidden, layer["mlp_b"], epi_scale=layer["ch_scale"], residual=tokens, min_rows=min_rows)

    def forward(self, feat: torch.Tensor, cells, knn: torch.Tensor, min_rows: Optional[int] = None):
        """feat fp32 [N, F], cells = per grid (cell int32 [N], start int32 [H*W + 1], order int32 [N], (H, W)), knn int32
        [N, k] -> (embedding [N, C], tokens [N, C], logits [N, classes]) on the kernels.  Raises if a kernel met an index
        out of range or a product operand left the f16 range."""
        from .lib import waffle_lib
        assert feat.is_cuda and len(cells) == len(self.grids)
        status = waffle_lib().new_status(feat.device)
        with torch.no_grad():
            emb = self.embedding(feat.contiguous(), knn, status, min_rows)
            tokens = emb.clone()
            most = max(H * W for _, _, _, (H, W) in cells)
            bufs = [torch.empty((most, self.C), dtype=torch.float32, device=feat.device) for _ in range(2)]
            for d, layer in enumerate(self.layers):
                tokens = self.spatial_mix(tokens, layer, cells[d % len(cells)], status, bufs)
                tokens = self.channel_mix(tokens, layer, min_rows)
            logits = linear(tokens, self.classif, min_rows=min_rows)
        s = int(status.item())
        if s:
            raise RuntimeError(f"pw kernels: status {s} (an index out of range)")
        from ..me.backend import backend_for
        backend_for(feat.device).check_status(feat.device)
        return emb, tokens, logits

    def forward_host(self, feat: torch.Tensor, cells, knn: torch.Tensor):
        """The same network as `host.forward`'s plain torch formulation, on the device `feat` is on."""
        with torch.no_grad():
            return host.forward(self, feat, [(c[0], c[-1]) for c in cells], knn)
