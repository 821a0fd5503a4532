"""k-nearest-neighbour up-sampling of voxel rows onto points: `knn_up`, `kNN` and `index_points` under the names and signatures a
MaskPLS-style segmenter imports from its `interpolate` module, so that

    sys.modules["pasco.maskpls.interpolate"] = pasco_amd.grad.knn

before that network's module is imported serves it.  Every point's row is the inverse-squared-distance
weighted mean of the rows of its k nearest voxels.

On a GPU the search is `pk_knn` (include/pasco_knn.h): exact under the header's ordering rule (fp32 squared distances, ties to the
lower voxel index), over a uniform grid instead of the all-pairs pass; fp32 only, another dtype is a `TypeError`.  CPU tensors of
any floating dtype run `pasco_amd.grad.host` (brute force under the same rule).  One call performs ONE host read on the device
route: the voxels' bounding box, which sizes the search grid (a host-side number) and doubles as the check that every voxel
coordinate is finite (a `ValueError` otherwise).  The grid is not cached between calls.

The gradient goes to the voxel rows only (the coordinates get none, as in the module this stands in for): `KnnInterpFunction`
performs the same launches with and without autograd, so the forward values are the same bits under `no_grad`,
`inference_mode` and autograd; its backward adds the terms of a voxel row in ascending (neighbour rank, point) order."""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import host
from ..waffle.host import SearchGrid

MAX_CELLS = 1 << 22             # cells of one search grid
MAX_VOXELS = 1 << 24            # voxels of one device search: the list entries pq_group serves (pk_knn itself takes n < 2^31)


class _HostKnn:
    """`host.knn_*` under the method names of `knnlib.KnnLib`."""
    weights = staticmethod(host.knn_weights)
    interp_fwd = staticmethod(host.knn_interp)
    interp_bwd = staticmethod(host.knn_interp_bwd)


_HOST_KNN = _HostKnn()


def knn_ops(t: torch.Tensor):
    """What serves the include/pasco_knn.h operators for `t`: the `pk_*` binding on a GPU (fp32 only), `host` otherwise."""
    if t.is_cuda:
        if t.dtype != torch.float32:
            raise TypeError(f"the k-nearest-neighbour kernels serve fp32 coordinates and rows on the device, got {t.dtype}")
        from .knnlib import knn_lib
        return knn_lib()
    if not t.is_floating_point():
        raise TypeError(f"k-nearest-neighbour up-sampling takes floating-point coordinates and rows, got {t.dtype}")
    return _HOST_KNN


def search_grid(mn, mx, n: int) -> SearchGrid:
    """The grid over a cloud of `n` points with per-axis minimum `mn` and maximum `mx`: about one cell per point over the
    bounding box (an axis without extent counts as a thousandth of the longest one), at most MAX_CELLS cells."""
    ext = [float(b) - float(a) for a, b in zip(mn, mx)]
    top = max(ext)
    if not top > 0.0:
        return SearchGrid(tuple(float(v) for v in mn), 1.0, (1, 1, 1))
    vol = 1.0
    for e in ext:
        vol *= max(e, 1e-3 * top)
    return SearchGrid.around(mn, mx, (vol / max(int(n), 1)) ** (1.0 / 3.0), MAX_CELLS)


def _xyz(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"{what}: [N, 3] coordinates, got {list(t.shape)}")
    return t.detach()


def knn_search(v_coor: torch.Tensor, p_coor: torch.Tensor, k: int):
    """-> (idx int32 [k, m], d2 [k, m]): the k nearest voxels of every point, nearest first (include/pasco_knn.h's ordering rule);
    idx = -1 / d2 = +inf where there are fewer than k voxels or the point has a non-finite coordinate.  A non-finite voxel
    coordinate is a `ValueError`.  On the device: one host read (see the module docstring), and fewer than 2^24 voxels (the
    CSR is built by `pq_group`; a `ValueError` that says so above)."""
    v, p = _xyz(v_coor, "v_coor"), _xyz(p_coor, "p_coor")
    ops = knn_ops(v)
    if p.device != v.device or p.dtype != v.dtype:
        raise TypeError(f"v_coor is {v.dtype} on {v.device}, p_coor {p.dtype} on {p.device}: one device and one dtype")
    n = int(v.shape[0])
    if ops is _HOST_KNN:
        if n and not bool(torch.isfinite(v).all()):
            raise ValueError("v_coor: a voxel coordinate is not finite")
        return host.knn_search(v, p, k)
    if n >= MAX_VOXELS:
        raise ValueError(f"knn_up / kNN: {n} voxels, fewer than 2^24 are served on the device (the cells are grouped by pq_group)")
    if v.stride(1) != 1:
        v = v.contiguous()
    if p.stride(1) != 1:
        p = p.contiguous()
    if n == 0:
        g = SearchGrid((0.0, 0.0, 0.0), 1.0, (1, 1, 1))
        start = torch.zeros(2, dtype=torch.int32, device=v.device)
        order = torch.zeros(0, dtype=torch.int32, device=v.device)
    else:
        box = torch.stack(torch.aminmax(v, dim=0)).cpu()                       # the one host read (a NaN poisons its column)
        if not bool(torch.isfinite(box).all()):
            raise ValueError("v_coor: a voxel coordinate is not finite")
        g = search_grid(box[0].tolist(), box[1].tolist(), n)
        # every voxel lies in the grid by construction (the same fp64 expression sizes it and places a point): the status
        # word the cell kernel ORs into is not read back
        start, order = ops.csr(v, g, torch.zeros(1, dtype=torch.int32, device=v.device))
    return ops.knn(v, start, order, g, p, k)


class KnnInterpFunction(torch.autograd.Function):
    """out[p] = sum_j w[j][p] * x[idx[j][p]] (`ops.interp_fwd`).  Backward: the [k, M] table flattened is a list of k M entries
    keyed by voxel row; grouped, the terms w[j][p] * dy[p] of every voxel row are added in ascending (j, p) (`ops.interp_bwd`).
    No gradient goes to the table or the weights."""

    @staticmethod
    def forward(ctx, x, idx, w):
        x = x.contiguous()
        ops = knn_ops(x)
        ctx.save_for_backward(idx, w)
        ctx.ops, ctx.n = ops, x.shape[0]
        return ops.interp_fwd(x, idx, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        idx, w = ctx.saved_tensors
        return ctx.ops.interp_bwd(dy.contiguous(), idx, w, ctx.n), None, None


def knn_interp(v_feats: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """v_feats [n, c], idx int32 [k, m], w [k, m] -> [m, c]; differentiable with respect to v_feats."""
    if torch.is_grad_enabled() and v_feats.requires_grad:
        return KnnInterpFunction.apply(v_feats, idx, w)
    return knn_ops(v_feats).interp_fwd(v_feats.contiguous(), idx, w)


class knn_up(nn.Module):
    """forward(v_coor [M, 3], v_feats [M, D], p_coor [N, 3]) -> [N, D]: every point's row is the weighted mean of the rows of its
    k nearest voxels, weight (1 / (d2 + 1e-8)) / the sum of those reciprocals, d2 the squared distance.  1 <= k <= 16.  One host
    read per call on the device route (the voxels' bounding box).  Served on the device: M < 2^24 voxels, and k * N < 2^24 in a
    backward; both are refused with a message above that."""

    def __init__(self, k):
        super().__init__()
        self.k = int(k)

    def forward(self, v_coor, v_feats, p_coor):
        if v_feats.dim() != 2 or v_feats.shape[0] != v_coor.shape[0]:
            raise ValueError(f"v_feats {list(v_feats.shape)}: one row per voxel of v_coor {list(v_coor.shape)}")
        if v_feats.device != v_coor.device:
            raise TypeError(f"v_feats on {v_feats.device}, v_coor on {v_coor.device}: one device")
        ops = knn_ops(v_feats)
        idx, d2 = knn_search(v_coor, p_coor, self.k)
        w = ops.weights(d2, idx)
        return knn_interp(v_feats, idx, w.to(v_feats.dtype))


def kNN(x_train, x_test, K):
    """-> (values [n_test, K], indices int64 [n_test, K]): the squared distances and indices of the K nearest rows of `x_train` for
    every row of `x_test`, nearest first; -1 / +inf where `x_train` has fewer than K rows."""
    idx, d2 = knn_search(x_train, x_test, K)
    return d2.t().contiguous(), idx.t().long().contiguous()


def index_points(points, idx):
    """points [N, C], idx integer [...] -> points[idx]."""
    return points[idx.long(), :]
