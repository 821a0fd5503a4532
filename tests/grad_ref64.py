"""Test helper: fp64 references of the training operators of the convolution family (include/pasco_grad.h), written from the
formulas, and the bounds tests/test_grad_cpu.py and tests/test_hip_grad.py hold the code to.

Weight gradient, element-wise:   |dw - ref| <= C_WGRAD * A,   A = sum_o |x[nbr[k][o]]|^T |dy[o]|
(the magnitude the products and their fp32 sum passed through, whatever the cancellation).  The a-priori cap of any fp32 sum of
n addends is (n + 1) * 2^-24 of A; a measured ratio above it is a bug, not a calibration.
Input gradient: the forward kernels over the inverse table, so `gather_sum64` and the `C_ROUTE * A + EPI_ROUNDING * E` bound of
tests/conv_ref64.py.  Bias gradient: (n + 1) * 2^-24 * sum |dy|."""
import torch
import torch.nn.functional as F

from tests.conv_ref64 import C_ROUTE, EPI_ROUNDING, gather_sum64  # noqa: F401

# calibrated on the MI355X (tests/test_hip_grad.py prints the worst err / A per case): the largest measured ratio over the case
# table is 1.187e-6 ((27, 32, 32) at R + 1 = 257 rows: the row of large values sits in the middle of a chain of MFMA
# accumulations, and every later addend is rounded at its magnitude); the others 5.7e-8 .. 1.16e-6.  The summation orders are
# fixed, so the results are deterministic and the budget of 4x that, rounded up to a power of two, cannot flake.  The a-priori cap
# at the 2 R + 3 = 515 rows of the three-slab case is 516 * 2^-24 = 3.08e-5.
# The launch-class cases added later (two to four channel tiles, the wide 2 x 2 tiles, scalar loads, two chunks, misaligned bases,
# out-of-range table entries) measure 3.8e-7 .. 1.60e-6 (65 x 96, one partial wide tile); the case whose slab length the workspace
# cap doubles (256 x 256 at 2305 rows: 5 slabs of 512) measures 2.210e-6 - twice as many rows follow the row of large values
# inside a slab.  All stay under C_WGRAD, so none needed the fallback bound against the fp32 per-offset product; every case also
# has to stay under its own a-priori cap sum_cap(rows), which at 1 and 33 rows is the tighter of the two.
C_WGRAD_MEASURED = 1.187e-6
C_WGRAD_MEASURED_LAUNCH_CLASSES = 2.210e-6
C_WGRAD = 2.0 ** -17

# the stack test: max |g - g64| <= STACK_M * max |g32 - g64| per parameter tensor, g32 / g64 = the torch twin in fp32 / fp64.
# Measured worst ratio over the eleven tensors: 2.856 on the CPU (host restatement, up.kernel), 3.51 on the MI355X (head.bias);
# asserted at 4x the larger
STACK_M_MEASURED = {"cpu": 2.856, "mi355x": 3.51}
STACK_M = 4 * 3.51


def sum_cap(n: int) -> float:
    """Relative bound of any fp32 summation of n addends (first order in 2^-24, with the product roundings)."""
    return (n + 1) * 2.0 ** -24


def wgrad64(x, dy, nbr):
    """x [n_in, cin], dy [n_out, cout], nbr int [K, n_out] (-1 = none) -> (ref, A) fp64 [K, cin, cout]."""
    n_in, cin = x.shape
    xd = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64, device=x.device)])
    yd = dy.double()
    nb = nbr.long()
    nb = torch.where((nb >= 0) & (nb < n_in), nb, torch.full_like(nb, n_in))       # index n_in = the zero row
    K = nbr.shape[0]
    ref = torch.zeros(K, cin, dy.shape[1], dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(ref)
    for k in range(K):
        g = xd[nb[k]]
        ref[k] = g.t() @ yd
        mag[k] = g.abs().t() @ yd.abs()
    return ref, mag


def invert_loop(nbr, n_in):
    """Brute force: inv[k][nbr[k][o]] = o."""
    K, n_out = nbr.shape
    inv = [[-1] * n_in for _ in range(K)]
    rows = nbr.tolist()
    for k in range(K):
        for o in range(n_out):
            if rows[k][o] >= 0:
                inv[k][rows[k][o]] = o
    return torch.tensor(inv, dtype=torch.int32).reshape(K, n_in)


def invert_torch(nbr, n_in):
    """The same table by one torch scatter (any device)."""
    K, n_out = nbr.shape
    inv = torch.full((K, n_in + 1), -1, dtype=torch.int32, device=nbr.device)
    if n_out:
        idx = torch.where(nbr >= 0, nbr, torch.full_like(nbr, n_in)).long()
        inv.scatter_(1, idx, torch.arange(n_out, dtype=torch.int32, device=nbr.device).expand(K, n_out).contiguous())
    return inv[:, :n_in].contiguous()


def conv_twin(x, w, nbr, bias=None):
    """sum_k x[nbr[k]] @ w[k] + bias with torch indexing, in x's dtype, differentiable by torch's autograd."""
    n_in = x.shape[0]
    if nbr is None:
        out = x @ w.reshape(x.shape[1], -1)
    else:
        xz = torch.cat([x, torch.zeros(1, x.shape[1], dtype=x.dtype, device=x.device)])
        nb = nbr.long()
        nb = torch.where(nb >= 0, nb, torch.full_like(nb, n_in))
        w3 = w.reshape(nbr.shape[0], x.shape[1], -1)
        out = None
        for k in range(nbr.shape[0]):
            t = xz[nb[k]] @ w3[k]
            out = t if out is None else out + t
    return out if bias is None else out + bias.reshape(1, -1)


def stack_twin(params, maps, x, tgt, dtype):
    """The stack of tests/grad_cases.py `Stack` in plain torch on the recorded maps, in `dtype` -> {name: gradient}, plus "x".
    `params`: name -> tensor; `maps`: nbr1, nbr2, nbr3, nbr4, keep, b2o, n_union."""
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in params.items()}
    xi = x.detach().to(dtype).requires_grad_(True)
    y1 = conv_twin(xi, p["c1.kernel"], maps["nbr1"], p["c1.bias"])
    h = F.batch_norm(y1, None, None, p["bn.bn.weight"], p["bn.bn.bias"], True, 0.1, 1e-5)
    h = torch.relu(h)
    h = conv_twin(h, p["c2.kernel"], maps["nbr2"])
    h = conv_twin(h, p["c3.kernel"], maps["nbr3"], p["c3.bias"])
    h = conv_twin(h, p["up.kernel"], maps["nbr4"])
    h = h[maps["keep"].long()]
    u = torch.zeros(maps["n_union"], h.shape[1], dtype=dtype, device=x.device)
    u = torch.cat([h, u[h.shape[0]:]])
    u = u.index_add(0, maps["b2o"].long(), y1)
    out = conv_twin(u, p["head.kernel"], None, p["head.bias"])
    loss = (out - tgt.to(dtype)).square().mean()
    loss.backward()
    g = {k: v.grad for k, v in p.items()}
    g["x"] = xi.grad
    return g
