"""Test helper: fp64 restatement of one fused convolution (the gather-matmul and the epilogue of conv_h2_common.h: bias -> BN ->
act, then the tail: second BN, per-axis table rows, dense residual, res_act) and the element-wise, condition-aware bound the
route tests hold every kernel to (tests/test_hip_conv_routes.py, tests/test_conv_routes_cpu.py).

The bound for one output element is

    |got - ref| <= C_ROUTE * A + EPI_ROUNDING * E

A = |BN scale| * |bn2 scale| * sum_k |x| . |w|: the magnitude the products and their fp32 sum passed through, so the split operands
(hi + lo f16 pairs) and the accumulation order get a relative budget of C_ROUTE of it, whatever the cancellation in the sum.
E = the sum of the magnitudes of every addend the fp32 epilogue rounds (the sum itself, bias, shifts, table rows, residual): a few
fp32 roundings of those.  No mean over the tensor enters, so an error confined to one row, one column or one tail term is caught."""
import torch

# calibrated on the MI355X (tests/test_hip_conv_routes.py prints the worst err / A per route): the largest measured ratio over
# every route and edge shape is 1.19e-7 (k_conv_wide 256 x 256, k_conv_mfma), the others 3e-8 .. 1.1e-7; the summation orders are
# fixed, so the results are deterministic and the budget of 4x that cannot flake
C_ROUTE = 2.0 ** -21
EPI_ROUNDING = 8 * 2.0 ** -24


def act64(v, act, slope):
    if act == 1:
        return torch.clamp_min(v, 0.0)
    if act == 2:
        return torch.where(v > 0, v, v * slope)
    return v


def gather_sum64(x, w, nbr, rows):
    """x [n_in, cin] (the values the operand stands for), w [kvol, cin, cout], nbr int [kvol, n_out] (-1 = no neighbour) or None
    (identity map, kvol 1), rows long [S] -> (acc, mag), fp64 [S, cout]: sum_k x[nbr[k, r]] @ w[k] and sum_k |x[nbr[k, r]]| @ |w[k]|."""
    n_in, cin = x.shape
    dev = x.device
    xd = torch.cat([x.double(), torch.zeros(1, cin, dtype=torch.float64, device=dev)])
    xa = xd.abs()
    wd = w.double()
    wa = wd.abs()
    nb = nbr[:, rows].long() if nbr is not None else rows[None].long()
    nb = torch.where(nb >= 0, nb, torch.full_like(nb, n_in))          # index n_in = the zero row
    acc = torch.zeros(rows.shape[0], w.shape[2], dtype=torch.float64, device=dev)
    mag = torch.zeros_like(acc)
    for k in range(w.shape[0]):
        acc += xd[nb[k]] @ wd[k]
        mag += xa[nb[k]] @ wa[k]
    return acc, mag


def has_tail(spec):
    return any(spec.get(k) is not None for k in ("residual", "epi2_scale", "epi2_shift", "axis")) or spec.get("res_act", 0) != 0


def epilogue64(acc, mag, spec, rows):
    """The epilogue of `spec` (conv_fwd's keyword arguments: bias, epi_scale, epi_shift, epi_act, slope, epi2_scale, epi2_shift,
    axis = (table [3, T, cout], coords [n_out, 4], lo), residual [n_out, cout], res_act) on the sampled rows, in fp64.
    -> (ref, A, E) [S, cout]: the result and the two magnitudes of the bound (module docstring)."""
    slope = spec.get("slope", 0.01)
    one = torch.ones(acc.shape[1], dtype=torch.float64, device=acc.device)

    def vec(name):
        v = spec.get(name)
        return None if v is None else v.double()

    bias, s, b = vec("bias"), vec("epi_scale"), vec("epi_shift")
    ref, e = acc, acc.abs()
    if bias is not None:
        ref = ref + bias
        e = e + bias.abs()
    sa = one if s is None else s.abs()
    if s is not None:
        ref = ref * s
    e = e * sa
    if b is not None:
        ref = ref + b
        e = e + b.abs()
    a = mag * sa
    ref = act64(ref, spec.get("epi_act", 0), slope)
    if has_tail(spec):
        s2, b2 = vec("epi2_scale"), vec("epi2_shift")
        if s2 is not None:
            ref = ref * s2
            e = e * s2.abs()
            a = a * s2.abs()
        if b2 is not None:
            ref = ref + b2
            e = e + b2.abs()
        if spec.get("axis") is not None:
            tab, coords, lo = spec["axis"]
            ai = (coords[rows][:, 1:4].long() - lo).clamp(0, tab.shape[1] - 1)      # the kernel clamps (and raises status 4)
            for ax in range(3):
                t = tab[ax][ai[:, ax]].double()
                ref = ref + t
                e = e + t.abs()
        if spec.get("residual") is not None:
            r = spec["residual"][rows].double()
            ref = ref + r
            e = e + r.abs()
        ref = act64(ref, spec.get("res_act", 0), slope)
    return ref, a, e


def bound(a, e, c=C_ROUTE):
    return c * a + EPI_ROUNDING * e + 1e-30


def violations(got, ref, a, e, c=C_ROUTE):
    """Boolean mask of the elements outside the bound (NaN / Inf count as outside)."""
    err = (got.double() - ref).abs()
    return ~(err <= bound(a, e, c))


def worst_ratio(got, ref, a, e):
    """max over the elements with A > 0 of (|got - ref| - the epilogue's rounding allowance) / A: what C_ROUTE must cover."""
    err = (got.double() - ref).abs() - EPI_ROUNDING * e
    ok = a > 0
    if not bool(ok.any()):
        return 0.0
    return max(0.0, float((err[ok] / a[ok]).max()))
