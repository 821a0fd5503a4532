"""Test helper: the torch twin of training-mode batch normalisation over rows (include/pasco_norm.h, pasco_amd/grad/norm.py)
and the bound tests/norm_cases.py holds the operator to.

The twin is plain torch: `F.batch_norm` in training mode over the CONCATENATED rows of all ranks, then the activation, then
torch's autograd.  In fp64 it is the reference v64; in fp32 on the device under test it is v32, whose distance from v64 is the
error torch itself makes on these inputs.  For each checked quantity v (y, dx, weight.grad, bias.grad, running_mean,
running_var)

    max |v - v64| <= NORM_M * max |v32 - v64|.

NORM_M_MEASURED: the worst ratio over every quantity of every case asserted against NORM_M (tests/test_norm_cpu.py,
tests/test_norm_gloo.py and tests/test_hip_norm.py print the ratios per case): the case table of tests/norm_cases.py, the
large-mean case, the virtual ranks, the merged records of a permuted split, the two gloo ranks and - on the GPU - the gradients
of tests/grad_cases.py `Stack` under set_me_norm("device").
  CPU restatement: 11.870 (weight.grad at n = 128, c = 1, ReLU; next 5.954, weight.grad at n = 63, c = 1; everything with more
    than one channel is under 2.3).  With c = 1 the "max" of torch's own error is one number, which here happens to be small:
    the operator's error there, 2.1e-7 of the gradient, is of the size of its other cases.
  MI355X: 2.804 (weight.grad at n = 128, c = 3, leaky); `Stack` 2.418 (bn.bn.bias); y at most 2.051, dx 1.246; the large-mean case 0.404.
The long cases of tests/norm_cases.py (9 T + 1 to 65 T + 3 rows at c = 2 .. 260, merged records of unequal chunks, the virtual
ranks at c = 128, misaligned rows at c = 256) stay under both: CPU restatement 2.456 (weight.grad at n = 32 T + 1), MI355X 1.443;
the merged moments of 8 .. 97 unequal records are within 1e-8 of torch's fp32 error on either.
Asserted at 4 x the larger of the two, the convention of tests/rowgrad_ref.py.  The reduction orders are fixed, so the results
are deterministic and the budget cannot flake."""
import torch
import torch.nn.functional as F

NORM_M_MEASURED = {"cpu": 11.870, "mi355x": 2.804}
NORM_M = 4 * max(NORM_M_MEASURED.values())

QUANTITIES = ("y", "dx", "dw", "db", "running_mean", "running_var")


def act_twin(z, act: str, slope: float):
    if act == "relu":
        return torch.relu(z)
    if act == "leaky":
        return F.leaky_relu(z, slope)
    return z


def norm_twin(xs, dys, weight, bias, running_mean, running_var, factor, eps, act, slope, dtype):
    """xs / dys: the row chunks of the ranks (lists of [n_r, c]); weight / bias / running_* [c] or None; `factor` = the
    exponential average factor.  -> {y, dx, dw, db, running_mean, running_var} in `dtype` over the concatenated rows (None where
    there is no such tensor)."""
    x = torch.cat(list(xs)).detach().to(dtype).requires_grad_(True)
    dy = torch.cat(list(dys)).detach().to(dtype)
    w = weight.detach().to(dtype).requires_grad_(True) if weight is not None else None
    b = bias.detach().to(dtype).requires_grad_(True) if bias is not None else None
    rm = running_mean.detach().to(dtype).clone() if running_mean is not None else None
    rv = running_var.detach().to(dtype).clone() if running_var is not None else None
    y = act_twin(F.batch_norm(x, rm, rv, w, b, True, factor, eps), act, slope)
    y.backward(dy)
    return {"y": y.detach(), "dx": x.grad, "dw": w.grad if w is not None else None, "db": b.grad if b is not None else None,
            "running_mean": rm, "running_var": rv}


def ratios(got: dict, v32: dict, v64: dict) -> dict:
    """name -> max |v - v64| / max |v32 - v64| over the quantities `got` has."""
    out = {}
    for k in QUANTITIES:
        if got.get(k) is None:
            continue
        e = float((got[k].double() - v64[k]).abs().max()) if got[k].numel() else 0.0
        e32 = float((v32[k].double() - v64[k]).abs().max()) if got[k].numel() else 0.0
        out[k] = e / e32 if e32 > 0 else (0.0 if e == 0 else float("inf"))
    return out
