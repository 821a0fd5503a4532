"""The cases and checks of the semantic completion losses shared by the CPU leg (tests/test_semloss_cpu.py: grad/host.py in
fp32) and the GPU leg (tests/test_hip_semloss.py: csrc/semloss.hip).  Every comparison is either exact (labels, counts, the
order) or smooth (the ratio rule of tests/sem_ref64.py); no gradient is compared across two different orders."""
import numpy as np
import torch

from tests import sem_ref64 as sref

from pasco_amd.grad import semlib

T = semlib.geometry(1, 2)["tile"]
SHAPES = [(1, 2), (2, 19), (63, 20), (64, 32), (65, 2), (T - 1, 20), (T, 19), (T + 1, 32), (3 * T + 1, 20)]
PATTERNS = ["random", "saturated", "single_class", "all_present", "ignore10", "all_ignore", "outside", "ties"]
assert semlib.geometry(3 * T + 1, 20)["ranges"] > 1 and semlib.geometry(T, 19)["ranges"] > 1

# Past the first trip: above 65 536 rows a range of k_rows_part is longer than a workgroup, so a thread carries its num and den
# over two and three rows, and the sort and the Lovasz scan see 33 and 65 tiles.  Appended, so that the shapes above keep their
# seeds and scales.  Four patterns only; C = 2 with `ties` is left out on purpose: at this size the fp32 yardstick of loss_c
# is exactly 0 there, so the ratio is infinite for any fp32 route.
LONG_SHAPES = [(65537, 3), (131077, 3)]
LONG_PATTERNS = ["random", "ignore10", "ties", "outside"]
SHAPES += LONG_SHAPES
# every (shape, pattern) the two legs run, in the order and under the ids the full product had
CASES = [(s, p) for p in PATTERNS for s in SHAPES if s not in LONG_SHAPES or p in LONG_PATTERNS]
CASE_IDS = ["N%d_C%d-%s" % (s + (p,)) for s, p in CASES]
ROWS_BLOCK = 256                 # csrc/semloss.hip: the threads of a workgroup of k_rows_part


# !! `launch_class` restates, through the binding's `geometry`, how ps_rows_fwd, ps_sort_desc and ps_lovasz_fwd split N rows.  It
# !! is used to CHOOSE shapes and to assert, at import, that SHAPES reaches the classes below - never to form an expected value.
def launch_class(n, c):
    g = semlib.geometry(n, c)
    return dict(rows_per_thread=g["range_rows"] // ROWS_BLOCK, tiles=g["tiles"], ranges=g["ranges"])


def _check_shapes():
    short = [launch_class(*s) for s in SHAPES if s not in LONG_SHAPES]
    assert all(x["rows_per_thread"] == 1 and x["tiles"] <= 4 for x in short), "the short shapes: one row per thread, four tiles"
    a, b = (launch_class(*s) for s in LONG_SHAPES)
    assert (a["rows_per_thread"], a["tiles"]) == (2, 33), "two rows per thread of k_rows_part, 33 tiles"
    assert (b["rows_per_thread"], b["tiles"]) == (3, 65), "three rows per thread of k_rows_part, 65 tiles"
    assert all(s[0] % (launch_class(*s)["rows_per_thread"] * ROWS_BLOCK) != 0 for s in LONG_SHAPES), "a partial last range"
    assert all((s, p) in CASES for s in LONG_SHAPES for p in LONG_PATTERNS) and len(CASES) == 9 * 8 + 2 * 4


_check_shapes()


def scale_of(shape, pattern):
    return (1, 2, 4)[(SHAPES.index(shape) + PATTERNS.index(pattern)) % 3]


def make_case(shape, pattern, scale=None, dims=(16, 12, 6)):
    """-> dict of CPU tensors: logits fp32 [N, C] (float16-exact values x 2, or +-80), coords int32 [N, 4], target uint8 dims,
    min_C / max_C int64 [3] (min_C negative and no multiple of the scale), scale, weights fp32 [C]."""
    n, c = shape
    scale = scale_of(shape, pattern) if scale is None else scale
    g = torch.Generator().manual_seed(1000 * n + 10 * c + PATTERNS.index(pattern))
    dims_t = torch.tensor(dims)
    nvox = int(dims_t.prod())
    min_C = torch.tensor([-7, -5, -3])
    max_C = min_C + dims_t * scale - 1
    target = (torch.arange(nvox) % c).to(torch.uint8)
    if pattern == "single_class":
        target = torch.full((nvox,), c - 1, dtype=torch.uint8)
    elif pattern not in ("all_present",):
        target = torch.randint(0, c, (nvox,), generator=g).to(torch.uint8)
    if pattern in ("ignore10", "outside"):
        target[torch.rand(nvox, generator=g) < 0.1] = 255
    if pattern == "all_ignore":
        target[:] = 255
    vox = torch.randint(0, nvox, (n,), generator=g)
    if pattern == "all_present":
        vox = torch.arange(n) % nvox
    cell = torch.stack([vox // (dims[1] * dims[2]), (vox // dims[2]) % dims[1], vox % dims[2]], dim=1)
    xyz = min_C + cell * scale + torch.randint(0, scale, (n, 3), generator=g)
    if pattern == "outside":
        # one row beyond each of the six faces, spread over the rows, and a run of 70 consecutive rows outside
        for f in range(min(6, n)):
            r = (f * 11) % n
            axis, hi = f % 3, f >= 3
            xyz[r, axis] = (max_C[axis] + 1) if hi else (min_C[axis] - 1)
        if n > 200:
            xyz[100:170, 0] = max_C[0] + 1 + torch.arange(70)
    coords = torch.cat([torch.zeros(n, 1, dtype=torch.long), xyz], dim=1).to(torch.int32)
    logits = (torch.randn(n, c, generator=g).half().float() * 2)
    if pattern == "saturated":
        logits = torch.full((n, c), -80.0)
        logits[torch.arange(n), torch.randint(0, c, (n,), generator=g)] = 80.0
    if pattern == "ties":
        # two equal saturated maxima: p = 0.5 exactly for both, so a foreground and a background row of either class have
        # bit-equal errors; the rows come in duplicated pairs that land in voxels of different labels
        a = torch.randint(0, c, (n,), generator=g)
        b = (a + 1 + torch.randint(0, c - 1, (n,), generator=g)) % c
        a[1::2], b[1::2] = a[0:n - n % 2:2], b[0:n - n % 2:2]
        logits = torch.full((n, c), -80.0)
        logits[torch.arange(n), a] = 80.0
        logits[torch.arange(n), b] = 80.0
    weights = (torch.rand(c, generator=g) + 0.5).float()
    return {"logits": logits, "coords": coords, "target": target.reshape(dims), "min_C": min_C, "max_C": max_C, "scale": scale,
            "weights": weights, "n": n, "c": c}


def device_of(kind):
    return torch.device("cuda", 0) if kind == "hip" else torch.device("cpu")


def run_stages(kind, case):
    """The three forward stages of the leg `kind` -> the dict of pasco_amd.grad.semloss._stages, as CPU tensors (copies)."""
    from pasco_amd.grad.semloss import _stages
    d = device_of(kind)
    box = torch.cat([case["min_C"], case["max_C"]]).to(device=d, dtype=torch.int32)
    out = _stages(case["logits"].to(d), case["coords"].to(d), case["target"].to(d), box, case["scale"], case["weights"].to(d))
    return {k: v.detach().cpu().clone() for k, v in out.items()}


def stable_desc(keys):
    """keys int32 [S, M] holding uint32 patterns -> numpy's stable descending argsort, int32 [S, M]."""
    k = keys.numpy().view(np.uint32).astype(np.int64)
    return torch.from_numpy(np.argsort(-k, axis=1, kind="stable").astype(np.int32))


def ce_sums(x, y, w, dtype):
    """-> (num, den) of the weighted cross entropy over the rows with y != 255, in `dtype`."""
    on = y != sref.IGNORE
    ls = torch.log_softmax(x.to(dtype), dim=1)[on]
    wy = w.to(dtype)[y[on]]
    return (-(ls[torch.arange(len(wy)), y[on]]) * wy).sum(), wy.sum()


def kept_perms(perm, keep):
    """perm int [C, N] over all rows -> int64 [C, kept]: the same order over the kept rows, indexing the kept rows."""
    new = torch.cumsum(keep.long(), 0) - 1
    return torch.stack([new[p.long()][keep[p.long()]] for p in perm]) if perm.shape[0] else perm.long()


def coef_ref(y, perms, c, dtype, closed):
    """coef [kept, C] and loss increments by the cumsum formulation in `dtype` (or the closed form in fp64) along `perms`."""
    m = len(y)
    coef = torch.zeros((m, c), dtype=torch.float64)
    for k in range(c):
        fg = y == k
        if not bool(fg.any()):
            continue
        p = perms[k]
        if closed:
            _, inc = sref.closed_form(torch.zeros(m), fg[p], int(fg.sum()))
        else:
            inc = sref.lovasz_grad(fg[p].to(dtype)).double()
        coef[p, k] = torch.where(fg[p], -inc, inc)
    return coef


def check_forward(kind, M, shape, pattern):
    """Stages 1 to 4 of one case; returns (case, stages) for the gradient check."""
    case = make_case(shape, pattern)
    n, c = shape
    tag = f"{kind} N{n} C{c} {pattern} s{case['scale']}"
    out = run_stages(kind, case)
    args = (case["logits"], case["coords"], case["target"], case["min_C"], case["max_C"], case["scale"], case["weights"])
    r64 = sref.losses(*args, torch.float64)
    r32 = sref.losses(*args, torch.float32)
    keep, y = r64["keep"], r64["y"]
    # 1. rows: exact
    label = torch.full((n,), sref.OUTSIDE, dtype=torch.int64)
    label[keep] = y
    assert torch.equal(out["label"].long(), label), f"{tag}: label"
    assert torch.equal(out["class_count"].long(), torch.bincount(y[y < c], minlength=c)), f"{tag}: class_count"
    assert out["info"].tolist() == [int(keep.sum()), 0, 0, 0], f"{tag}: info {out['info'].tolist()}"
    err = out["keys"].view(torch.float32)
    assert bool((out["keys"][:, ~keep] == 0).all()), f"{tag}: a row outside the box has a key"
    if keep.any():
        sref.ratio_check(f"{tag} err", err[:, keep], r64["err"], r32["err"], M)
    x = case["logits"][keep]
    num64, den64 = ce_sums(x, y, case["weights"], torch.float64)
    num32, den32 = ce_sums(x, y, case["weights"], torch.float32)
    sref.ratio_check(f"{tag} ce_num", out["ce"][1], num64, num32, M)
    sref.ratio_check(f"{tag} ce_den", out["ce"][2], den64, den32, M)
    # 2. the order: exact
    assert torch.equal(out["perm"], stable_desc(out["keys"])), f"{tag}: perm is not the stable descending order of the keys"
    # 3. increments along that order: the closed form and the cumsum formulation in fp64, the cumsum formulation in fp32
    perms = kept_perms(out["perm"], keep)
    assert bool((out["coef"][~keep] == 0).all()), f"{tag}: coef of a row outside the box"
    absent = torch.bincount(y[y < c], minlength=c) == 0
    assert bool((out["coef"][:, absent] == 0).all()) and bool((out["loss_c"][absent] == 0).all()), f"{tag}: an absent class"
    if keep.any():
        c32 = coef_ref(y, perms, c, torch.float32, False)
        sref.ratio_check(f"{tag} coef/closed", out["coef"][keep], coef_ref(y, perms, c, None, True), c32, M)
        sref.ratio_check(f"{tag} coef/cumsum", out["coef"][keep], coef_ref(y, perms, c, torch.float64, False), c32, M)
        p64 = sref.lovasz_terms(x, y, torch.float64, perms)[0]
        p32 = sref.lovasz_terms(x, y, torch.float32, perms)[0]
        sref.ratio_check(f"{tag} loss_c/perm", out["loss_c"], p64, p32, M)
    # 4. the values against the fp64 formulation with its OWN order
    sref.ratio_check(f"{tag} loss_c", out["loss_c"], r64["loss_c"], r32["loss_c"], M)
    sref.ratio_check(f"{tag} ce", out["ce"][0], r64["ce"], r32["ce"], M)
    sref.ratio_check(f"{tag} lovasz", out["lovasz"][0], r64["lovasz"], r32["lovasz"], M)
    assert int(out["present"]) == r64["present"]
    return case, out, perms, keep, not bool((y != sref.IGNORE).any())


def public_call(kind, case):
    """SemComplLossFunction on the leg's device -> (F leaf, ce, lovasz)."""
    from pasco_amd.grad.semloss import sem_compl_loss
    d = device_of(kind)
    F = case["logits"].to(d).requires_grad_(True)
    ce, lov = sem_compl_loss(F, case["coords"].to(d), case["target"].to(d), case["min_C"], case["max_C"], case["scale"],
                             case["weights"].to(d))
    return F, ce, lov


def grad_of(F, loss):
    F.grad = None
    loss.backward(retain_graph=True)
    return F.grad.detach().cpu().clone()


def check_case(kind, M, shape, pattern):
    """Stages 1 to 5 of one case."""
    case, out, perms, keep, no_ce = check_forward(kind, M, shape, pattern)
    n, c = shape
    tag = f"{kind} N{n} C{c} {pattern} s{case['scale']}"
    F, ce, lov = public_call(kind, case)
    assert torch.equal(ce.detach().cpu(), out["ce"][0]) or (torch.isnan(ce) and torch.isnan(out["ce"][0])), f"{tag}: ce bits"
    assert torch.equal(lov.detach().cpu(), out["lovasz"][0]), f"{tag}: lovasz bits of a second call"
    args = (case["logits"], case["coords"], case["target"], case["min_C"], case["max_C"], case["scale"], case["weights"])
    # 5. the Lovasz gradient along the leg's own order (asserted stable above); the CE gradient needs no order
    d_lov = grad_of(F, lov)
    g64 = sref.losses(*args, torch.float64, perms=perms, g_ce=0.0)
    g32 = sref.losses(*args, torch.float32, perms=perms, g_ce=0.0)
    sref.ratio_check(f"{tag} dlogits/lovasz", d_lov, g64["dlogits"], g32["dlogits"], M)
    if not no_ce:
        d_ce = grad_of(F, ce)
        h64 = sref.losses(*args, torch.float64, g_lov=0.0)
        h32 = sref.losses(*args, torch.float32, g_lov=0.0)
        sref.ratio_check(f"{tag} dlogits/ce", d_ce, h64["dlogits"], h32["dlogits"], M)
        assert bool((d_ce[~keep] == 0).all()), f"{tag}: the CE gradient of a row outside the box"
    else:       # no row with a label: ce is torch's 0/0, and no class is present
        assert torch.isnan(ce) and float(lov.detach()) == 0.0, f"{tag}: all rows ignored gives (NaN, 0)"
        assert not bool(d_lov.any()), f"{tag}: all rows ignored has a zero Lovasz gradient"
    assert bool((d_lov[~keep] == 0).all()), f"{tag}: the Lovasz gradient of a row outside the box"
    if not no_ce:
        d0 = grad_of(F, ce * 0.0 + lov * 0.0)
        assert not bool(d0.any()) and not bool(torch.signbit(d0).any()), f"{tag}: zero incoming gradients give +0 everywhere"
    try:
        torch.autograd.grad(torch.autograd.grad(lov, F, create_graph=True)[0].sum(), F)
    except RuntimeError:
        pass
    else:
        raise AssertionError(f"{tag}: a double backward was not refused")
