"""The semantic completion losses on the CPU: the host restatement (pasco_amd/grad/host.py, fp32) through the public layer
(pasco_amd/grad/semloss.py) against tests/sem_ref64.py, stage by stage; the geometry mirror; the edges; the drop-in functions;
the recorded reference scenes.  The GPU side is tests/test_hip_semloss.py."""
import numpy as np
import pytest
import torch

from tests import sem_cases as sc
from tests import sem_ref64 as sref


@pytest.mark.parametrize("shape,pattern", sc.CASES, ids=sc.CASE_IDS)
def test_host_stages_values_and_gradients_against_fp64(shape, pattern):
    sc.check_case("host", sref.PS_HOST_M, shape, pattern)


def test_geometry_mirror_matches_the_library():
    from pasco_amd.build import build_hip
    from pasco_amd.grad import semlib
    L = semlib.SemLib(build_hip(verbose=False))
    T = semlib.SORT_TILE
    for n in (0, 1, 255, 256, 257, T - 1, T, T + 1, 3 * T + 1, 65536, 65537, 300000, 1 << 24, (1 << 24) + 1, -1):
        for c in (1, 2, 19, 20, 32, 33):
            assert L.geometry(n, c) == semlib.geometry(n, c), (n, c)
            assert L.workspace_bytes(n, c) == semlib.geometry(n, c)["workspace_bytes"]
    for s, m in ((1, 0), (1, 1), (3, T + 1), (32, 3 * T + 1), (65535, 5), (65536, 5), (0, 5), (2, (1 << 24) + 1)):
        assert L.sort_workspace_bytes(s, m) == semlib.sort_workspace_bytes(s, m), (s, m)
    g = semlib.geometry(300000, 20)
    assert g["ranges"] <= 256 and g["range_rows"] % 256 == 0 and g["tiles"] == -(-300000 // T)


SORT_KEYS = ["random", "equal", "ascending", "descending", "two_values", "top_byte", "bottom_byte"]


def sort_keys(kind, s, m, seed=0):
    """uint32 [S, M] as int32 bit patterns."""
    rng = np.random.default_rng(seed + 17 * s + m)
    if kind == "random":
        k = rng.integers(0, 1 << 32, (s, m), dtype=np.uint64)
    elif kind == "equal":
        k = np.full((s, m), 0x3F000000, dtype=np.uint64)
    elif kind == "ascending":
        k = np.tile(np.arange(m, dtype=np.uint64) * 70001 % (1 << 32), (s, 1))
        k.sort(axis=1)
    elif kind == "descending":
        k = np.tile(np.arange(m, dtype=np.uint64) * 70001 % (1 << 32), (s, 1))
        k = -np.sort(-k.astype(np.int64), axis=1)
    elif kind == "two_values":
        k = np.where(rng.random((s, m)) < 0.5, 0x3F800000, 0x00000001).astype(np.uint64)
    elif kind == "top_byte":
        k = (rng.integers(0, 256, (s, m), dtype=np.uint64) << 24) | 0x00123456
    else:
        k = rng.integers(0, 256, (s, m), dtype=np.uint64) | 0x3F123400
    return torch.from_numpy(k.astype(np.uint32).view(np.int32).reshape(s, m))


@pytest.mark.parametrize("kind", SORT_KEYS)
@pytest.mark.parametrize("s", [1, 3, 32])
def test_host_sort_is_numpys_stable_descending_order(kind, s):
    from pasco_amd.grad import host
    for m in (1, 65, sc.T + 1) + ((sc.LONG_SHAPES[0][0],) if s == 3 else ()):
        keys = sort_keys(kind, s, m)
        wide = torch.from_numpy(keys.numpy().view(np.uint32).astype(np.int64))
        assert torch.equal(host.sem_sort_desc(wide), sc.stable_desc(keys)), (kind, s, m)


def _empty_case(c=20, n=0):
    case = sc.make_case((max(n, 1), c), "random", scale=2)
    for k in ("logits", "coords"):
        case[k] = case[k][:n]
    return case


def check_edges(kind):
    """N = 0; no row inside the box; the exceptions; the class-count refusal.  Shared with the GPU leg."""
    from pasco_amd.grad.semloss import sem_compl_loss
    d = sc.device_of(kind)
    case = _empty_case()
    F, ce, lov = sc.public_call(kind, case)
    assert torch.isnan(ce) and float(lov.detach()) == 0.0
    (ce * 0 + lov).backward()
    assert tuple(F.grad.shape) == (0, 20)
    # no row inside the box: every row is moved beyond the upper x face
    case = sc.make_case((65, 20), "random", scale=2)
    case["coords"][:, 1] = int(case["max_C"][0]) + 1
    out = sc.run_stages(kind, case)
    assert out["info"].tolist() == [0, 0, 0, 0] and bool((out["label"] == 254).all()) and not bool(out["keys"].any())
    assert not bool(out["coef"].any()) and float(out["lovasz"]) == 0.0 and int(out["present"]) == 0 and torch.isnan(out["ce"][0])
    F, ce, lov = sc.public_call(kind, case)
    lov.backward()
    assert not bool(F.grad.any())
    # a label in C..254 / an index outside the grid are counted, and stored as ignore
    case = sc.make_case((65, 19), "random", scale=4)
    case["target"].view(-1)[:] = 19
    out = sc.run_stages(kind, case)
    assert out["info"].tolist() == [65, 0, 65, 0] and bool((out["label"] == 255).all())
    case = sc.make_case((65, 19), "random", scale=1)
    case["max_C"] = case["max_C"] + 1
    case["coords"][7, 1:] = case["max_C"].to(torch.int32)
    out = sc.run_stages(kind, case)
    assert out["info"].tolist() == [65, 1, 0, 0] and int(out["label"][7]) == 255
    with pytest.raises(ValueError, match="classes not served"):
        sem_compl_loss(torch.zeros(4, 33, device=d), case["coords"][:4].to(d), case["target"].to(d), case["min_C"], case["max_C"], 1,
                       torch.ones(33, device=d))
    with pytest.raises(ValueError, match="classes not served"):
        sem_compl_loss(torch.zeros(4, 1, device=d), case["coords"][:4].to(d), case["target"].to(d), case["min_C"], case["max_C"], 1,
                       torch.ones(1, device=d))


def test_host_edges():
    check_edges("host")


class _Rows:
    def __init__(self, F, C):
        self.F, self.C = F, C


def dropin_inputs(kind, c=20, seed=5):
    """3 scales x 2 subnets; subnet 1 at scale 4 has no row in its box.  -> (args of the drop-ins, the per-pair cases)."""
    d = sc.device_of(kind)
    g = torch.Generator().manual_seed(seed)
    freq = {f"1_{s}": (torch.rand(c, generator=g).double().numpy() * 1000 + 5) for s in (1, 2, 4)}
    labels, logits, cases = {}, {}, {}
    min_Cs, max_Cs = [], []
    for s in (1, 2, 4):
        labels[f"1_{s}"], logits[s] = [], []
        for i in range(2):
            case = sc.make_case((130 + 7 * s + i, c), "ignore10" if i == 0 else "outside", scale=s, dims=(32 // s, 24 // s, 8 // s))
            if s == 4 and i == 1:
                case["coords"][:, 3] = int(case["min_C"][2]) - 1
            cases[(s, i)] = case
            labels[f"1_{s}"].append(case["target"].to(d))
            logits[s].append(_Rows(case["logits"].to(d).requires_grad_(True), case["coords"].to(d)))
            if s == 1:
                min_Cs.append(case["min_C"].to(d))
                max_Cs.append(case["max_C"].to(d))
    return (labels, logits, min_Cs, max_Cs, freq), cases, freq


def dropin_reference(cases, freq, exponent, skip_empty, dtype):
    ces, lovs = [], []
    for (s, i), case in cases.items():
        f = freq[f"1_{s}"] / np.sum(freq[f"1_{s}"])
        w = torch.from_numpy(np.power(np.amax(f) / f, exponent))
        r = sref.losses(case["logits"], case["coords"], case["target"], case["min_C"], case["max_C"], s, w.to(dtype), dtype)
        if skip_empty and not bool(r["keep"].any()):
            continue
        ces.append(r["ce"])
        lovs.append(r["lovasz"])
    return torch.stack(ces).mean(), torch.stack(lovs).mean()


def check_dropin(kind, M):
    from pasco_amd.grad import compute_sem_compl_loss, compute_sem_compl_loss_kitti360
    args, cases, freq = dropin_inputs(kind)
    for s in (1, 2, 4):       # every subnet's box has the same extent in voxels at every scale
        for i in range(2):
            assert torch.equal(cases[(s, i)]["min_C"], cases[(1, i)]["min_C"]) and torch.equal(cases[(s, i)]["max_C"], cases[(1, i)]["max_C"])
    ce, lov = compute_sem_compl_loss(*args)
    r64 = dropin_reference(cases, freq, 1 / 3.0, True, torch.float64)
    r32 = dropin_reference(cases, freq, 1 / 3.0, True, torch.float32)
    sref.ratio_check(f"{kind} drop-in ce", ce, r64[0], r32[0], M)
    sref.ratio_check(f"{kind} drop-in lovasz", lov, r64[1], r32[1], M)
    (ce + lov).backward()
    grads = [[r.F.grad for r in args[1][s]] for s in (1, 2, 4)]
    assert all(bool(g.any()) for g in grads[0] + grads[1] + grads[2][:1])
    assert grads[2][1] is None or not bool(grads[2][1].any()), "the skipped pair receives no gradient"
    # the other exponent gives another value; the KITTI-360 function skips nothing, so its empty pair makes the mean NaN
    ce360, lov360 = compute_sem_compl_loss_kitti360(*args)
    assert torch.isnan(ce360)
    k64 = dropin_reference(cases, freq, 1 / 1.5, False, torch.float64)
    k32 = dropin_reference(cases, freq, 1 / 1.5, False, torch.float32)
    sref.ratio_check(f"{kind} drop-in kitti360 lovasz", lov360, k64[1], k32[1], M)
    full = {k: v for k, v in cases.items() if k != (4, 1)}
    a2 = ({k: v[:1] for k, v in args[0].items()}, {s: v[:1] for s, v in args[1].items()}, args[2][:1], args[3][:1], args[4])
    ce360, _ = compute_sem_compl_loss_kitti360(*a2)
    one = {k: v for k, v in full.items() if k[1] == 0}
    k64, k32 = (dropin_reference(one, freq, 1 / 1.5, False, t) for t in (torch.float64, torch.float32))
    sref.ratio_check(f"{kind} drop-in kitti360 ce", ce360, k64[0], k32[0], M)
    w64 = dropin_reference(one, freq, 1 / 3.0, False, torch.float64)
    assert abs(float(k64[0]) - float(w64[0])) > 1e-3, "the two weight exponents give different losses"
    # all pairs skipped
    a3 = ({"1_4": args[0]["1_4"][1:]}, {4: args[1][4][1:]}, args[2][1:], args[3][1:], args[4])
    assert compute_sem_compl_loss(*a3) == (0.0, 0.0)
    # the two exceptions
    bad = {k: [t.clone() for t in v] for k, v in args[0].items()}
    bad["1_2"][0][:] = 200
    with pytest.raises(ValueError, match="labels outside"):
        compute_sem_compl_loss(bad, *args[1:])
    far = [m + 3 for m in args[3]]
    with pytest.raises(IndexError, match="outside the label grid"):
        moved = {s: [_Rows(r.F, r.C.clone()) for r in v] for s, v in args[1].items()}
        moved[1][0].C[0, 1:] = far[0].to(torch.int32)
        compute_sem_compl_loss(args[0], moved, args[2], far, args[4])


def test_host_dropins_mean_over_the_surviving_pairs():
    check_dropin("host", sref.PS_HOST_M)


def check_head_gradient(kind, M):
    """GPU leg only (pasco_amd.me has no CPU path).  A k = 1 convolution of pasco_amd.me in front of the loss: its kernel.grad through the leg equals the one through the host
    restatement fed with the same logits, by the ratio rule (fp64: the formulation's gradient pushed through x^T)."""
    import pasco_amd.me as ME
    from pasco_amd.grad.semloss import sem_compl_loss
    d = sc.device_of(kind)
    case = sc.make_case((300, 20), "ignore10", scale=1)
    torch.manual_seed(3)
    coords = torch.unique(case["coords"], dim=0)
    n = coords.shape[0]
    feats = (torch.randn(n, 8).half().float()).to(d)
    conv = ME.MinkowskiConvolution(8, 20, kernel_size=1, dimension=3).to(d)
    x = ME.SparseTensor(feats, coordinates=coords.to(d))
    y = conv(x)
    ce, lov = sem_compl_loss(y.F, y.C, case["target"].to(d), case["min_C"], case["max_C"], 1, case["weights"].to(d))
    (ce + lov).backward()
    got = conv.kernel.grad.detach().cpu().reshape(8, 20)
    # the same logits through the host restatement (fp32) and through the fp64 formulation along the host's order
    Fh = y.F.detach().cpu().clone().requires_grad_(True)
    Ch = y.C.detach().cpu()
    ce_h, lov_h = sem_compl_loss(Fh, Ch, case["target"], case["min_C"], case["max_C"], 1, case["weights"])
    (ce_h + lov_h).backward()
    idx = torch.tensor([int((coords == r).all(dim=1).nonzero()[0]) for r in Ch]) if not torch.equal(Ch, coords) else torch.arange(n)
    xin = feats.detach().cpu()[idx]
    host_grad = xin.t() @ Fh.grad
    case2 = dict(case, logits=Fh.detach(), coords=Ch)
    out = sc.run_stages("host", case2)
    keep, _ = sref.labels_of(Ch, case["target"], case["min_C"], case["max_C"], 1)
    perms = sc.kept_perms(out["perm"], keep)
    args = (Fh.detach(), Ch, case["target"], case["min_C"], case["max_C"], 1, case["weights"])
    g64 = xin.double().t() @ sref.losses(*args, torch.float64, perms=perms)["dlogits"]
    g32 = xin.t() @ sref.losses(*args, torch.float32, perms=perms)["dlogits"]
    if kind == "hip":
        # the device may order near-ties differently from the host: then the two gradients are both valid and differ; the
        # comparison through the ratio rule is made only along a shared order
        dev_out = sc.run_stages("hip", case2)
        if not torch.equal(dev_out["perm"], out["perm"]):
            perms = sc.kept_perms(dev_out["perm"], keep)
            g64 = xin.double().t() @ sref.losses(*args, torch.float64, perms=perms)["dlogits"]
            g32 = xin.t() @ sref.losses(*args, torch.float32, perms=perms)["dlogits"]
            host_grad = None
    sref.ratio_check(f"{kind} head kernel.grad", got, g64, g32, M)
    if host_grad is not None:
        sref.ratio_check(f"{kind} head kernel.grad (host)", host_grad, g64, g32, sref.PS_HOST_M)


GOLDEN = ["a", "b", "c"]


def check_golden(kind, M, name):
    """A recorded scene of the reference (tests/golden/make_golden_sem.py): its fp32 losses and CE gradients are the yardstick,
    tests/sem_ref64.py in fp64 the reference - and each recorded loss must lie within 2^-16 relative of that fp64 value, so that
    a wrong restatement cannot hide behind a large yardstick.  The Lovasz gradient is compared along the leg's own order."""
    import os
    import pasco_amd.grad as G
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"sem_{name}.npz"))
    d = sc.device_of(kind)
    fn_name, subnets, c = str(z["fn"]), int(z["subnets"]), int(z["c"])
    kitti360 = fn_name.endswith("kitti360")
    exponent = 1 / 1.5 if kitti360 else 1 / 3.0
    scales = [int(s) for s in z["scales"]]
    min_Cs = [torch.from_numpy(z["min_Cs"][i]) for i in range(subnets)]
    max_Cs = [torch.from_numpy(z["max_Cs"][i]) for i in range(subnets)]
    cases, labels, logits, freq = {}, {}, {}, {}
    for s in scales:
        freq[f"1_{s}"] = z[f"freq_{s}"]
        f = freq[f"1_{s}"] / np.sum(freq[f"1_{s}"])
        w = torch.from_numpy(np.power(np.amax(f) / f, exponent))
        labels[f"1_{s}"], logits[s] = [], []
        for i in range(subnets):
            case = {"logits": torch.from_numpy(z[f"logits_{s}_{i}"]).float(), "coords": torch.from_numpy(z[f"coords_{s}_{i}"]),
                    "target": torch.from_numpy(z[f"target_{s}_{i}"]), "min_C": min_Cs[i], "max_C": max_Cs[i], "scale": s,
                    "weights": w.float(), "w64": w}
            cases[(s, i)] = case
            labels[f"1_{s}"].append(case["target"].to(d))
            logits[s].append(_Rows(case["logits"].to(d).requires_grad_(True), case["coords"].to(d)))
    ce, lov = getattr(G, fn_name)(labels, logits, [m.to(d) for m in min_Cs], [m.to(d) for m in max_Cs], freq)

    def ref_args(case, dtype):
        return (case["logits"], case["coords"], case["target"], case["min_C"], case["max_C"], case["scale"], case["w64"].to(dtype), dtype)
    r64 = {k: sref.losses(*ref_args(v, torch.float64)) for k, v in cases.items()}
    alive = [k for k in cases if kitti360 or bool(r64[k]["keep"].any())]
    assert len(alive) == len(cases) - (1 if name == "c" else 0)
    ce64 = torch.stack([r64[k]["ce"] for k in alive]).mean()
    lov64 = torch.stack([r64[k]["lovasz"] for k in alive]).mean()
    ce32, lov32 = torch.tensor(float(z["ce32"])), torch.tensor(float(z["lovasz32"]))
    for what, v32, v64 in (("ce", ce32, ce64), ("lovasz", lov32, lov64)):
        rel = abs(float(v32) - float(v64)) / abs(float(v64))
        print(f"PS_GOLDEN {name} {what}: recorded fp32 {float(v32):.9g}, fp64 formulation {float(v64):.12g}, relative {rel:.2e}")
        assert rel <= 2.0 ** -16, f"scene {name} {what}: the fp64 formulation is not the reference's ({rel:.2e})"
    sref.ratio_check(f"{kind} golden {name} ce", ce, ce64, ce32, M)
    sref.ratio_check(f"{kind} golden {name} lovasz", lov, lov64, lov32, M)
    rows = {(s, i): logits[s][i] for s in scales for i in range(subnets)}
    for r in rows.values():
        r.F.grad = None
    ce.backward(retain_graph=True)
    for k in alive:
        g64 = sref.losses(*ref_args(cases[k], torch.float64), g_lov=0.0)["dlogits"] / len(alive)
        rec = torch.from_numpy(z[f"dce32_{k[0]}_{k[1]}"])
        got = rows[k].F.grad.cpu()
        sref.ratio_check(f"{kind} golden {name} dce s{k[0]} subnet {k[1]}", got, g64, rec, M)
        assert bool((got[~r64[k]["keep"]] == 0).all()) and bool((rec[~r64[k]["keep"]] == 0).all())
    for r in rows.values():
        r.F.grad = None
    lov.backward()
    for k in alive:
        out = sc.run_stages(kind, cases[k])
        assert torch.equal(out["perm"], sc.stable_desc(out["keys"]))
        perms = sc.kept_perms(out["perm"], r64[k]["keep"])
        g64 = sref.losses(*ref_args(cases[k], torch.float64), perms=perms, g_ce=0.0)["dlogits"] / len(alive)
        g32 = sref.losses(*ref_args(cases[k], torch.float32), perms=perms, g_ce=0.0)["dlogits"] / len(alive)
        got = rows[k].F.grad.cpu()
        sref.ratio_check(f"{kind} golden {name} dlovasz s{k[0]} subnet {k[1]}", got, g64, g32, M)
        rec = torch.from_numpy(z[f"dlovasz32_{k[0]}_{k[1]}"])
        assert bool((got[~r64[k]["keep"]] == 0).all()) and bool((rec[~r64[k]["keep"]] == 0).all())
    for k in cases:
        if k not in alive:
            assert rows[k].F.grad is None or not bool(rows[k].F.grad.any())


@pytest.mark.parametrize("name", GOLDEN)
def test_host_recorded_reference_scenes(name):
    check_golden("host", sref.PS_HOST_M, name)
