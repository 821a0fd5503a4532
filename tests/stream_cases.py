"""Test helper: the table and the harness of the stream-contract tests (tests/test_hip_streams.py on the GPU,
tests/test_streams_cpu.py for the table's completeness).  DESIGN.md 4v is the method.

The eight training families promise "all work is enqueued on `stream`; no call synchronises, allocates or reads the host".
On torch's default stream (the null stream) a launch that lost its stream argument, a memset on stream 0, a scratch buffer
shared between streams and a hidden read-back all give correct results.  The harness here runs every launching entry point of
the eight bindings on a side stream behind a pending producer, on two streams at once, and in a captured graph.

An `Entry` is one call (or the call sequence of one step):

    make(seed, device) -> dict.  Shapes, host constants and index ranges are fixed; the values depend on the seed.
        plain key, tensor value      an operand: the harness copies it device-to-device from another seed's dict
        plain key, any other value   a host constant: equal for every seed (asserted)
        key "out..."                 a buffer the call overwrites: filled with a poison pattern, in stream order, before the call
        key "_..."                   private to the dict (tables that hold addresses of the dict's own buffers): never copied
    run(inputs) -> tuple of tensors: everything the call writes, buffers written in place included.

Every run gets a dict of its own from `make`, so an operand updated in place starts from the seed's values each time.  The
module imports without a GPU and without the library; the bindings are loaded inside `make` / `run`."""
import time
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch

from tests import grad_cases as gc
from tests import rowgrad_cases as rc

# seeds no other test of the process uses
SEED_A, SEED_B = 770001, 770002
PAIR_SEEDS = (770011, 770012, 770013, 770014)
FLOOR_MS = 5.0                # the least producer length
HOST_FACTOR = 20              # the producer is at least this many times the host time of the entry's warm call
POISON = 0xA5

# what each binding's _SIGNATURES names besides its launching entry points
NON_LAUNCHING = {
    "pg": ("abi_version", "last_error", "wgrad_slab_rows", "wgrad_workspace_bytes", "colsum_workspace_bytes"),
    "pr": ("abi_version", "last_error"),
    "pa": ("abi_version", "last_error", "attn_bwd_workspace_bytes"),
    "pm": ("abi_version", "last_error", "pair_sums_ranges", "pair_sums_workspace_bytes", "assign"),      # pm_assign: a host function
    "ps": ("abi_version", "last_error", "geometry", "workspace_bytes", "sort_workspace_bytes"),
    "pn": ("abi_version", "last_error", "ws_bytes"),
    "po": ("abi_version", "last_error", "table_check"),
    "pt": ("abi_version", "last_error", "resample_workspace_bytes"),
}


def signatures():
    """family -> the names of its binding's _SIGNATURES (no library is loaded)."""
    from pasco_amd.data import target_lib
    from pasco_amd.grad import attnlib, lib, matchlib, normlib, optimlib, rowlib, semlib
    return {"pg": set(lib._SIGNATURES), "pr": set(rowlib._SIGNATURES), "pa": set(attnlib._SIGNATURES),
            "pm": set(matchlib._SIGNATURES), "ps": set(semlib._SIGNATURES), "pn": set(normlib._SIGNATURES),
            "po": set(optimlib._SIGNATURES), "pt": set(target_lib._SIGNATURES)}


class Entry(NamedTuple):
    name: str
    family: str
    covers: Tuple[str, ...]                  # the names of the family's _SIGNATURES this entry launches
    make: Callable
    run: Callable
    two_streams: bool = False                # part 3 runs it on two streams at once
    caches_scratch: bool = False             # ... and expects release_stream to find per-stream scratch afterwards
    step_keys: Optional[Tuple[str, ...]] = None     # po: the operands a second step replaces (the gradients); None = all


def _gen(seed, salt=0):
    return torch.Generator().manual_seed(int(seed) * 31 + salt)


# ---- pg_* --------------------------------------------------------------------------------------------------------------------
_MAPS = {}


def _map(kind, rows, device):
    """The neighbour table of tests/grad_cases.py (seed 0) cut to `rows` output rows, made once per device: the tables of every
    seed are this one with its output rows permuted, so n_in and the shape are fixed."""
    key = (kind, rows, str(device))
    if key not in _MAPS:
        nbr, n_in = gc.table_with_rows(kind, rows, device)
        _MAPS[key] = (nbr.contiguous(), int(n_in))
    return _MAPS[key]


def _permuted(nbr, seed):
    perm = torch.randperm(nbr.shape[1], generator=_gen(seed, 1)).to(nbr.device)
    return nbr[:, perm].contiguous()


def _make_nbr_invert(seed, device):
    nbr, n_in = _map("same", None, device)
    return {"nbr": _permuted(nbr, seed), "n_in": n_in, "out_inv": torch.empty((nbr.shape[0], n_in), dtype=torch.int32, device=device)}


def _run_nbr_invert(d):
    from pasco_amd.grad.lib import grad_lib
    return (grad_lib().nbr_invert(d["nbr"], d["n_in"], out=d["out_inv"]),)


def _make_wgrad(cin, cout, rows):
    def make(seed, device):
        nbr, n_in = _map("same", rows, device)
        x, dy = gc.operands(n_in, cin, rows, cout, device, seed)
        return {"x": x, "dy": dy, "nbr": _permuted(nbr, seed),
                "out_dw": torch.empty((nbr.shape[0], cin, cout), dtype=torch.float32, device=device)}
    return make


def _run_wgrad(d):
    from pasco_amd.grad.lib import grad_lib
    return (grad_lib().conv_wgrad(d["x"], d["dy"], d["nbr"], out=d["out_dw"]),)


def _make_colsum(seed, device):
    dy = torch.randn(gc.COLSUM_ROWS + 1, 20, generator=_gen(seed))
    return {"dy": dy.to(device), "out_sum": torch.empty(20, dtype=torch.float32, device=device)}


def _run_colsum(d):
    from pasco_amd.grad.lib import grad_lib
    return (grad_lib().colsum(d["dy"], out=d["out_sum"]),)


R = gc.SLAB_ROWS
assert gc.wgrad_geometry(27, 32, 32, 2 * R + 3)["slabs"] == 3, "32 x 32 at 2 R + 3 rows: three slabs, the reduce runs"
assert gc.wgrad_geometry(27, 256, 256, R + 1)["slabs"] == 2 and gc.wgrad_geometry(27, 256, 256, R + 1)["wide"]

# ---- pr_* --------------------------------------------------------------------------------------------------------------------
GRID, ROWS_N, ROWS_C, MIN3, TS = (12, 12, 6), 131, 65, (-8, 0, 8), 2
POOL_C = 20


def _make_dense_rows(seed, device):
    dense = rc.values((rc.BATCH, ROWS_C) + GRID, seed, device)
    coords = rc.coords_of(rc.site_rows(GRID, ROWS_N, seed, True), MIN3, TS).to(device)
    return {"dense": dense, "coords": coords, "out_rows": torch.empty((ROWS_N, ROWS_C), dtype=torch.float32, device=device)}


def _run_dense_rows(d):
    from pasco_amd.grad.rowlib import rowgrad_lib
    return (rowgrad_lib().dense_rows(d["dense"], d["coords"], MIN3, TS, out=d["out_rows"]),)


def _make_rows_dense(seed, device):
    return {"rows": rc.values((ROWS_N, ROWS_C), seed, device), "sites": rc.site_rows(GRID, ROWS_N, seed, True).to(device),
            "out_dense": torch.empty((rc.BATCH, ROWS_C) + GRID, dtype=torch.float32, device=device)}


def _run_rows_dense(d):
    from pasco_amd.grad.rowlib import rowgrad_lib
    return (rowgrad_lib().rows_dense(d["rows"], d["sites"], (rc.BATCH, ROWS_C) + GRID, out=d["out_dense"]),)


def _pool_operands(seed, device):
    from pasco_amd.me.backend import hip_backend
    nbr, n_in = _map("down", None, device)
    nbr = _permuted(nbr, seed)
    x = torch.randint(-2, 3, (n_in, POOL_C), generator=_gen(seed)).float().to(device)      # repeated maxima inside a window
    return x, nbr, n_in, hip_backend().maxpool_fwd(x, nbr)


def _make_maxpool_arg(seed, device):
    x, nbr, n_in, pooled = _pool_operands(seed, device)
    return {"x": x, "nbr": nbr, "pooled": pooled}


def _run_maxpool_arg(d):
    from pasco_amd.grad.rowlib import rowgrad_lib
    return (rowgrad_lib().maxpool_arg(d["x"], d["nbr"], d["pooled"]),)


def _make_maxpool_bwd(seed, device):
    from pasco_amd.grad.lib import grad_lib
    from pasco_amd.grad.rowlib import rowgrad_lib
    x, nbr, n_in, pooled = _pool_operands(seed, device)
    arg = rowgrad_lib().maxpool_arg(x, nbr, pooled)
    inv = grad_lib().nbr_invert(nbr, n_in)
    dy = rc.values((nbr.shape[1], POOL_C), seed + 1, device)
    return {"dy": dy, "arg": arg, "inv": inv, "n_in": n_in, "out_dx": torch.empty((n_in, POOL_C), dtype=torch.float32, device=device)}


def _run_maxpool_bwd(d):
    from pasco_amd.grad.rowlib import rowgrad_lib
    return (rowgrad_lib().maxpool_bwd(d["dy"], d["arg"], d["inv"], d["n_in"], out=d["out_dx"]),)


# ---- pa_* --------------------------------------------------------------------------------------------------------------------
def _make_attn(shape):
    def make(seed, device):
        from pasco_amd.me.backend import hip_backend
        from tests.attn_grad_cases import Inputs
        x = Inputs(shape, "mask_any", seed=seed)
        bits, any_ = x.words()
        d = {k: t.to(device).contiguous() for k, t in (("q", x.q), ("k", x.k), ("v", x.v), ("bits", bits), ("any", any_), ("dout", x.dout))}
        d["fwd"] = hip_backend().attn_cross_fwd(d["q"], d["k"], d["v"], d["bits"], d["any"])
        return d
    return make


def _run_attn_stats(d):
    from pasco_amd.grad.attnlib import attn_grad_lib
    return attn_grad_lib().attn_bwd_stats(d["q"], d["k"], d["bits"], d["any"], d["fwd"], d["dout"])


def _run_attn_bwd(d):
    from pasco_amd.grad.attnlib import attn_grad_lib
    return attn_grad_lib().attn_cross_bwd(d["q"], d["k"], d["v"], d["bits"], d["any"], d["fwd"], d["dout"])


# ---- pm_* --------------------------------------------------------------------------------------------------------------------
PM_Q, PM_T, PM_N = 5, 65, 129


def _make_pm_pack(seed, device):
    from tests.match_cases import pack_case
    masks, unknown, coords, _ = pack_case(PM_T, seed=seed)
    return {"masks": masks.to(device), "unknown": unknown.to(device), "coords": coords[:PM_N].contiguous().to(device),
            "origin": (3, -2, 10)}


def _run_pm_pack(d):
    from pasco_amd.grad.matchlib import match_lib
    return match_lib().target_pack(d["masks"], d["unknown"], d["coords"], d["origin"])


def _pm_operands(seed, device):
    from tests.match_cases import pack_words
    g = _gen(seed)
    logits = torch.randn(PM_N, PM_Q, generator=g)
    tgt = torch.nn.functional.one_hot(torch.randint(0, PM_T, (PM_N,), generator=g), PM_T).bool()
    tgt &= (torch.rand(PM_N, generator=g) >= 0.3)[:, None]
    known = torch.rand(PM_N, generator=g) >= 0.2
    tbits, flags = pack_words(tgt, known)
    tq = torch.randperm(PM_T, generator=g)[:PM_Q].to(torch.int32)
    tq[int(torch.randint(0, PM_Q, (1,), generator=g))] = -1                                  # one unmatched query
    coef = torch.randn(PM_Q, 3, generator=g)
    return {"logits": logits.to(device), "tbits": tbits.to(device), "flags": flags.to(device), "tgt_of_query": tq.to(device),
            "coef": coef.to(device)}


def _make_pm_sums(seed, device):
    d = _pm_operands(seed, device)
    return {k: d[k] for k in ("logits", "tbits", "flags")}


def _run_pm_sums(d):
    from pasco_amd.grad.matchlib import BIT_MATCHABLE, match_lib
    return match_lib().pair_sums(d["logits"], d["tbits"], d["flags"], BIT_MATCHABLE, PM_T)


def _run_pm_bwd(d):
    from pasco_amd.grad.matchlib import match_lib
    return (match_lib().mask_loss_bwd(d["logits"], d["tbits"], d["flags"], d["tgt_of_query"], d["coef"], PM_T),)


# ---- ps_* --------------------------------------------------------------------------------------------------------------------
def _sem_shape():
    from tests import sem_cases as sc
    shape = min((s for s in sc.SHAPES if sc.launch_class(*s)["ranges"] >= 2 and sc.launch_class(*s)["tiles"] >= 2), key=lambda s: s[0])
    return shape


SEM_DIMS, SEM_SCALE = (16, 12, 6), 2


def _sem_operands(seed, device):
    """The "random" pattern of tests/sem_cases.make_case with 10 % of the voxels ignored, from this seed."""
    n, c = _sem_shape()
    g = _gen(seed)
    dims_t = torch.tensor(SEM_DIMS)
    nvox = int(dims_t.prod())
    min_C = torch.tensor([-7, -5, -3])
    max_C = min_C + dims_t * SEM_SCALE - 1
    target = torch.randint(0, c, (nvox,), generator=g).to(torch.uint8)
    target[torch.rand(nvox, generator=g) < 0.1] = 255
    vox = torch.randint(0, nvox, (n,), generator=g)
    cell = torch.stack([vox // (SEM_DIMS[1] * SEM_DIMS[2]), (vox // SEM_DIMS[2]) % SEM_DIMS[1], vox % SEM_DIMS[2]], dim=1)
    xyz = min_C + cell * SEM_SCALE + torch.randint(0, SEM_SCALE, (n, 3), generator=g)
    coords = torch.cat([torch.zeros(n, 1, dtype=torch.long), xyz], dim=1).to(torch.int32)
    logits = torch.randn(n, c, generator=g).half().float() * 2
    weights = (torch.rand(c, generator=g) + 0.5).float()
    return {"logits": logits.to(device), "coords": coords.to(device), "target": target.reshape(SEM_DIMS).to(device),
            "box": torch.cat([min_C, max_C]).to(device=device, dtype=torch.int32), "weights": weights.to(device)}


def _sem_stages(seed, device):
    """The operands and every intermediate of one forward (made on a workspace of its own)."""
    from pasco_amd.grad.semlib import geometry, sem_lib
    d = _sem_operands(seed, device)
    n, c = _sem_shape()
    ws = torch.empty(max(geometry(n, c)["workspace_bytes"], 256), dtype=torch.uint8, device=device)
    out = sem_lib().forward(d["logits"], d["coords"], d["target"], d["box"], SEM_SCALE, d["weights"], ws=ws)
    out = {k: v.clone() for k, v in out.items()}
    out.update(d)
    return out


def _make_sem_forward(seed, device):
    return _sem_operands(seed, device)


def _run_sem_forward(d):
    from pasco_amd.grad.semlib import sem_lib
    o = sem_lib().forward(d["logits"], d["coords"], d["target"], d["box"], SEM_SCALE, d["weights"])
    # keys and perm are views of the stream's workspace: copied in stream order
    return (o["label"], o["ce"], o["class_count"], o["info"], o["loss_c"], o["coef"], o["lovasz"], o["present"], o["keys"].clone(),
            o["perm"].clone())


def _make_sem_rows(seed, device):
    from pasco_amd.grad.semlib import geometry
    n, c = _sem_shape()
    d = _sem_operands(seed, device)
    d["out_keys"] = torch.empty((c, n), dtype=torch.int32, device=device)
    d["_ws"] = torch.empty(max(geometry(n, c)["rows_bytes"], 256), dtype=torch.uint8, device=device)
    return d


def _run_sem_rows(d):
    from pasco_amd.grad.semlib import sem_lib
    out = sem_lib().rows_fwd(d["logits"], d["coords"], d["target"], d["box"], SEM_SCALE, d["weights"], d["out_keys"], d["_ws"])
    return out + (d["out_keys"],)


def _make_sem_sort(seed, device):
    s = _sem_stages(seed, device)
    return {"keys": s["keys"], "out_perm": torch.empty_like(s["perm"])}


def _run_sem_sort(d):
    from pasco_amd.grad.semlib import sem_lib
    return (sem_lib().sort_desc(d["keys"], d["out_perm"]),)


def _make_sem_lovasz(seed, device):
    s = _sem_stages(seed, device)
    return {k: s[k] for k in ("perm", "label", "keys", "class_count")}


def _run_sem_lovasz(d):
    from pasco_amd.grad.semlib import sem_lib
    return sem_lib().lovasz_fwd(d["perm"], d["label"], d["keys"], d["class_count"])


def _make_sem_bwd(seed, device):
    s = _sem_stages(seed, device)
    d = {k: s[k] for k in ("logits", "label", "coef", "weights", "ce", "present")}
    d["g"] = (torch.rand(2, generator=_gen(seed, 2)) + 0.5).to(device)
    return d


def _run_sem_bwd(d):
    from pasco_amd.grad.semlib import sem_lib
    return (sem_lib().loss_bwd(d["logits"], d["label"], d["coef"], d["weights"], d["ce"], d["present"], d["g"]),)


# ---- pn_* --------------------------------------------------------------------------------------------------------------------
PN_C, PN_R, PN_SLOPE, PN_EPS, PN_MOMENTUM = 20, 9, 0.07, 1e-5, 0.1


def _pn_rows():
    from pasco_amd.grad.normlib import PN_TILE_ROWS
    return 9 * PN_TILE_ROWS + 1


def _record(x):
    """The moments record fp64 [3, c] of the rows x, in torch."""
    x = x.double()
    mean = x.mean(0)
    return torch.stack([torch.full_like(mean, x.shape[0]), mean, (x - mean).square().sum(0)])


def _pn_operands(seed, device):
    n, g = _pn_rows(), _gen(seed)
    x = torch.randn(n, PN_C, generator=g) * 1.3 + 0.37
    dy = torch.randn(n, PN_C, generator=g) * 0.71 + 0.05
    w = torch.randn(PN_C, generator=g) * 0.37 + 1.13
    b = torch.randn(PN_C, generator=g) * 0.29 + 0.11
    rm, rv = torch.randn(PN_C, generator=g) * 0.3, torch.rand(PN_C, generator=g) + 0.5
    rec = _record(x)
    mean_rstd = torch.stack([rec[1], (rec[2] / n + PN_EPS).rsqrt()]).float()
    # nine records of unequal counts, one of them empty, and nine sums records
    cuts = [0, 1, 4, 4, 200, 330, 331, 700, 1000, n]
    recs = torch.stack([_record(x[a:z]) if z > a else torch.zeros(3, PN_C, dtype=torch.float64) for a, z in zip(cuts[:-1], cuts[1:])])
    xhat = (x.double() - rec[1]) * mean_rstd[1].double()
    sums = torch.stack([torch.stack([dy[a:z].double().sum(0), (dy[a:z].double() * xhat[a:z]).sum(0)]) for a, z in zip(cuts[:-1], cuts[1:])])
    assert recs.shape == (PN_R, 3, PN_C) and sums.shape == (PN_R, 2, PN_C)
    d = {"x": x, "dy": dy, "weight": w, "bias": b, "running_mean": rm, "running_var": rv, "rec": rec, "mean_rstd": mean_rstd,
         "recs": recs, "sums": sums, "total_sums": sums.sum(0)}
    return {k: v.contiguous().to(device) for k, v in d.items()}


def _pn_make(*keys):
    def make(seed, device):
        d = _pn_operands(seed, device)
        return {k: d[k] for k in keys}
    return make


def _pn(name, keys, call):
    def run(d):
        from pasco_amd.grad.norm import ACTS
        from pasco_amd.grad.normlib import norm_lib
        out = call(norm_lib(), d, ACTS["leaky"])
        return out if isinstance(out, tuple) else (out,)
    return Entry("pn." + name, "pn", (name,), _pn_make(*keys), run)


_PN_ENTRIES = [
    _pn("moments", ("x",), lambda L, d, act: L.moments(d["x"])),
    _pn("moments_merge", ("recs",), lambda L, d, act: L.moments_merge(d["recs"])),
    _pn("finish", ("rec", "running_mean", "running_var"),
        lambda L, d, act: (L.finish(d["rec"], PN_EPS, PN_MOMENTUM, d["running_mean"], d["running_var"]), d["running_mean"],
                           d["running_var"])),
    _pn("apply", ("x", "mean_rstd", "weight", "bias"),
        lambda L, d, act: L.apply(d["x"], d["mean_rstd"], d["weight"], d["bias"], act, PN_SLOPE)),
    _pn("bwd_sums", ("dy", "x", "mean_rstd", "weight", "bias"),
        lambda L, d, act: L.bwd_sums(d["dy"], d["x"], d["mean_rstd"], d["weight"], d["bias"], act, PN_SLOPE)),
    _pn("sums_merge", ("sums",), lambda L, d, act: L.sums_merge(d["sums"])),
    _pn("bwd_dx", ("dy", "x", "mean_rstd", "weight", "bias", "total_sums", "rec"),
        lambda L, d, act: L.bwd_dx(d["dy"], d["x"], d["mean_rstd"], d["weight"], d["bias"], act, PN_SLOPE, d["total_sums"], d["rec"])),
]

# ---- po_* --------------------------------------------------------------------------------------------------------------------
PO_HYPER = [(1e-3, 0.9, 0.999, 1e-8, 0.1), (1e-3, 0.9, 0.999, 1e-8, 0.0)]
PO_MAX_NORM = 0.5


def _po_sizes():
    from pasco_amd.grad.optimlib import PO_CHUNK
    return [1 + i % 9 for i in range(36)] + [PO_CHUNK + 5]


def _make_po(seed, device):
    """One step's operands as four flat buffers (every tensor at a multiple of four elements), the records of a table that has
    taken three steps, and the two tables over the addresses of THIS dict's buffers."""
    from pasco_amd.grad.optim import _upload, build_tables
    from pasco_amd.grad.optimlib import STATE_DTYPE
    sizes, g = _po_sizes(), _gen(seed)
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 3) // 4 * 4
    T = len(sizes)
    d = {"p": torch.randn(total, generator=g), "g": torch.randn(total, generator=g) * 0.05,
         "m": torch.randn(total, generator=g) * 0.01, "v": torch.rand(total, generator=g) * 1e-3}
    rec = np.array([(3, 0.9 ** 3, 0.999 ** 3)] * T, dtype=STATE_DTYPE)
    d["states"] = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.float64).reshape(-1, 3).copy())
    d = {k: v.to(device) for k, v in d.items()}
    d["out_scalars"] = torch.empty((T, 8), dtype=torch.float32, device=device)
    d["result"] = torch.zeros(3, dtype=torch.float64, device=device)          # the skipped count is carried from step to step
    d["out_step"] = torch.empty(2, dtype=torch.int32, device=device)
    addr = lambda name, i: d[name].data_ptr() + 4 * offs[i]
    tab, chunks = build_tables([(i, i % 2, addr("p", i), addr("g", i), n) for i, n in enumerate(sizes)],
                               [addr("m", i) for i in range(T)], [addr("v", i) for i in range(T)])
    d["_tensors"], d["_chunks"], d["_counts"] = _upload(tab, device), _upload(chunks, device), (T, len(chunks))
    d["out_partials"] = torch.empty(len(chunks), dtype=torch.float64, device=device)
    return d


def _run_po(d):
    from pasco_amd.grad.optimlib import PO_POLICY_PROPAGATE, optim_lib
    lib, (T, C) = optim_lib(), d["_counts"]
    lib.sqnorm(d["_tensors"], T, d["_chunks"], C, d["out_partials"])
    lib.prepare(d["_tensors"], T, d["out_partials"], C, PO_HYPER, PO_MAX_NORM, 1.0, PO_POLICY_PROPAGATE, d["states"], d["out_scalars"],
                d["result"], d["out_step"])
    lib.adamw(d["_tensors"], T, d["_chunks"], C, d["out_scalars"], d["out_step"])
    return (d["p"], d["m"], d["v"], d["states"], d["out_scalars"], d["result"], d["out_step"], d["out_partials"])


# ---- pt_* --------------------------------------------------------------------------------------------------------------------
PT_GRID = (64, 64, 16)
PT_T = 13            # ten stuff classes (9 .. 18) and the three instance ids of tests/target_cases._scene
PT_ROWS = 1000
PT_CROP_U = ((0.3, 0.6, 0.1), (0.0, 0.0, 0.5))


def _pt_Ts():
    from tests.target_cases import lattice_T
    return [lattice_T(), lattice_T(flip_y=True, quarter_turns=1, shift_voxels=(3.0, -2.0, 1.0))]


def _pt_grids(seed, device, cut: bool = False):
    """The scene of tests/target_cases.py at this seed, with a fourth instance at a seeded place.  Which voxels are known does
    not depend on the seed, so neither do the bounds; with `cut` the layers from a seeded height up are unknown, so they do."""
    from tests.target_cases import _scene
    sem, ins = _scene(PT_GRID, seed)
    rng = np.random.default_rng(seed)
    x, y = int(rng.integers(10, 50)), int(rng.integers(10, 50))
    ins[x:x + 2, y:y + 2, 6:8] = 4
    if cut:
        z0 = 9 + int(seed) % 6
        sem[:, :, z0:] = 255
        ins[:, :, z0:] = 255
    return torch.from_numpy(sem).to(device), torch.from_numpy(ins).to(device)


def _pt_boxes(device):
    from pasco_amd.data.frame_lib import box_upper_bound
    from pasco_amd.data.target_lib import BOUNDS
    Ts = _pt_Ts()
    ub = box_upper_bound(PT_GRID, Ts)
    stride = (int((ub[:, 3:] - ub[:, :3] + 1).long().prod(dim=1).max()) + 15) // 16 * 16
    M = len(Ts)
    return Ts, ub, {"out_sem_box": torch.empty((M, stride), dtype=torch.uint8, device=device),
                    "out_ins_box": torch.empty((M, stride), dtype=torch.uint8, device=device),
                    "out_bounds": torch.empty((M, BOUNDS), dtype=torch.int32, device=device)}


def _make_pt_resample(seed, device, cut: bool = False):
    sem, ins = _pt_grids(seed, device, cut)
    Ts, ub, outs = _pt_boxes(device)
    return {"sem": sem, "ins": ins, "ub": ub.tolist(), **outs}


def _run_pt_resample(d):
    from pasco_amd.data.target_lib import target_lib
    Ts = _pt_Ts()
    target_lib().resample(d["sem"], d["ins"], Ts, [torch.inverse(T) for T in Ts], torch.tensor(d["ub"], dtype=torch.int32),
                          d["out_sem_box"], d["out_ins_box"], d["out_bounds"])
    return (d["out_sem_box"], d["out_ins_box"], d["out_bounds"])


def _pt_resampled(seed, device, cut: bool = False):
    """The box grids of one seed, their bounds on the host and the crop windows (`data.targets.prepare_targets` up to there)."""
    from pasco_amd.data.semantic_kitti import crop_window_from_bounds
    d = _make_pt_resample(seed, device, cut)
    for k in ("out_sem_box", "out_ins_box"):
        d[k].fill_(255)                         # bytes past a subnet's volume are not written: the same for every seed
    sem_box, ins_box, bounds = _run_pt_resample(d)
    hb = bounds.cpu()
    windows = torch.stack([crop_window_from_bounds(hb[m, 6:9], hb[m, 9:12], np.asarray(PT_CROP_U[m], dtype=np.float64))
                           for m in range(hb.shape[0])])
    return sem_box, ins_box, d["ub"], windows


def _make_pt_crop(seed, device, cut: bool = True):
    """With `cut` the box grids are those of a scene cut at a seeded height, under the windows of the uncut scene: the bounds
    of what the crop keeps then depend on the seed."""
    from pasco_amd.data.target_lib import CROP_BOUNDS
    sem_box, ins_box, ub, windows = _pt_resampled(seed, device, cut)
    if cut:
        windows = _pt_resampled(0, device)[3]
    return {"sem_box": sem_box, "ins_box": ins_box, "ub": ub, "windows": windows.tolist(),
            "out_cb": torch.empty((len(ub), CROP_BOUNDS), dtype=torch.int32, device=device)}


def _run_pt_crop(d):
    from pasco_amd.data.target_lib import target_lib
    target_lib().crop_bounds(d["sem_box"], d["ins_box"], torch.tensor(d["ub"], dtype=torch.int32),
                             torch.tensor(d["windows"], dtype=torch.float64), d["out_cb"])
    return (d["out_cb"],)


def _make_pt_labels(seed, device):
    """The geometry of the label grids follows `prepare_targets`: it depends on which voxels are known, and `_scene` makes the
    same ones known for every seed."""
    from pasco_amd.data.semantic_kitti import completion_bounds, compute_scene_size
    from pasco_amd.data.target_lib import TABLE
    from pasco_amd.data.targets import _union
    d = _make_pt_crop(seed, device, cut=False)
    hc = _run_pt_crop(d)[0].cpu()
    geo = []
    for m in range(hc.shape[0]):
        lo, hi = _union(hc[m, 0:3], hc[m, 3:6], hc[m, 6:9], hc[m, 9:12])
        min_c, max_c = completion_bounds(lo, hi, 8)
        scene = [int(v) for v in compute_scene_size(min_c, max_c, scale=8)]
        geo.append(([int(v) for v in min_c.tolist()], scene))
        n1 = scene[0] * scene[1] * scene[2]
        d[f"out_grids{m}"] = torch.empty(3 * n1 + 2 * (n1 // 8) + 2 * (n1 // 64), dtype=torch.uint8, device=device)
    del d["out_cb"]
    d["geo"] = geo
    d["out_table"] = torch.empty((len(geo), TABLE), dtype=torch.int32, device=device)
    return d


def _run_pt_labels(d):
    from pasco_amd.data.target_lib import target_lib
    outs = []
    for m, (min_c, scene) in enumerate(d["geo"]):
        n1 = scene[0] * scene[1] * scene[2]
        parts = torch.split(d[f"out_grids{m}"], [n1, n1, n1, n1 // 8, n1 // 8, n1 // 64, n1 // 64])
        shape = lambda s: (scene[0] // s, scene[1] // s, scene[2] // s)
        outs.append({"semantic": parts[0].view(shape(1)), "instance": parts[1].view(shape(1)), "geo_1": parts[2].view(shape(1)),
                     "geo_2": parts[3].view(shape(2)), "sem_2": parts[4].view(shape(2)), "geo_4": parts[5].view(shape(4)),
                     "sem_4": parts[6].view(shape(4)), "min_C": min_c, "scene": scene})
    target_lib().labels(d["sem_box"], d["ins_box"], torch.tensor(d["ub"], dtype=torch.int32),
                        torch.tensor(d["windows"], dtype=torch.float64), outs, 20, d["out_table"])
    return tuple(d[f"out_grids{m}"] for m in range(len(outs))) + (d["out_table"],)


def _make_pt_presence(seed, device):
    from pasco_amd.data.target_lib import TABLE
    sem, ins = _pt_grids(seed, device)
    return {"sem": sem, "ins": ins, "out_table": torch.empty(TABLE, dtype=torch.int32, device=device)}


def _run_pt_presence(d):
    from pasco_amd.data.target_lib import target_lib
    target_lib().presence(d["sem"], d["ins"], d["out_table"])
    return (d["out_table"],)


def _pt_slots(device):
    cls_slot, ins_slot = [-1] * 256, [-1] * 256
    for c in range(9, 19):
        cls_slot[c] = c - 9
    for i in (1, 2, 3):
        ins_slot[i] = 9 + i
    return torch.tensor(cls_slot, dtype=torch.int32, device=device), torch.tensor(ins_slot, dtype=torch.int32, device=device)


def _make_pt_masks(seed, device):
    sem, ins = _pt_grids(seed, device)
    cls_slot, ins_slot = _pt_slots(device)
    return {"sem": sem, "ins": ins, "cls_slot": cls_slot, "ins_slot": ins_slot}


def _run_pt_masks(d):
    from pasco_amd.data.target_lib import target_lib
    return (target_lib().masks(d["sem"], d["ins"], d["cls_slot"], d["ins_slot"], PT_T),)


def _make_pt_pack(seed, device):
    d = _make_pt_masks(seed, device)
    g = _gen(seed, 3)
    origin = (3, -2, 10)
    xyz = torch.stack([torch.randint(0, PT_GRID[a], (PT_ROWS,), generator=g) + origin[a] for a in range(3)], dim=1)
    d["coords"] = torch.cat([torch.full((PT_ROWS, 1), 9), xyz], dim=1).to(torch.int32).to(device)
    d["unknown"] = (d["sem"] == 255).to(torch.uint8)
    d["origin"] = origin
    return d


def _run_pt_pack(d):
    from pasco_amd.data.target_lib import target_lib
    return target_lib().target_pack(d["sem"], d["ins"], d["cls_slot"], d["ins_slot"], d["unknown"], d["coords"], PT_T, d["origin"])


# ---- the table ---------------------------------------------------------------------------------------------------------------
ENTRIES = [
    Entry("pg.nbr_invert", "pg", ("nbr_invert",), _make_nbr_invert, _run_nbr_invert),
    Entry("pg.conv_wgrad/32x32_2R+3", "pg", ("conv_wgrad",), _make_wgrad(32, 32, 2 * R + 3), _run_wgrad, two_streams=True),
    Entry("pg.conv_wgrad/256x256_R+1", "pg", ("conv_wgrad",), _make_wgrad(256, 256, R + 1), _run_wgrad),
    Entry("pg.colsum", "pg", ("colsum",), _make_colsum, _run_colsum),
    Entry("pr.dense_rows", "pr", ("dense_rows",), _make_dense_rows, _run_dense_rows),
    Entry("pr.rows_dense", "pr", ("rows_dense",), _make_rows_dense, _run_rows_dense),
    Entry("pr.maxpool_arg", "pr", ("maxpool_arg",), _make_maxpool_arg, _run_maxpool_arg),
    Entry("pr.maxpool_bwd", "pr", ("maxpool_bwd",), _make_maxpool_bwd, _run_maxpool_bwd),
    Entry("pa.attn_bwd_stats/1x2x40x50", "pa", ("attn_bwd_stats",), _make_attn((1, 2, 40, 50)), _run_attn_stats),
    Entry("pa.attn_bwd_stats/2x8x100x333", "pa", ("attn_bwd_stats",), _make_attn((2, 8, 100, 333)), _run_attn_stats),
    Entry("pa.attn_cross_bwd/1x2x40x50", "pa", ("attn_cross_bwd",), _make_attn((1, 2, 40, 50)), _run_attn_bwd),
    Entry("pa.attn_cross_bwd/2x8x100x333", "pa", ("attn_cross_bwd",), _make_attn((2, 8, 100, 333)), _run_attn_bwd, two_streams=True,
          caches_scratch=True),
    Entry("pm.target_pack", "pm", ("target_pack",), _make_pm_pack, _run_pm_pack),
    Entry("pm.pair_sums", "pm", ("pair_sums",), _make_pm_sums, _run_pm_sums, two_streams=True, caches_scratch=True),
    Entry("pm.mask_loss_bwd", "pm", ("mask_loss_bwd",), _pm_operands, _run_pm_bwd),
    Entry("ps.forward", "ps", ("rows_fwd", "sort_desc", "lovasz_fwd"), _make_sem_forward, _run_sem_forward, two_streams=True,
          caches_scratch=True),
    Entry("ps.rows_fwd", "ps", ("rows_fwd",), _make_sem_rows, _run_sem_rows),
    Entry("ps.sort_desc", "ps", ("sort_desc",), _make_sem_sort, _run_sem_sort),
    Entry("ps.lovasz_fwd", "ps", ("lovasz_fwd",), _make_sem_lovasz, _run_sem_lovasz),
    Entry("ps.loss_bwd", "ps", ("loss_bwd",), _make_sem_bwd, _run_sem_bwd),
] + _PN_ENTRIES + [
    Entry("po.step", "po", ("sqnorm", "prepare", "adamw"), _make_po, _run_po, step_keys=("g",)),
    Entry("pt.resample", "pt", ("resample",), _make_pt_resample, _run_pt_resample),
    Entry("pt.crop_bounds", "pt", ("crop_bounds",), _make_pt_crop, _run_pt_crop),
    Entry("pt.labels", "pt", ("labels",), _make_pt_labels, _run_pt_labels),
    Entry("pt.presence", "pt", ("presence",), _make_pt_presence, _run_pt_presence),
    Entry("pt.masks", "pt", ("masks",), _make_pt_masks, _run_pt_masks),
    Entry("pt.target_pack", "pt", ("target_pack",), _make_pt_pack, _run_pt_pack),
]
ENTRY_IDS = [e.name for e in ENTRIES]
PAIR_ENTRIES = [e for e in ENTRIES if e.two_streams]


# ---- the harness -------------------------------------------------------------------------------------------------------------
def bits_equal(a, b) -> bool:
    """Two results (tensors, None, or tuples of them) hold the same bits."""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(bits_equal(x, y) for x, y in zip(a, b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def operand_keys(d):
    return [k for k, v in d.items() if isinstance(v, torch.Tensor) and not k.startswith(("out", "_"))]


def same_constants(a, b):
    """Two dicts of one entry: the same keys, the same shapes and dtypes, the same host constants."""
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("_"):
            continue
        if isinstance(a[k], torch.Tensor):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{k}: the shapes of an entry are fixed"
        else:
            assert a[k] == b[k], f"{k}: a host constant differs between two seeds: {a[k]} / {b[k]}"


def poison(d):
    """Every output buffer filled with the poison pattern, on the current stream."""
    for k, v in d.items():
        if k.startswith("out"):
            v.view(torch.uint8).fill_(POISON)


def scrub(shapes, device):
    """Blocks of the results' sizes taken from the current stream's pool, poisoned in stream order and given back: a result
    the call allocates itself then starts from the poison pattern too, not from what an earlier run left in the block."""
    junk = [torch.empty(shape, dtype=dtype, device=device) for shape, dtype in shapes]
    for t in junk:
        t.view(-1).view(torch.uint8).fill_(POISON)


def load(work, real, keys=None):
    """Device-to-device copies of `real`'s operands into `work`'s, on the current stream."""
    for k in operand_keys(work) if keys is None else keys:
        work[k].copy_(real[k], non_blocking=True)


def eager(entry, seed, device, steps=None):
    """The call on the current stream with a dict of its own: `steps` = the seeds of the gradients of further steps (po)."""
    d = entry.make(seed, device)
    poison(d)
    out = entry.run(d)
    for s in steps or ():
        load(d, entry.make(s, device), entry.step_keys)
        out = entry.run(d)
    return tuple(None if t is None else t.clone() for t in out)


class Producer:
    """Work that keeps a stream busy for a given time: `torch.cuda._sleep` calibrated once with events, or, where torch has
    none, a chain of matrix products calibrated the same way."""

    def __init__(self, device):
        self.device = device
        self.sleep = getattr(torch.cuda, "_sleep", None)
        self.a = None if self.sleep is not None else torch.randn(1024, 1024, device=device)
        self.unit = 1_000_000 if self.sleep is not None else 8
        for _ in range(2):                       # the first launch loads the kernel
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(device)
            t0.record()
            self._issue(self.unit)
            t1.record()
            torch.cuda.synchronize(device)
            self.units_per_ms = self.unit / max(t0.elapsed_time(t1), 1e-3)

    def _issue(self, units):
        if self.sleep is not None:
            self.sleep(int(units))
        else:
            x = self.a
            for _ in range(int(units)):
                x = (x @ self.a) * 1e-3
            self._keep = x

    def run(self, ms: float):
        """Enqueue `ms` milliseconds of work on the current stream."""
        self._issue(max(1, int(ms * self.units_per_ms)))


def overtakes(first, second, producer: Producer, device, ms: float = 2.0) -> bool:
    """Work issued on `second` after pending work on `first` runs before it: the two streams do not share a hardware queue
    and neither waits for the other."""
    flag, seen = torch.zeros(1, device=device), torch.ones(1, device=device)
    torch.cuda.synchronize(device)
    with torch.cuda.stream(first):
        producer.run(ms)
        flag.fill_(1.0)
    with torch.cuda.stream(second):
        seen.copy_(flag)
    torch.cuda.synchronize(device)
    return float(seen) == 0.0


class SideStreams:
    """Side streams for the checks, chosen by measurement.  A process has a few hardware queues and torch hands out its pool
    of streams round robin, so some side streams share the null stream's queue: a launch that lost its stream argument would
    still run in order there and nothing could be seen.  `streams` are streams that the null stream demonstrably overtakes and
    that overtake each other; `tried` is how many of torch's streams were looked at."""

    def __init__(self, device, producer: Producer, want: int = 2, tries: int = 32):
        self.device, self.streams, self.tried, self.shared = device, [], 0, 0
        null = torch.cuda.default_stream(device)
        seen = set()
        while len(self.streams) < want and self.tried < tries:
            s = torch.cuda.Stream(device)
            self.tried += 1
            if s.cuda_stream in seen:
                continue
            seen.add(s.cuda_stream)
            if overtakes(s, null, producer, device) and all(overtakes(s, t, producer, device) and overtakes(t, s, producer, device)
                                                            for t in self.streams):
                self.streams.append(s)
            else:
                self.shared += 1

    def one(self):
        assert self.streams, (f"none of {self.tried} side streams runs concurrently with the null stream: a mis-streamed launch "
                              f"cannot be seen here and the method is void")
        return self.streams[0]

    def two(self):
        assert len(self.streams) >= 2, f"of {self.tried} side streams fewer than two run concurrently with each other and the null stream"
        return self.streams[0], self.streams[1]


class OrderReport(NamedTuple):
    name: str
    host_ms: float
    producer_ms: float
    busy: bool
    failures: tuple


def order_check(entry: Entry, device, producer: Producer, stream=None, seeds=(SEED_A, SEED_B), need_busy: bool = True) -> OrderReport:
    """Part 2: the call on a side stream (`SideStreams.one()`; a fresh one if none is given) behind a pending producer, its
    operands copied in stream order behind the producer as well.  -> the report; `failures` is empty when the call kept the
    contract."""
    A, B = seeds
    real, work, warm1, warm2 = entry.make(A, device), entry.make(B, device), entry.make(B, device), entry.make(B, device)
    same_constants(real, work)
    s = torch.cuda.Stream(device) if stream is None else stream
    torch.cuda.synchronize(device)
    try:
        with torch.cuda.stream(s):
            poison(warm1), poison(warm2)
            entry.run(warm1)                     # per-stream workspaces, cached tables, the allocator's blocks of this stream
            s.synchronize()
            t0 = time.perf_counter()
            warm_out = entry.run(warm2)
            host_ms = (time.perf_counter() - t0) * 1e3
            s.synchronize()
            shapes = [(t.shape, t.dtype) for t in warm_out if t is not None and t.numel()]
            del warm_out
        length = max(FLOOR_MS, HOST_FACTOR * host_ms)
        torch.cuda.synchronize(device)
        with torch.cuda.stream(s):
            producer.run(length)
            load(work, real)
            poison(work)
            scrub(shapes, device)
            got = entry.run(work)
            busy = not s.query()
            s.synchronize()
        got = tuple(None if t is None else t.clone() for t in got)
        torch.cuda.synchronize(device)
    finally:
        release(s)
    want = eager(entry, A, device)
    other = eager(entry, B, device)
    torch.cuda.synchronize(device)
    failures = []
    if not bits_equal(got, want):
        bad = [i for i, (x, y) in enumerate(zip(got, want)) if not bits_equal(x, y)]
        failures.append(f"{entry.name}: the stream run differs from the default-stream run in result(s) {bad}: a launch, a memset "
                        f"or a copy did not wait for the stream it was given")
    if bits_equal(want, other):
        failures.append(f"{entry.name}: the two seeds give the same result, so the comparison shows nothing")
    if need_busy and not busy:
        failures.append(f"{entry.name}: the stream had drained when the call returned (producer {length:.1f} ms, host time of the "
                        f"warm call {host_ms:.3f} ms): the producer was too short or the call blocked on the device")
    return OrderReport(entry.name, host_ms, length, busy, tuple(failures))


def release(stream) -> int:
    from pasco_amd.me.backend import hip_backend
    return hip_backend().release_stream(stream)


def pair_check(entry: Entry, device, producer: Producer, pair=None, seeds=PAIR_SEEDS):
    """Part 3: two streams (`SideStreams.two()`) released by one event on a third run the call alternately, two rounds on
    different seeds each.  -> (failures, the counts of the first and the second release_stream per stream)."""
    s0, s1 = (torch.cuda.Stream(device), torch.cuda.Stream(device)) if pair is None else pair
    p = torch.cuda.Stream(device)
    dicts = [entry.make(x, device) for x in seeds]
    warm = [entry.make(SEED_B, device) for _ in range(2)]
    torch.cuda.synchronize(device)
    try:
        for s, w in zip((s0, s1), warm):
            with torch.cuda.stream(s):
                poison(w)
                entry.run(w)
        torch.cuda.synchronize(device)
        ev = torch.cuda.Event()
        with torch.cuda.stream(p):
            producer.run(FLOOR_MS)
            ev.record()
        s0.wait_event(ev), s1.wait_event(ev)
        got = []
        for i, d in enumerate(dicts):            # s0, s1, s0, s1
            with torch.cuda.stream((s0, s1)[i % 2]):
                poison(d)
                got.append(entry.run(d))
        torch.cuda.synchronize(device)
        got = [tuple(None if t is None else t.clone() for t in g) for g in got]
    finally:
        first = [release(s) for s in (s0, s1)]
        second = [release(s) for s in (s0, s1)]
    failures = []
    for i, x in enumerate(seeds):
        if not bits_equal(got[i], eager(entry, x, device)):
            failures.append(f"{entry.name}: call {i} (stream {i % 2}) differs from its serial default-stream run")
    torch.cuda.synchronize(device)
    return failures, first, second


def capture_check(entry: Entry, device, stream=None, seeds=(SEED_A, SEED_B)):
    """Part 4: one call captured on a side stream, new values copied into the captured operands, one replay.  For an entry with
    `step_keys` (po) the warm call runs on the captured operands themselves, so the replay is one more step: it is held to two
    eager steps.  -> failures."""
    A, B = seeds
    s = torch.cuda.Stream(device) if stream is None else stream
    work, new = entry.make(B, device), entry.make(A, device)
    warm = work if entry.step_keys is not None else entry.make(B, device)
    torch.cuda.synchronize(device)
    try:
        with torch.cuda.stream(s):
            poison(warm)
            entry.run(warm)
        torch.cuda.synchronize(device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s, capture_error_mode="thread_local"):
            outs = entry.run(work)
        load(work, new, entry.step_keys)
        if entry.step_keys is None:
            poison(work)
        torch.cuda.synchronize(device)
        g.replay()
        torch.cuda.synchronize(device)
        got = tuple(None if t is None else t.clone() for t in outs)
        del g, outs
    finally:
        release(s)
    want = eager(entry, B, device, steps=(A,)) if entry.step_keys is not None else eager(entry, A, device)
    torch.cuda.synchronize(device)
    if not bits_equal(got, want):
        bad = [i for i, (x, y) in enumerate(zip(got, want)) if not bits_equal(x, y)]
        return [f"{entry.name}: the replay differs from the eager call on the same values in result(s) {bad}"]
    return []
