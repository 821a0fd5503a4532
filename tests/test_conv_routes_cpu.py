"""CPU side of tests/test_hip_conv_routes.py: the element-wise bound of tests/conv_ref64.py rejects the corruptions a wrong
kernel produces (and passes the fp32 oracle), `CBackend.weight_fragments` equals a loop restatement of its documented layout, and
the caches keyed on tensor versions work on inference tensors (torch.inference_mode())."""
import pytest
import torch

from pasco_amd.me.backend import CBackend
from pasco_amd.me.core import kernel_offsets
from tests.conv_ref64 import epilogue64, gather_sum64, violations, worst_ratio


def _layer(oracle):
    """A stride-1 3x3x3 layer of 64 -> 48 channels on 300 output rows (2 row tiles + ragged) of a 700-row input, with
    rows that have no neighbour, and the full epilogue: bias, signed BN, leaky ReLU, second BN, table rows, residual, res_act."""
    g = torch.Generator().manual_seed(11)
    sites = torch.randperm(16 * 16 * 8, generator=g)[:700]
    coords = torch.stack([torch.zeros_like(sites), sites // 128, (sites // 8) % 16, sites % 8], 1).int().contiguous()
    tk, tv, _, _, _ = oracle.map_insert(coords, dedup=False)
    n_out = 300
    nbr = oracle.nbr_build(coords[:n_out].contiguous(), tk, tv, kernel_offsets(3, 1))
    nbr[:, 5] = -1                                     # an isolated row
    cin, cout = 64, 48
    x = torch.randn(700, cin, generator=g)
    w = torch.randn(27, cin, cout, generator=g) / (27 * cin / 2) ** 0.5
    T, lo = 12, -2
    spec = dict(bias=torch.randn(cout, generator=g),
                epi_scale=(torch.rand(cout, generator=g) + 0.5) * torch.where(torch.rand(cout, generator=g) < 0.3, -1.0, 1.0),
                epi_shift=torch.randn(cout, generator=g) * 0.1, epi_act=2, slope=0.1,
                epi2_scale=torch.rand(cout, generator=g) + 0.5, epi2_shift=torch.randn(cout, generator=g) * 0.1,
                axis=(torch.randn(3, T, cout, generator=g),
                      torch.cat([torch.zeros(n_out, 1, dtype=torch.int32),
                                 torch.randint(lo, lo + T - 1, (n_out, 3), generator=g, dtype=torch.int32)], 1).contiguous(), lo),
                residual=torch.randn(n_out, cout, generator=g), res_act=2)
    return x, w, nbr, n_out, spec


def _ref(x, w, nbr, n_out, spec):
    rows = torch.arange(n_out)
    acc, mag = gather_sum64(x, w, nbr, rows)
    return epilogue64(acc, mag, spec, rows)


def test_bound_passes_the_fp32_oracle(oracle):
    x, w, nbr, n_out, spec = _layer(oracle)
    ref, a, e = _ref(x, w, nbr, n_out, spec)
    got = oracle.conv_fwd(x, w, nbr, n_out, **spec)
    assert not bool(violations(got, ref, a, e).any()), worst_ratio(got, ref, a, e)
    assert not bool(violations(ref.float(), ref, a, e).any())
    # the isolated row is the epilogue of the bias alone: its magnitude A is 0, the bound there is the rounding allowance only
    assert float(a[5].abs().max()) == 0.0


def _corruptions(x, w, nbr, n_out, spec, ref):
    """-> {name: fp32 result of a kernel with that bug}"""
    out = {}
    r = 77
    k = int((nbr[:, r] >= 0).nonzero()[0])
    nb = nbr.clone()
    nb[k if k != 13 else int((nbr[:, r] >= 0).nonzero()[1]), r] = -1
    out["offset dropped for one row"] = _ref(x, w, nb, n_out, spec)[0].float()
    s = dict(spec, bias=spec["bias"].clone())
    s["bias"][7] = 0.0
    out["one column's bias missing"] = _ref(x, w, nbr, n_out, s)[0].float()
    s = dict(spec, residual=spec["residual"].clone())
    s["residual"][r] *= 2
    out["residual added twice on one row"] = _ref(x, w, nbr, n_out, s)[0].float()
    tab, coords, lo = spec["axis"]
    c2 = coords.clone()
    c2[r, 2] += 1                                  # y table row of the neighbouring entry (still inside the table)
    out["axis row of the neighbouring entry"] = _ref(x, w, nbr, n_out, dict(spec, axis=(tab, c2, lo)))[0].float()
    g = ref.float().clone()
    g[-1] = 0.0
    out["last ragged row unwritten"] = g
    g = ref.float().clone()
    i = int(ref.abs().argmax())
    g.view(-1)[i] = float(ref.view(-1)[i]) * (1 + 2.0 ** -12)
    out["one element off by 2^-12 relative"] = g
    return out


def test_bound_rejects_realistic_corruptions(oracle):
    x, w, nbr, n_out, spec = _layer(oracle)
    ref, a, e = _ref(x, w, nbr, n_out, spec)
    for name, got in _corruptions(x, w, nbr, n_out, spec, ref).items():
        bad = violations(got, ref, a, e)
        assert bool(bad.any()), f"the bound lets '{name}' through"


# ---- CBackend.weight_fragments -----------------------------------------------------------------------------------------------
def _frag_loop(w_split, kvol, cout, cpad):
    """The documented layout (backend.py): f16 [kvol, cpad / 16, 2 (column block j), 2 (hi, lo), 64 (lane = l31 + 32 h), 8]: the
    lane's 8 channels 16 c + 8 h .. + 7 of column min(32 j + l31, cout - 1); w_split rows are (k, column), [cpad / 32, 2, 32]."""
    ws = w_split.view(kvol, cout, cpad // 32, 2, 32)
    out = torch.empty(kvol, cpad // 16, 2, 2, 64, 8, dtype=w_split.dtype)
    for k in range(kvol):
        for c in range(cpad // 16):
            for j in range(2):
                for lane in range(64):
                    col = min(32 * j + lane % 32, cout - 1)
                    ch = 16 * c + 8 * (lane // 32)
                    for p in range(2):
                        out[k, c, j, p, lane] = ws[k, col, ch // 32, p, ch % 32: ch % 32 + 8]
    return out


@pytest.mark.parametrize("cout", [33, 40, 48, 63, 64])
@pytest.mark.parametrize("cpad", [32, 64, 96, 256])
def test_weight_fragments_match_the_documented_layout(cout, cpad):
    kvol = 2
    g = torch.Generator().manual_seed(cout * 1000 + cpad)
    w_split = torch.randn(kvol * cout, cpad // 32, 2, 32, generator=g).half()
    frag = CBackend.weight_fragments(w_split, kvol, cout, cpad)
    assert frag.shape == (kvol, cpad // 16, 2, 2, 64, 8) and frag.is_contiguous()
    assert torch.equal(frag.view(torch.int16), _frag_loop(w_split, kvol, cout, cpad).view(torch.int16))
    assert CBackend.weight_fragments(w_split, kvol, cout, cpad) is frag            # cached on the operand


def test_weight_fragments_under_inference_mode():
    """An operand made under torch.inference_mode() is an inference tensor: no version counter to read."""
    kvol, cout, cpad = 27, 48, 64
    with torch.inference_mode():
        w_split = torch.randn(kvol * cout, cpad // 32, 2, 32, generator=torch.Generator().manual_seed(3)).half()
        assert w_split.is_inference()
        frag = CBackend.weight_fragments(w_split, kvol, cout, cpad)
        assert CBackend.weight_fragments(w_split, kvol, cout, cpad) is frag
    assert torch.equal(frag.view(torch.int16), _frag_loop(w_split, kvol, cout, cpad).view(torch.int16))


def test_version_keyed_caches_on_inference_tensors(oracle_registered):
    """The drop-in modules built AND run under torch.inference_mode(): parameters, masks and operands are inference tensors."""
    import pasco_amd.me as ME
    from pasco_amd.me.core import tensor_version

    with torch.inference_mode():
        t = torch.zeros(3)
        assert tensor_version(t) is None
    assert tensor_version(torch.zeros(3)) == 0
    g = torch.Generator().manual_seed(5)
    sites = torch.randperm(12 * 12 * 6, generator=g)[:400]
    coords = torch.stack([torch.zeros_like(sites), sites // 72, (sites // 6) % 12, sites % 6], 1).int()
    feats = torch.randn(400, 16, generator=g)
    oracle_registered.checker_split = True
    try:
        with torch.inference_mode():
            torch.manual_seed(1)
            conv = ME.MinkowskiConvolution(16, 16, kernel_size=3, bias=True, dimension=3).eval()
            bn = ME.MinkowskiBatchNorm(16).eval()
            prune = ME.MinkowskiPruning()
            assert conv.kernel.is_inference()
            x = ME.SparseTensor(feats, coords)
            y1 = bn(conv(x))
            y2 = bn(conv(x))
            keep = y1.F[:, 0] > 0
            p1, p2 = prune(y1, keep), prune(y2, keep)
            conv.kernel.mul_(2.0)                  # in-place update of an inference parameter: no version counter to see it
            y3 = conv(x)
    finally:
        oracle_registered.checker_split = False
    assert torch.equal(y1.F, y2.F) and torch.equal(p1.F, p2.F) and p1.F.shape[0] == int(keep.sum())
    with torch.no_grad():
        torch.manual_seed(1)
        ref_conv = ME.MinkowskiConvolution(16, 16, kernel_size=3, bias=True, dimension=3).eval()
        ref = ref_conv(ME.SparseTensor(feats, coords)).F
        ref_conv.kernel.mul_(2.0)
        ref2 = ref_conv(ME.SparseTensor(feats, coords)).F
    assert torch.allclose(y3.F, ref2, rtol=1e-5, atol=1e-5) and not torch.allclose(y3.F, ref, rtol=1e-3, atol=1e-3)
