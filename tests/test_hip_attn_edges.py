"""The attention edge cases of tests/attn_edge_cases.py on libpascohip.so (csrc/attn.hip), held to the fp64 reference of
tests/attn_ref64.py (the same cases run on the C oracle in tests/test_attn_edges_cpu.py), and one leg at the size of the
benchmark scene's finest level."""
import pytest
import torch

from tests import attn_ref64 as ref
from tests.attn_edge_cases import CASES, DH, Problem, angle_eps, pack, run_feat, run_fwd, run_split

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.__name__)
def test_attn_edges_hip(hip, case):
    case(hip, torch.device("cuda", 0))


def test_attn_edges_full_size(hip):
    """(B, H, Q, N) = (3, 8, 100, 210 542), the voxel count of the benchmark scene's finest level: 6580 tiles of
    32 keys in 21 ranges of 314 per head, the last range 300 and the last tile 14 keys.  Elements 0 and 2 allow every query
    exactly one key, the last one (every range but the last hands the merge an empty partial); element 1 is unmasked.
    fp64 on output rows only, never on a stored score tensor: all 2400 (b, h, q) rows, one (b, h) at a time."""
    dev = torch.device("cuda", 0)
    B, H, Q, N = 3, 8, 100, 210542
    g = torch.Generator(device=dev).manual_seed(210542)
    q = torch.randn(B, H, Q, DH, device=dev, generator=g) * DH ** -0.5
    k = torch.randn(B * N, H * DH, device=dev, generator=g) * 1.7
    v = torch.randn(B * N, H * DH, device=dev, generator=g)
    allow = torch.zeros(B, N, Q, dtype=torch.bool, device=dev)
    allow[:, N - 1] = True
    allow[1] = True
    bits, any_ = pack(hip, dev, allow)
    ks, vs = hip.split_rows(k), hip.split_rows(v)
    del k, v
    exp, scale = ref.attention(q, ref.unsplit64(ks, H * DH).view(B, N, -1), ref.unsplit64(vs, H * DH).view(B, N, -1), allow)
    ratios = {}
    got, rc = run_split(hip, dev, q, ks, vs, N, bits, any_)
    assert rc == 0
    ratios["split"] = ref.ratio(got, exp, scale)
    k2, v2 = ref.unsplit(ks, H * DH).view(B, N, -1).contiguous(), ref.unsplit(vs, H * DH).view(B, N, -1).contiguous()
    del ks, vs
    got, rc = run_fwd(hip, dev, q, k2, v2, bits, any_)
    assert rc == 0
    ratios["fwd"] = ref.ratio(got, exp, scale)
    del k2, v2, exp, scale
    p = Problem(1, H, Q, 1, seed=5)                                      # the Q2 recipe; the rows are drawn on the device
    q2 = p.q2.expand(B, H, Q, -1).contiguous().to(dev) * (1 + 0.1 * torch.rand(B, 1, 1, 1, device=dev, generator=g))
    x = torch.randn(B * N, 64, device=dev, generator=g) * torch.rand(B * N, 1, device=dev, generator=g) * 3
    coords = torch.randint(-2, 260, (B * N, 4), device=dev, generator=g, dtype=torch.int32)
    eps, lo = angle_eps(dev)
    xs, aug = hip.split_rows(x), hip.pos_aug(coords, eps, lo)
    r = ref.feat_rows(xs, aug, B, N)
    exp, scale = ref.attention(q2, r, r, allow, per_head=False)
    got, rc = run_feat(hip, dev, q2, xs, aug, N, bits, any_)
    assert rc == 0
    ratios["feat"] = ref.ratio(got, exp, scale)
    hip.check_status(dev)
    for kname, x in ratios.items():
        print(f"ATTN_RATIO full_size B{B} H{H} Q{Q} N{N} {kname} {x:.4f}")
    assert all(x <= 1.0 for x in ratios.values()), ratios
