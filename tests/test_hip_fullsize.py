"""Full-size (S10: 256x256x32 at ~10 % occupancy, ~210 k voxels) GPU checks through size-independent
properties - no oracle run at this size:
  * insert -> find round trip, idempotent re-insert, dedup of a doubled input
  * kernel-map symmetry: (i -> o at offset k) <=> (o -> i at offset K-1-k) for the centred k=3 kernel
  * linearity of the sparse convolution, equality with a per-offset torch formulation on a row sample
  * prune is order preserving and idempotent; union(a, b) covers both, lhs first
  * stride / generative expansion: every fine voxel has exactly one parent; children of parents tile
  * dense <-> sparse round trip
plus the whole MIMO graph on config-shaped variants (KITTI-360 channel counts, heavy decoder) against
the CPU oracle on a reduced grid."""
import numpy as np
import pytest
import torch

import pasco_amd.me as ME
from pasco_amd.graph.synth import make_occupancy, make_scene, TeacherKeep
from pasco_amd.me.core import kernel_offsets

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def s10():
    g1 = np.argwhere(make_occupancy(0))
    c = torch.from_numpy(np.ascontiguousarray(np.concatenate([np.zeros((g1.shape[0], 1), np.int64), g1], 1)))
    return c.int().cuda().contiguous()


def test_insert_find_roundtrip_and_dedup(hip, s10):
    n = s10.shape[0]
    tk, tv, r2u, uq, nu = hip.map_insert(s10)
    assert nu == n and torch.equal(r2u, torch.arange(n, dtype=torch.int32, device="cuda"))
    assert torch.equal(hip.map_find(s10, tk, tv), r2u)
    doubled = torch.cat([s10, s10.flip(0)]).contiguous()
    _, _, r2u2, uq2, nu2 = hip.map_insert(doubled)
    assert nu2 == n and torch.equal(uq2, torch.arange(n, dtype=torch.int32, device="cuda"))
    assert torch.equal(r2u2[n:], torch.arange(n - 1, -1, -1, dtype=torch.int32, device="cuda"))
    shifted = (s10 + torch.tensor([0, 1000, 0, 0], dtype=torch.int32, device="cuda")).contiguous()
    assert int((hip.map_find(shifted, tk, tv) >= 0).sum()) == 0


def test_kernel_map_symmetry_and_counts(hip, s10):
    n = s10.shape[0]
    tk, tv, _, _, _ = hip.map_insert(s10, dedup=False)
    nbr = hip.nbr_build(s10, tk, tv, kernel_offsets(3, 1))
    assert torch.equal(nbr[13], torch.arange(n, dtype=torch.int32, device="cuda"))      # centre offset = identity
    pin, pout, cnt = hip.kmap_compact(nbr)
    cnt = cnt.tolist()
    assert cnt[13] == n and all(cnt[k] == cnt[26 - k] for k in range(27))
    for k in (0, 5, 12):
        i, o = pin[k, :cnt[k]].long(), pout[k, :cnt[k]].long()
        assert torch.equal(nbr[26 - k][i], o.int())                                        # mirrored pair exists
        assert bool((o[1:] > o[:-1]).all())                                                # pairs sorted by out row
    assert 14.0 < sum(cnt) / n < 17.0                                                      # S10: ~15.4 pairs / voxel


def test_conv_linearity_and_row_sample(hip, s10):
    n = s10.shape[0]
    tk, tv, _, _, _ = hip.map_insert(s10, dedup=False)
    nbr = hip.nbr_build(s10, tk, tv, kernel_offsets(3, 1))
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(n, 64, device="cuda", generator=g)
    y = torch.randn(n, 64, device="cuda", generator=g)
    w = torch.randn(27, 64, 64, device="cuda", generator=g) / 40
    cx, cy = hip.conv_fwd(x, w, nbr, n), hip.conv_fwd(y, w, nbr, n)
    cz = hip.conv_fwd(2.0 * x - 0.5 * y, w, nbr, n)
    assert torch.allclose(cz, 2.0 * cx - 0.5 * cy, rtol=1e-3, atol=1e-4)
    rows = torch.randint(0, n, (2000,), device="cuda", generator=g)
    ref = torch.zeros(2000, 64, device="cuda", dtype=torch.float64)
    for k in range(27):
        idx = nbr[k][rows].long()
        ok = idx >= 0
        ref[ok] += x[idx[ok]].double() @ w[k].double()
    assert torch.allclose(cx[rows], ref.float(), rtol=1e-3, atol=1e-4)


def test_prune_union_stride_expand_properties(hip, oracle):
    from pasco_amd.me import backend
    g1 = np.argwhere(make_occupancy(0))
    c = torch.from_numpy(np.concatenate([np.zeros((g1.shape[0], 1), np.int64), g1], 1)).int().cuda()
    x = ME.SparseTensor(torch.randn(c.shape[0], 8, device="cuda"), c)
    prune = ME.MinkowskiPruning()
    m = x.F[:, 0] > 0
    p = prune(x, m)
    assert torch.equal(p.C, x.C[m]) and torch.equal(p.F, x.F[m])
    pp = prune(p, torch.ones(p.F.shape[0], dtype=torch.bool, device="cuda"))
    assert torch.equal(pp.C, p.C) and torch.equal(pp.F, p.F)
    q = prune(x, x.F[:, 1] > 0)
    u = p + q
    both = m | (x.F[:, 1] > 0)
    assert u.F.shape[0] == int(both.sum()) and torch.equal(u.C[: p.F.shape[0]], p.C)
    rows = x.coordinate_manager.find(u.coordinate_map_key, x.C[both].contiguous())
    assert int((rows < 0).sum()) == 0
    exp = torch.where(m[both][:, None], x.F[both], torch.zeros_like(x.F[both])) + \
        torch.where((x.F[:, 1] > 0)[both][:, None], x.F[both], torch.zeros_like(x.F[both]))
    assert torch.allclose(u.F[rows.long()], exp)
    # stride 2: every voxel has exactly one parent; the parents' children cover the voxels
    mgr = x.coordinate_manager
    k2 = mgr.stride(x.coordinate_map_key, 2)
    nbr = mgr.kernel_map(x.coordinate_map_key, k2, 2)
    assert int((nbr >= 0).sum()) == x.F.shape[0]
    kids = mgr.expand(k2, 2)
    assert mgr.size(kids) == 8 * mgr.size(k2)
    assert int((mgr.find(kids, x.C) < 0).sum()) == 0
    # dense round trip on the canonical grid
    d, _, _ = x.dense(shape=torch.Size([1, 8, 256, 256, 32]), min_coordinate=torch.IntTensor([0, 0, 0]))
    t = ME.to_sparse(d)
    assert torch.equal(t.C, x.C) and torch.equal(t.F, x.F)        # S10 rows are already lexicographic


@pytest.mark.parametrize("cfg", [dict(n_classes=19, in_channels=8, heavy=True, n_infers=2),
                                 dict(n_classes=20, in_channels=16, heavy=False, n_infers=3),
                                 dict(n_classes=19, in_channels=8, heavy=False, n_infers=3),    # BASELINE config 4
                                 dict(n_classes=20, in_channels=16, heavy=False, n_infers=8)])  # config 5's arithmetic
def test_config_shaped_graphs_vs_oracle(hip, oracle, cfg):
    """BASELINE.json configurations on the HIP path against the oracle on a reduced grid: SSCBench-KITTI360-shaped
    graphs (8 input channels, 19 classes; scripts/train_kitti360.py:115,152) with M = 2 (heavy decoder) and M = 3
    (config 4), SemanticKITTI-shaped MIMO-3 (config 3) and the M = 8 graph whose heads config 5 spreads over 8 GPUs
    (decoder_v3.py:211-229: occ_thres is only dereferenced when training, so M = 8 works at test time)."""
    from pasco_amd.graph import PascoNet
    from pasco_amd.me import backend
    torch.manual_seed(11)
    net = PascoNet(n_classes=cfg["n_classes"], n_infers=cfg["n_infers"], in_channels=cfg["in_channels"], f=16,
                   num_queries=10, heavy_decoder=cfg["heavy"]).eval()
    scene = make_scene(9, n_infers=cfg["n_infers"], in_channels=cfg["in_channels"], grid=(40, 40, 8), occupancy=0.12)

    def run(device):
        n, sc = net.to(device), scene.to(device)
        tk = TeacherKeep(sc, device)
        with torch.no_grad():
            x = n.prepare_input(sc.in_feats, sc.in_coords)
            return n(x, sc.global_min_Cs, sc.global_max_Cs, sc.min_Cs, sc.max_Cs, keep_override=tk)

    got = run(torch.device("cuda"))
    backend.register_checker_backend(oracle)
    try:
        exp = run(torch.device("cpu"))
    finally:
        backend.register_checker_backend(None)
    for s in exp["sem_logits_at_scales"]:
        for a, b in zip(got["sem_logits_at_scales"][s], exp["sem_logits_at_scales"][s]):
            assert torch.equal(a.C.cpu(), b.C)
            assert a.F.shape[1] == cfg["n_classes"]
            assert torch.allclose(a.F.cpu(), b.F, rtol=1e-3, atol=1e-3)
    for a, b in zip(got["panop_predictions"], exp["panop_predictions"]):
        assert torch.equal(a["voxel_logits"].C.cpu(), b["voxel_logits"].C)
        assert torch.allclose(a["voxel_logits"].F.cpu(), b["voxel_logits"].F, rtol=2e-3, atol=2e-3)
        assert torch.allclose(a["query_logits"].cpu(), b["query_logits"], rtol=2e-3, atol=2e-3)


def test_graft_entry_smoke(hip):
    """The driver's smoke(): one small MIMO-2 scene, HIP vs oracle."""
    import __graft_entry__ as g
    g.smoke()


def test_subnet_parallel_forward_nccl_world1(hip):
    """The C4 exchange path (`subnet_parallel_forward`: trunk, own heads, variable-size all-gather of per-voxel
    logits) under torch.distributed with the RCCL backend on one GPU / world size 1: same predictions as the plain
    forward.  The 2-rank semantics are covered on gloo (tests/test_dist_gloo.py); 8 GPUs are the driver's to run."""
    import socket
    import torch.distributed as dist
    from pasco_amd.graph import PascoNet
    from pasco_amd.graph.dist import subnet_parallel_forward
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dev = torch.device("cuda", 0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        torch.manual_seed(13)
        net = PascoNet(n_classes=20, n_infers=4, in_channels=16, f=16, num_queries=10, heavy_decoder=False).eval().to(dev)
        sc = make_scene(3, n_infers=4, in_channels=16, grid=(40, 40, 8), occupancy=0.12).to(dev)
        tk = TeacherKeep(sc, dev)
        with torch.no_grad():
            x = net.prepare_input(sc.in_feats, sc.in_coords)
            args = (x, sc.global_min_Cs, sc.global_max_Cs, sc.min_Cs, sc.max_Cs)
            ref = net(*args, keep_override=tk)
            got = subnet_parallel_forward(net, *args, keep_override=tk)
        assert len(got["panop_predictions"]) == 4
        for a, b in zip(got["panop_predictions"], ref["panop_predictions"]):
            assert torch.equal(a["voxel_logits"].C, b["voxel_logits"].C)
            assert torch.allclose(a["voxel_logits"].F, b["voxel_logits"].F, rtol=1e-4, atol=1e-5)
            assert torch.allclose(a["query_logits"], b["query_logits"], rtol=1e-4, atol=1e-5)
        # round 5: the site-sharded ensembler + panoptic stage on RCCL (all_reduce of the occupancy bytes, all_to_all of
        # the mask slabs, all_gather of the matching partials, all_reduce of the panoptic areas) == the single-process
        # stage on the same predictions, bit for bit (the 2 / 4-rank semantics: tests/test_dist_gloo.py)
        from pasco_amd.graph.dist import gather_sharded, site_sharded_ensemble, site_sharded_panoptic
        net.ensembler.scene_size = (40, 40, 8)
        from pasco_amd.graph.ensemble import GRAM_SLABS
        net.ensembler.gram_slabs = GRAM_SLABS              # the reference adds the slabs in the sharded run's order
        with torch.no_grad():
            _, _, ens_ref = net.ensemble(got, sc.Ts)
            pi_ref = net.panoptic(ens_ref)
            _, sharded, st = site_sharded_ensemble(net, got, sc.Ts)
            full = gather_sharded(net, sharded)
            pis = site_sharded_panoptic(net, sharded)
        assert len(full) == len(ens_ref) == 5 and st["collectives"] >= 3
        for a, b in zip(full, ens_ref):
            assert torch.equal(a["voxel_probs"].C, b["voxel_probs"].C) and torch.equal(a["voxel_probs"].F, b["voxel_probs"].F)
            assert torch.equal(a["sem_probs"].F, b["sem_probs"].F) and torch.equal(a["query_probs"], b["query_probs"])
        for p, r in zip(pis, pi_ref):
            assert torch.equal(p["panoptic"], r["panoptic_seg_sparses"][0])
            assert [s["query_id"] for s in p["segments_infos"]] == [s["query_id"] for s in r["segments_infos"][0]]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_flight", [2, 3])
def test_scenes_in_flight_match_one_at_a_time(hip, n_flight):
    """bench.py's serving shape (`pasco_amd.graph.serve.SceneServer`, default 3 in flight): worker threads, each bound to its
    own HIP stream, run different scenes at the same time through ONE net (shared weights / operand caches; per-stream
    workspaces, status words and query-side graphs).  Every scene's outputs must equal, bit for bit, what the same scene
    gives alone on the default stream - also after the server's own warm-up (allocator settling, block write test)."""
    from pasco_amd.graph import PascoNet
    from pasco_amd.graph.serve import SceneServer, vet_cached_blocks
    dev = torch.device("cuda", 0)
    torch.manual_seed(21)
    net = PascoNet(n_classes=20, n_infers=2, in_channels=16, f=32, num_queries=20, heavy_decoder=False).eval().to(dev)
    scenes = [make_scene(40 + i, n_infers=2, in_channels=16, grid=(96, 96, 16), occupancy=0.12).to(dev) for i in range(n_flight)]
    teachers = [TeacherKeep(sc, dev) for sc in scenes]

    def step(j):
        sc = scenes[j]
        x = net.prepare_input(sc.in_feats, sc.in_coords)
        ret = net(x, sc.global_min_Cs, sc.global_max_Cs, sc.min_Cs, sc.max_Cs, keep_override=teachers[j])
        conf, sem, panop = net.ensemble(ret, sc.Ts)
        return [p["voxel_logits"].F.clone() for p in ret["panop_predictions"]] + \
               [p["query_logits"].clone() for p in ret["panop_predictions"]] + [t.clone() for t in sem] + [t.clone() for t in conf]

    with torch.no_grad():
        ref = [step(j) for j in range(n_flight)]
    torch.cuda.synchronize()
    server = SceneServer(dev, step, in_flight=n_flight)
    info = server.warm(range(n_flight), max_rounds=3)
    vet = vet_cached_blocks(dev, [torch.cuda.current_stream(dev)] + server.streams, min_bytes=8 << 20)
    assert vet["quarantined"] == 0 or vet["replaced"] == vet["quarantined"]
    got = {}
    server.run([j for _ in range(4) for j in range(n_flight)], on_done=lambda j, out: got.__setitem__(j, out))
    assert info["in_flight_rounds"] >= 1 and sorted(got) == list(range(n_flight))
    for j in range(n_flight):
        assert len(got[j]) == len(ref[j])
        for a, b in zip(got[j], ref[j]):
            assert a.shape == b.shape and torch.equal(a, b)


def test_scene_server_close_restores_what_it_changed(hip):
    """`SceneServer` changes the interpreter's switch interval and keys workspaces, status pairs and query-side
    hipGraphs by its worker streams; `close()` puts the interval back and drops exactly those entries."""
    import sys
    from pasco_amd.graph import PascoNet
    from pasco_amd.graph.serve import SceneServer
    dev = torch.device("cuda", 0)
    torch.manual_seed(5)
    net = PascoNet(n_classes=20, n_infers=2, in_channels=16, f=16, num_queries=12, heavy_decoder=False).eval().to(dev)
    sc = make_scene(7, n_infers=2, in_channels=16, grid=(40, 40, 8), occupancy=0.12).to(dev)
    tk = TeacherKeep(sc, dev)

    def step(_):
        x = net.prepare_input(sc.in_feats, sc.in_coords)
        return net(x, sc.global_min_Cs, sc.global_max_Cs, sc.min_Cs, sc.max_Cs, keep_override=tk)

    before = sys.getswitchinterval()
    server = SceneServer(dev, step, in_flight=2, switch_interval_ms=0.5, allocator_rounding=None)
    assert abs(sys.getswitchinterval() - 0.5e-3) < 1e-9
    server.run([0, 1, 2, 3])
    handles = {int(s.cuda_stream) for s in server.streams}
    graphs = net.transformer_predictor.__dict__.get("_qgraphs", {})
    assert any(k[-1] in handles for k in graphs) or net.transformer_predictor.query_graph_state() != "graph"
    streams = list(server.streams)
    assert all("status" in hip.scratch.held(s) for s in streams), "every worker stream holds its status pair"
    for s in streams:
        with torch.cuda.stream(s):
            hip.status_ptr(dev)                           # the address is cached by stream handle
            hip.status_word(dev).fill_(1)                 # a flag nobody read
    torch.cuda.synchronize()
    server.close()
    assert sys.getswitchinterval() == before
    assert not any(k[-1] in handles for k in net.transformer_predictor.__dict__.get("_qgraphs", {}))
    assert all(hip.scratch.held(s) == set() for s in streams)
    keep = []                                             # held until the end, so that no new pair can land on a freed one's block
    for s in streams:
        with torch.cuda.stream(s):
            ptr = hip.status_ptr(dev)                     # not the cached address of the dropped pair: a fresh pair ...
            pair = hip.scratch.get("status", dev)
            keep.append(pair)
            assert pair.data_ptr() == ptr and pair.tolist() == [0, 0], "... whose words are 0"
            assert hip.status_word(dev).data_ptr() == ptr
        hip.release_stream(s)
    assert len({p.data_ptr() for p in keep}) == len(streams)
