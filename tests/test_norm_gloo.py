"""`MinkowskiSyncBatchNorm` across ranks, on the CPU: spawned gloo processes (the pattern of tests/test_dist_gloo.py) run a small
conv -> BatchNorm -> ReLU stack that went through `convert_sync_batchnorm`, each rank on rows of its own, and hold outputs,
input gradients, parameter gradients and running statistics to the fp64 twin over ALL ranks' rows (tests/norm_ref64.py).  With
statistics taken per rank - what the module did before it synchronised - the two-rank test fails."""
import os
import socket

import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

CIN, C = 5, 12


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rows(rank):
    """Rank r has 40 + 25 r rows: features, distinct coordinates, output gradients."""
    n = 40 + 25 * rank
    g = torch.Generator().manual_seed(500 + rank)
    feats = torch.randn(n, CIN, generator=g) * 1.3 + 0.37
    dy = torch.randn(n, C, generator=g) * 0.71 + 0.05
    idx = torch.arange(n, dtype=torch.int32)
    coords = torch.stack([torch.zeros_like(idx), idx % 7, (idx // 7) % 7, idx // 49], 1).contiguous()
    return feats, coords, dy


def _net():
    import pasco_amd.me as ME
    torch.manual_seed(21)
    net = nn.Sequential(ME.MinkowskiConvolution(CIN, C, kernel_size=1, bias=True, dimension=3), ME.MinkowskiBatchNorm(C),
                        ME.MinkowskiReLU()).train()
    with torch.no_grad():
        net[1].bn.weight.uniform_(0.6, 1.7), net[1].bn.bias.uniform_(-0.4, 0.4)
        net[1].bn.running_mean.uniform_(-0.3, 0.3), net[1].bn.running_var.uniform_(0.5, 1.5)
    return net


def _run_net(net, rank):
    import pasco_amd.me as ME
    feats, coords, dy = _rows(rank)
    feats.requires_grad_(True)
    out = net(ME.SparseTensor(feats, coords))
    out.F.backward(dy)
    bn = net[1].bn
    return {"y": out.F.detach(), "dx": feats.grad, "dw": bn.weight.grad, "db": bn.bias.grad, "dk": net[0].kernel.grad,
            "running_mean": bn.running_mean.clone(), "running_var": bn.running_var.clone(),
            "counter": int(bn.num_batches_tracked), "grad_fn": type(out.F.grad_fn).__name__}


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["OMP_NUM_THREADS"] = "2"
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import pasco_amd.me as ME
        from pasco_amd.me import backend
        from tests.conftest import load_oracle
        backend.register_checker_backend(load_oracle())
        plain = _run_net(_net(), rank)                                                    # today's MinkowskiBatchNorm
        sync = _run_net(ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_net()), rank)
        again = _run_net(ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(_net()), rank)
        q.put((rank, _pack(plain), _pack(sync), _pack(again)))     # plain arrays: nothing shared with a process that ends
    finally:
        dist.destroy_process_group()


def _pack(d):
    return {k: v.detach().numpy().copy() if isinstance(v, torch.Tensor) else v for k, v in d.items()}


def _unpack(d):
    return {k: v if isinstance(v, (int, str)) else torch.from_numpy(v) for k, v in d.items()}


def _spawn(world):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [(r, _unpack(a), _unpack(b), _unpack(c)) for r, a, b, c in res]


def _twin(world, dtype):
    """conv (k = 1: a matrix product) -> batch_norm over the rows of all ranks -> ReLU, in plain torch."""
    import torch.nn.functional as F
    net = _net()
    p = {k: v.detach().to(dtype).requires_grad_(True) for k, v in net.named_parameters()}
    rows = [_rows(r) for r in range(world)]
    xs = [f.to(dtype).requires_grad_(True) for f, _, _ in rows]
    rm, rv = net[1].bn.running_mean.to(dtype).clone(), net[1].bn.running_var.to(dtype).clone()
    h = torch.cat([x @ p["0.kernel"] + p["0.bias"] for x in xs])
    y = torch.relu(F.batch_norm(h, rm, rv, p["1.bn.weight"], p["1.bn.bias"], True, 0.1, 1e-5))
    y.backward(torch.cat([d for _, _, d in rows]).to(dtype))
    cuts = [0]
    for f, _, _ in rows:
        cuts.append(cuts[-1] + f.shape[0])
    return {"y": [y.detach()[a:z] for a, z in zip(cuts[:-1], cuts[1:])], "dx": [x.grad for x in xs], "dw": p["1.bn.weight"].grad,
            "db": p["1.bn.bias"].grad, "dk": p["0.kernel"].grad, "running_mean": rm, "running_var": rv}


def test_two_ranks_normalise_over_both_ranks_rows():
    from tests.norm_ref64 import NORM_M
    world = 2
    res = _spawn(world)
    v32, v64 = _twin(world, torch.float32), _twin(world, torch.float64)
    worst = {}

    def hold(name, got, k32, k64):
        e, e32 = float((got.double() - k64).abs().max()), float((k32.double() - k64).abs().max())
        worst[name] = max(worst.get(name, 0.0), e / e32)

    for rank, _, sync, again in res:
        assert sync["grad_fn"] == "ReluBackward0" and sync["counter"] == 1
        hold("y", sync["y"], v32["y"][rank], v64["y"][rank])
        hold("dx", sync["dx"], v32["dx"][rank], v64["dx"][rank])
        hold("running_mean", sync["running_mean"], v32["running_mean"], v64["running_mean"])
        hold("running_var", sync["running_var"], v32["running_var"], v64["running_var"])
        for k in ("y", "dx", "dw", "db", "dk", "running_mean", "running_var"):
            assert torch.equal(sync[k], again[k]), f"rank {rank}: {k} differs between two runs"
    # parameter gradients are the LOCAL sums (a data-parallel wrapper adds them): their sum over the ranks is the twin's
    for k in ("dw", "db", "dk"):
        hold(k, sum(r[2][k].double() for r in res), v32[k], v64[k])
    assert torch.equal(res[0][2]["running_mean"], res[1][2]["running_mean"]), "every rank holds the same statistics"
    assert torch.equal(res[0][2]["running_var"], res[1][2]["running_var"])
    print("[norm] two gloo ranks: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v <= NORM_M}
    assert not bad, f"ratio over NORM_M = {NORM_M}: {bad}"
    # and the statistics really are those of both ranks: a rank normalising alone is far outside the bound
    alone = float((res[0][1]["y"].double() - v64["y"][0]).abs().max())
    assert alone > 1e3 * float((res[0][2]["y"].double() - v64["y"][0]).abs().max())


def test_one_rank_is_todays_batch_norm():
    """World size 1: torch.nn.SyncBatchNorm's condition does not hold, the converted stack is MinkowskiBatchNorm bit for bit."""
    (_, plain, sync, _), = _spawn(1)
    for k in ("y", "dx", "dw", "db", "dk", "running_mean", "running_var"):
        assert torch.equal(plain[k], sync[k]), k
    assert plain["counter"] == sync["counter"] == 1
