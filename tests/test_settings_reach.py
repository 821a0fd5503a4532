"""Every switch of `pasco_amd.settings` that no numeric test flips is at least REACHABLE: with the field on the branch it
guards is taken, with it off it is not - shown by counting calls of the function behind the branch (as test_attn_feat_cpu.py
counts `attn_cross_feat`), on the tiny net of test_range_fallback.py.  No numbers are compared: the forms have their
numeric tests where they differ.  CPU legs on the oracle wherever the branch is live there; `-m gpu` where it needs the GPU."""
import os

import pytest
import torch

from pasco_amd import settings
from pasco_amd.graph import dist as dist_mod
from pasco_amd.graph import fused
from pasco_amd.me.core import CoordinateManager
from tests.test_range_fallback import _net_scene, _run


def _count(monkeypatch, owner, name, returns=None):
    """Replace `owner.name` by a counting wrapper (or, with `returns`, a counting stub) -> the list of its calls' arguments."""
    inner, calls = getattr(owner, name), []

    def spy(*a, **kw):
        calls.append((a, kw))
        return returns if returns is not None else inner(*a, **kw)

    monkeypatch.setattr(owner, name, spy)
    return calls


@pytest.fixture(scope="module")
def tiny():
    return _net_scene()


# ---- CPU: the oracle serves the branch -----------------------------------------------------------------------------------------
def test_keep_fused_guards_the_keep_mask_kernel(oracle_registered, tiny, monkeypatch):
    calls = _count(monkeypatch, oracle_registered, "keep_mask")
    _run(*tiny, "cpu")
    assert len(calls) > 0
    del calls[:]
    with settings.override(keep_fused=False):
        _run(*tiny, "cpu")
    assert len(calls) == 0


def test_input_fused_guards_the_pooled_merge(oracle_registered, tiny, monkeypatch):
    net, scene = tiny
    calls = _count(monkeypatch, oracle_registered, "pooled_merge")
    with torch.no_grad():
        net.prepare_input(scene.in_feats, scene.in_coords)
        assert len(calls) == 1
        with settings.override(input_fused=False):
            net.prepare_input(scene.in_feats, scene.in_coords)
    assert len(calls) == 1


def test_panoptic_kernel_guards_the_row_kernels(oracle_registered, monkeypatch):
    from pasco_amd.graph import panoptic as P
    from tests.test_panoptic_rows import THINGS, make_case
    import pasco_amd.me as ME
    coords, masks, qp, extent = make_case(seed=3, n=200, q=6)
    kw = dict(overlap_threshold=0.4, object_mask_threshold=0.7, thing_ids=THINGS, scene_size=extent,
              min_C=torch.zeros(3, dtype=torch.int32), input_query_logit=False, input_voxel_logit=False)
    calls = _count(monkeypatch, oracle_registered, "panoptic_rows")
    P.panoptic_inference(ME.SparseTensor(masks, coords), qp, **kw)
    assert len(calls) == 1
    with settings.override(panoptic_kernel=False):
        P.panoptic_inference(ME.SparseTensor(masks, coords), qp, **kw)
    assert len(calls) == 1


def test_bench_pin_off_returns_before_the_affinity_call(monkeypatch):
    pinned = _count(monkeypatch, os, "sched_setaffinity", returns=())
    chosen = _count(monkeypatch, dist_mod, "rank_cpu_set", returns=[0])
    with settings.override(bench_pin=False):
        assert dist_mod.pin_rank(0, 1) == []
    assert pinned == [] and chosen == []


def test_bench_pin_on_goes_past_the_switch(monkeypatch):
    """With the field on `pin_rank` chooses the rank's CPUs (`rank_cpu_set`: stubbed, so nothing of /sys is read) and applies
    them (`os.sched_setaffinity`: stubbed, the test process keeps its affinity)."""
    pinned = _count(monkeypatch, os, "sched_setaffinity", returns=())
    chosen = _count(monkeypatch, dist_mod, "rank_cpu_set", returns=[0])
    assert settings.current().bench_pin is True
    assert dist_mod.pin_rank(0, 1) == [0]
    assert [a for a, _ in chosen] == [(0, 1, None)] and [a for a, _ in pinned] == [(0, [0])]


def test_c4_exchange_f16_halves_the_mask_logits(oracle_registered, monkeypatch):
    """`subnet_parallel_forward` on a world-1 gloo group: the mask logits handed to the exchange are f16 under
    c4_exchange="f16" and fp32 otherwise."""
    import torch.distributed as dist
    from tests.test_dist_gloo import _free_port
    net, scene = _net_scene()
    sent = _count(monkeypatch, dist_mod, "packed_allgather")
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        from pasco_amd.graph.synth import TeacherKeep
        tk = TeacherKeep(scene, torch.device("cpu"))
        with torch.no_grad():
            x = net.prepare_input(scene.in_feats, scene.in_coords)
            args = (net, x, scene.global_min_Cs, scene.global_max_Cs, scene.min_Cs, scene.max_Cs)
            got = dist_mod.subnet_parallel_forward(*args, keep_override=tk)
            assert got["exchange"]["payload"] == "f32" and {a[0][0].dtype for a, _ in sent} == {torch.float32}
            del sent[:]
            with settings.override(c4_exchange="f16"):
                got = dist_mod.subnet_parallel_forward(*args, keep_override=tk)
            assert got["exchange"]["payload"] == "f16" and {a[0][0].dtype for a, _ in sent} == {torch.float16}
            assert all(p["voxel_logits"].F.dtype == torch.float32 for p in got["panop_predictions"])
    finally:
        dist.destroy_process_group()


# ---- GPU: the branch needs device_type == "cuda" -------------------------------------------------------------------------------
@pytest.fixture()
def tiny_cuda(hip, monkeypatch):
    """The tiny net on the GPU with the tall-operand thresholds lowered (performance heuristics): its few thousand rows take the
    routes the benchmark's layers take."""
    monkeypatch.setattr(fused, "MIN_ROWS_LINEAR", 1)
    monkeypatch.setattr(fused, "MIN_ROWS_WINDOWS", 1)
    net, scene = _net_scene()
    return net.cuda(), scene


@pytest.mark.gpu
def test_conv_rl_guards_the_row_lists(tiny_cuda, monkeypatch):
    calls = _count(monkeypatch, CoordinateManager, "kernel_rowlist")
    _run(*tiny_cuda, "cuda")
    assert len(calls) > 0
    del calls[:]
    with settings.override(conv_rl=False):
        _run(*tiny_cuda, "cuda")
    assert len(calls) == 0


@pytest.mark.gpu
def test_conv_win_wide_extends_the_window_tables(hip, tiny_cuda, monkeypatch):
    """Off: only convolutions with 33 .. 64 output channels are given window tables; on: the others too."""
    calls = _count(monkeypatch, hip, "conv_fwd")
    wide = lambda: [a[1].shape[-1] for a, kw in calls if kw.get("win") is not None and not 33 <= a[1].shape[-1] <= 64]
    _run(*tiny_cuda, "cuda")
    assert any(kw.get("win") is not None for _, kw in calls) and wide() == []
    del calls[:]
    with settings.override(conv_win_wide=True):
        _run(*tiny_cuda, "cuda")
    assert len(wide()) > 0


@pytest.mark.gpu
def test_query_graph_guards_the_capture(tiny_cuda, monkeypatch):
    from pasco_amd.graph.transformer import TransformerPredictorV2
    net, scene = tiny_cuda
    captures = _count(monkeypatch, TransformerPredictorV2, "_capture_query_step")
    with settings.override(query_graph=False):
        _run(net, scene, "cuda")
        assert len(captures) == 0 and net.transformer_predictor.query_graph_state() == "eager"
    _run(net, scene, "cuda")
    assert len(captures) > 0 and net.transformer_predictor.query_graph_state() == "graph"
