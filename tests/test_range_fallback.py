"""Robustness of the split-precision path: an activation outside the f16 range must cost time, not the answer
(VERDICT r2 item 8).  `PascoNet.forward` redoes the step - input stage included - on the exact fp32 path when the device
status word reports bit 0; other status bits still raise; the status word is per stream."""
import pytest
import torch

from pasco_amd import settings
from pasco_amd.graph import PascoNet, fused
from pasco_amd.graph.synth import TeacherKeep, make_scene
from pasco_amd.me import backend
from pasco_amd.me.backend import F16RangeError, StatusError


def _net_scene(seed=3):
    torch.manual_seed(seed)
    net = PascoNet(n_classes=20, n_infers=2, in_channels=16, f=32, num_queries=12, heavy_decoder=False).eval()
    scene = make_scene(4, n_infers=2, in_channels=16, grid=(32, 32, 8), occupancy=0.15)
    return net, scene


def _run(net, scene, device, feats=None):
    sc = scene.to(device)
    tk = TeacherKeep(sc, torch.device(device))
    with torch.no_grad():
        x = net.prepare_input(feats if feats is not None else sc.in_feats, sc.in_coords)
        return net(x, sc.global_min_Cs, sc.global_max_Cs, sc.min_Cs, sc.max_Cs, keep_override=tk)


def _compare(got, ref, rtol, atol):
    for s in ref["sem_logits_at_scales"]:
        for a, b in zip(got["sem_logits_at_scales"][s], ref["sem_logits_at_scales"][s]):
            assert torch.equal(a.C.cpu(), b.C.cpu())
            assert torch.isfinite(a.F).all()
            assert torch.allclose(a.F.cpu(), b.F.cpu(), rtol=rtol, atol=atol), float((a.F.cpu() - b.F.cpu()).abs().max())


def test_forward_redoes_the_step_in_fp32_on_the_range_flag_cpu(oracle):
    """CPU tier (the oracle takes the split descriptors): inputs of magnitude 1e4 raise the flag in the point MLP's operand
    emission; the forward must come back with the exact path's numbers and count the fallback."""
    backend.register_checker_backend(oracle)
    oracle.status_word(torch.device("cpu")).zero_()
    old = fused.MIN_ROWS_LINEAR
    try:
        net, scene = _net_scene()
        big = [f * 1.0e4 for f in scene.in_feats]
        with fused.precision_override("f32"):
            ref = _run(net, scene, "cpu", feats=big)
        oracle.checker_split = True
        fused.MIN_ROWS_LINEAR = 1
        net.range_fallbacks = 0
        got = _run(net, scene, "cpu", feats=big)
        assert net.range_fallbacks == 1
        _compare(got, ref, 1e-4, 1e-3)
        # in range: no fallback, and the override did not leak into the process-wide setting
        got2 = _run(net, scene, "cpu")
        assert net.range_fallbacks == 1 and fused.conv_precision() == "f16x3"
        assert all(torch.isfinite(t.F).all() for t in got2["sem_logits_at_scales"][1])
    finally:
        oracle.checker_split = False
        fused.MIN_ROWS_LINEAR = old
        backend.register_checker_backend(None)


def test_status_error_types_and_all_bits_reported(oracle):
    dev = torch.device("cpu")
    w = oracle.status_word(dev)
    w.fill_(1)
    with pytest.raises(F16RangeError, match="f16 range"):
        oracle.check_status(dev)
    oracle.check_status(dev)                                     # cleared by the read
    w.fill_(1 | 2 | 4)
    with pytest.raises(StatusError) as ei:
        oracle.check_status(dev)
    assert not isinstance(ei.value, F16RangeError) and ei.value.bits == 7
    for piece in ("f16 range", "packable range", "per-axis table", "PASCO_RESIZE_ABSORB"):
        assert piece in str(ei.value)


@pytest.mark.gpu
def test_forward_redoes_the_step_in_fp32_on_the_range_flag_gpu(hip):
    net, scene = _net_scene()
    net = net.cuda()
    big = [f.cuda() * 1.0e4 for f in scene.in_feats]
    with fused.precision_override("f32"):
        ref = _run(net, scene, "cuda", feats=big)
    old = fused.MIN_ROWS_LINEAR
    fused.MIN_ROWS_LINEAR = 1
    try:
        net.range_fallbacks = 0
        got = _run(net, scene, "cuda", feats=big)
        assert net.range_fallbacks == 1
        _compare(got, ref, 1e-4, 1e-3)
    finally:
        fused.MIN_ROWS_LINEAR = old


@pytest.mark.gpu
def test_status_word_is_per_stream(hip):
    """A flag raised by a launch on stream A is reported on stream A only - neither lost to nor seen by a check made from
    another stream (scenes in flight on worker threads)."""
    dev = torch.device("cuda", 0)
    n, c = 256, 64
    x = torch.randn(n, c, device=dev)
    x[3, 5] = 1.0e5
    w = (torch.randn(c, c, device=dev) / 8)
    split = hip.split_weight_rows(w)
    torch.cuda.synchronize()
    sa, sb = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with torch.cuda.stream(sa):
        hip.check_status(dev)
        hip.conv_fwd(x, w, None, n, split=split)                 # raises bit 0 into stream A's word
    with torch.cuda.stream(sb):
        hip.check_status(dev)                                    # stream B: nothing
        hip.conv_fwd(torch.randn(n, c, device=dev), w, None, n, split=split)
        hip.check_status(dev)
    with torch.cuda.stream(sa):
        with pytest.raises(F16RangeError):
            hip.check_status(dev)
        hip.check_status(dev)
    torch.cuda.synchronize()


def _same(a, b):
    for s in b["sem_logits_at_scales"]:
        for x, y in zip(a["sem_logits_at_scales"][s], b["sem_logits_at_scales"][s]):
            assert torch.equal(x.C.cpu(), y.C.cpu()) and torch.equal(x.F.cpu(), y.F.cpu())
    for x, y in zip(a["panop_predictions"], b["panop_predictions"]):
        assert torch.equal(x["voxel_logits"].C.cpu(), y["voxel_logits"].C.cpu())
        assert torch.equal(x["voxel_logits"].F.cpu(), y["voxel_logits"].F.cpu())
        assert torch.equal(x["query_logits"].cpu(), y["query_logits"].cpu())


def test_optimistic_shortcuts_give_the_checked_paths_results_cpu(oracle_registered, monkeypatch):
    """`PascoNet.forward` takes its shortcuts without host reads (attention-mask block lookups, leading-rows selection, no
    all-zero bottleneck site) and validates them at the end of the step: whether they held (no fallback) or not (the step is
    redone on the checked paths), the results are those of `settings.optimistic` off (PASCO_OPTIMISTIC=0) bit for bit.  A forced violation must be seen."""
    dev = torch.device("cpu")
    oracle_registered.status_word(dev).zero_()
    oracle_registered.optimistic_word(dev).zero_()
    net, scene = _net_scene()
    with settings.override(optimistic=False):
        ref = _run(net, scene, "cpu")
    net.optimistic_fallbacks = 0
    got = _run(net, scene, "cpu")
    _same(got, ref)
    natural = net.optimistic_fallbacks
    # a violation nobody can miss: raise the flag from inside the step
    from pasco_amd.graph import decoder
    inner = decoder.DecoderGenerativeSepConvV2.predict_panop

    def poisoned(self, *a, **k):
        from pasco_amd.graph import fused as f
        w = f.optimistic_word(dev)
        if w is not None:
            w.fill_(1)
        return inner(self, *a, **k)

    monkeypatch.setattr(decoder.DecoderGenerativeSepConvV2, "predict_panop", poisoned)
    got2 = _run(net, scene, "cpu")
    assert net.optimistic_fallbacks == natural + 1
    _same(got2, ref)
    oracle_registered.check_status(dev)                           # nothing left behind
