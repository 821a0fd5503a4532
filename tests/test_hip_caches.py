"""The derived-tensor caches of the fused graph on the MI355X: the cases of tests/cache_cases.py on the device, where
the query side of the mask transformer is replayed from captured hipGraphs, entries are published to every stream and a
module can travel to the host and back.  After every event a warm net must give what a cold net gives; the graphs must still be
graphs and none may be left behind.  The CPU side is tests/test_caches_cpu.py."""
import pytest
import torch

from pasco_amd.graph import fused
from tests import cache_cases as cc

pytestmark = pytest.mark.gpu

_BENCHES = {}
# The comparison is bit for bit where the cold net repeats itself bit for bit; where it does not, the bound is 4 x the largest
# difference between two runs of the COLD net (two runs are a small sample), never a figure of the net under test.  It must stay
# far below what a stale entry costs (1.5e-1 at the least on the CPU tier, 8 - 10 for a stale convolution kernel).
REPEAT_CEILING = 1e-3


@pytest.fixture()
def small_rows(hip, monkeypatch):
    """The 1.2 k-voxel scene through the launches of a full-size one: the tall-operand threshold is the subject of other tests."""
    monkeypatch.setattr(fused, "MIN_ROWS_LINEAR", 1)
    yield hip
    fused.set_fusion(True)


def bench_of(heavy):
    if heavy not in _BENCHES:
        b = cc.Bench(heavy, "split", torch.device("cuda", 0))
        d = cc.repeatability(b)
        print(f"cold net against itself ({'heavy' if heavy else 'light'} decoder): max difference {d:.3e}")
        assert d <= REPEAT_CEILING, f"the cold net differs from itself by {d:.3e}: no bound separates a stale entry from that"
        b.bound = 4.0 * d
        _BENCHES[heavy] = b
    return _BENCHES[heavy]


def _passes(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad)


@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
def test_cold_net_repeats_itself(heavy, small_rows):
    b = bench_of(heavy)
    print(f"bound of the comparisons: {b.bound:.3e}")
    net = b.warm()
    assert net.transformer_predictor.query_graph_state() == "graph"


@pytest.mark.parametrize("event", ["load", "assign", "sgd", "inference_mode", "deepcopy"])
@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
def test_warm_net_equals_cold_net(heavy, event, small_rows):
    _passes(cc.EVENTS[event](bench_of(heavy)))


@pytest.mark.parametrize("event", sorted(cc.DEVICE_EVENTS))
@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
def test_device_events(heavy, event, small_rows):
    _passes(cc.DEVICE_EVENTS[event](bench_of(heavy)))
