"""The derived-tensor caches of the fused graph on the CPU tier: after every way of changing the weights a warm
net must give, bit for bit, what a cold net gives.  The checker library takes split-operand descriptors and the tall-operand
threshold is 1, so the small scene runs the launches (and fills the caches) the device runs.  The cases are tests/cache_cases.py;
the GPU side is tests/test_hip_caches.py."""
import pytest
import torch

from pasco_amd.graph import fused
from pasco_amd.me import backend
from tests import cache_cases as cc

CPU = torch.device("cpu")
_BENCHES = {}


@pytest.fixture()
def split_checker(oracle, monkeypatch):
    backend.register_checker_backend(oracle)
    oracle.status_word(CPU).zero_()      # other tests raise the range flag on purpose
    oracle.checker_split = True
    monkeypatch.setattr(fused, "MIN_ROWS_LINEAR", 1)
    try:
        yield oracle
    finally:
        oracle.checker_split = False
        fused.set_fusion(True)
        backend.register_checker_backend(None)


def bench_of(heavy, route):
    """One scene and one set of cold references per (decoder, route), shared by the tests of this module."""
    key = (heavy, route)
    if key not in _BENCHES:
        _BENCHES[key] = cc.Bench(heavy, route, CPU)
    return _BENCHES[key]


def _passes(bad):
    assert not bad, f"{len(bad)} failures:\n" + "\n".join(bad)


BENCHES = [(h, r) for h in (False, True) for r in cc.ROUTES]
BENCH_IDS = [f"{'heavy' if h else 'light'}-{r}" for h, r in BENCHES]


@pytest.mark.parametrize("heavy, route", BENCHES, ids=BENCH_IDS)
def test_cold_net_repeats_itself(heavy, route, split_checker):
    """What makes the bit-for-bit comparison fair: two cold nets of one checkpoint, and a second run of one, differ by 0.0."""
    assert cc.repeatability(bench_of(heavy, route)) == 0.0


@pytest.mark.parametrize("event", sorted(cc.EVENTS))
@pytest.mark.parametrize("heavy, route", BENCHES, ids=BENCH_IDS)
def test_warm_net_equals_cold_net(heavy, route, event, split_checker):
    _passes(cc.EVENTS[event](bench_of(heavy, route)))


@pytest.mark.parametrize("heavy", [False, True], ids=["light", "heavy"])
def test_route_round_trips(heavy, split_checker):
    _passes(cc.event_round_trips(bench_of(heavy, "split")))


@pytest.mark.parametrize("route", cc.ROUTES)
def test_one_tensor_at_a_time(route, split_checker):
    """One instance per (owner class, tensor name) pair on the light decoder (the sweep is two forwards per change; the heavy
    decoder holds the same classes), on every route: each route fills entries of its own (unfused: pasco_amd.me's)."""
    bad, pairs, more, exempt = cc.event_one_tensor_at_a_time(bench_of(False, route))
    print(f"single-tensor sweep ({route}): {pairs} (class, tensor) pairs covered, {exempt} of them exempt; {more} more tensors "
          "that feed an entry of a sibling module")
    assert pairs - exempt >= 20
    _passes(bad)
