"""`pasco_amd._clib.StreamScratch`, the per-stream scratch table of a backend, off the GPU: every entry is keyed (name, cpu, 0).
The same table on side streams of the device is held to its contract in tests/test_hip_streams.py."""
import torch

from pasco_amd import _clib
from pasco_amd._clib import StreamScratch

CPU = torch.device("cpu")


def test_key_off_the_device_is_handle_zero():
    assert StreamScratch.key(CPU) == (CPU, 0)


def test_bytes_keeps_the_floor_and_grows_by_replacement(monkeypatch):
    s = StreamScratch()
    a = s.bytes("ws", CPU, 10, floor=256)
    assert a.dtype == torch.uint8 and a.numel() == 256, "a new buffer has max(need, floor) bytes"
    assert s.bytes("ws", CPU, 256, floor=256) is a and s.bytes("ws", CPU, 1, floor=256) is a, "large enough: reused"
    assert s.bytes("bare", CPU, 10).numel() == 10 and s.bytes("bare", CPU, 0).numel() == 10, "no floor: exactly the need"
    assert s.bytes("four", CPU, 0, floor=4).numel() == 4
    seen = []
    real = torch.empty

    def empty(*args, **kw):
        seen.append(s.get("ws", CPU))             # what the table holds when the larger buffer is allocated
        return real(*args, **kw)

    monkeypatch.setattr(_clib.torch, "empty", empty)
    b = s.bytes("ws", CPU, 257, floor=256)
    monkeypatch.undo()
    assert seen == [None], "the smaller buffer had left the table before the larger one was made"
    assert b.numel() == 257 and s.get("ws", CPU) is b and s.held() == {"ws", "bare", "four"}


def test_bytes_lets_go_of_the_smaller_buffer_itself():
    """Nothing but the caller's own reference keeps a replaced buffer alive."""
    import weakref
    s = StreamScratch()
    old = weakref.ref(s.bytes("ws", CPU, 8).untyped_storage())
    s.bytes("ws", CPU, 16)
    assert old() is None


def test_words_are_zeroed_once():
    s = StreamScratch()
    w = s.words("status", CPU, 2)
    assert w.dtype == torch.int32 and w.tolist() == [0, 0]
    w[1] = 7
    again = s.words("status", CPU, 2)
    assert again is w and again.tolist() == [0, 7], "the second call neither makes a new pair nor clears the old one"
    assert s.words("keep_any", CPU, 1).tolist() == [0] and s.words("status", "cpu", 2) is w


def test_words_made_in_inference_mode_can_be_written_outside_it():
    s = StreamScratch()
    with torch.inference_mode():
        w = s.words("status", CPU, 2)
    assert not w.is_inference()
    w.zero_()
    w[0] = 3
    assert w.tolist() == [3, 0]


def test_release_counts_the_names_held():
    s = StreamScratch()
    s.bytes("ws", CPU, 8), s.bytes("attn", CPU, 8), s.words("status", CPU, 2)
    ptr = s.status_ptr(CPU)                       # the address cache is not part of the count
    assert ptr == s.get("status", CPU).data_ptr()
    assert s.held() == s.held(0) == {"ws", "attn", "status"} and s.held(77) == set()
    assert s.release(77) == 0 and s.held() == {"ws", "attn", "status"}
    assert s.release(0) == 3 and s.held() == set() and s.release(0) == 0


def test_drop_forgets_one_name():
    s = StreamScratch()
    s.bytes("semloss", CPU, 8), s.bytes("ws", CPU, 8)
    assert s.drop("semloss") == 1 and s.held() == {"ws"} and s.drop("semloss") == 0
    assert s.drop("ws", CPU) == 1 and s.get("ws", CPU) is None


def test_release_leaves_another_backend_alone(oracle):
    from tests.conftest import load_oracle
    other = load_oracle()
    assert other.scratch is not oracle.scratch
    oracle.workspace(10, CPU), other.workspace(10, CPU)
    oracle.status_word(CPU), other.status_word(CPU).fill_(1)
    held = other.scratch.held()
    assert oracle.release_stream(0) >= 2 and oracle.scratch.held() == set()
    assert other.scratch.held() == held == {"ws", "status"} and other.status_word(CPU).tolist() == [1]


def test_status_ptr_after_release_is_rebuilt_and_reads_zero(oracle):
    oracle.release_stream(0)
    first = oracle.status_ptr(CPU)
    keep = oracle.scratch.get("status", CPU)      # held, so that the next pair cannot land on this one's memory
    assert keep.data_ptr() == first and oracle.status_ptr(CPU) == first
    oracle.status_word(CPU).fill_(1)
    oracle.optimistic_word(CPU).fill_(1)
    assert oracle.release_stream(0) == 1
    second = oracle.status_ptr(CPU)
    assert second != first, "the cached address went with the pair"
    assert oracle.scratch.get("status", CPU).data_ptr() == second and oracle.scratch.get("status", CPU).tolist() == [0, 0]
    oracle.check_status(CPU)                      # nothing raised: the unread flag went with the stream


def test_pinned_status_overrides_the_table(oracle):
    oracle.release_stream(0)
    with oracle.pin_status(CPU):
        pinned = oracle.status_ptr(CPU)
        oracle.release_stream(0)                  # the stream's pair goes, the pin stays what this thread reports into
        assert oracle.status_ptr(CPU) == pinned and oracle.status_word(CPU).data_ptr() == pinned
