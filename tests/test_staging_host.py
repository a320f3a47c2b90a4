"""The pinned staging ring (patch2pix_amd/staging.py) in its CPU mode: slot order and waiting, buffer growth, typed views,
generations of read-back handles, the stacked upload.  Events are recording fakes substituted through `staging.new_event`."""
import numpy as np
import pytest
import torch

from patch2pix_amd import staging

CPU = torch.device("cpu")


class _FakeEvent:
    def __init__(self, log):
        self.log, self.recorded = log, None

    def record(self, stream=None):
        self.recorded = sum(1 for what, _ in self.log if what == "record")          # number of this record, from 0
        self.log.append(("record", self.recorded))

    def synchronize(self):
        self.log.append(("synchronize", self.recorded))


@pytest.fixture
def log(monkeypatch):
    entries = []
    monkeypatch.setattr(staging, "new_event", lambda device: _FakeEvent(entries))
    return entries


def test_slot_order_and_waiting(log):
    slots = 4
    ring = staging.PinnedRing(slots)
    taken = []
    for k in range(slots + 3):
        before = len(log)
        slot = ring.take(CPU, 100)
        waited = [n for what, n in log[before:] if what == "synchronize"]
        # take k + slots waits for exactly the record of take k: nothing earlier is due, nothing younger may be waited for
        assert waited == ([k - slots] if k >= slots else [])
        taken.append(slot)
        slot.record()
        assert log[-1] == ("record", k)
    assert all(taken[k] is taken[k - slots] for k in range(slots, slots + 3))
    assert len({id(s) for s in taken}) == slots


def test_growth(log):
    ring = staging.PinnedRing(1)
    slot = ring.take(CPU, 1000)
    assert slot.buffer.dtype == torch.uint8 and slot.buffer.numel() >= 4096        # never below 4 KiB
    caps, ptr = [slot.buffer.numel()], slot.buffer.data_ptr()
    for n in (4096, 10, 0, caps[0]):                                               # no larger than the capacity: same storage
        slot = ring.take(CPU, n)
        assert slot.buffer.data_ptr() == ptr
        caps.append(slot.buffer.numel())
    for n in (caps[0] + 1, 100, 70000, 5000, 1 << 20, 3):
        before = slot.buffer.numel()
        slot = ring.take(CPU, n)
        cap = slot.buffer.numel()
        caps.append(cap)
        assert cap >= n
        if n > before:                                                             # x1.5, rounded up to 4 KiB
            assert slot.buffer.data_ptr() != ptr and cap == -(-(n + n // 2) // 4096) * 4096
        else:
            assert slot.buffer.data_ptr() == ptr and cap == before
        ptr = slot.buffer.data_ptr()
    assert caps == sorted(caps)                                                    # never shrinks


SPECS = [((1001,), torch.uint8), ((7, 4), torch.int64), ((7,), torch.float32), ((3, 4), torch.float64)]


def test_views(log):
    ring = staging.PinnedRing(2)
    slot = ring.take(CPU, 4096)
    views = slot.views(SPECS)
    base, spans = slot.buffer.data_ptr(), []
    for v, (shape, dtype) in zip(views, SPECS):
        assert v.dtype == dtype and tuple(v.shape) == shape and v.is_contiguous()
        offset = v.data_ptr() - base
        assert offset % 256 == 0 and 0 <= offset and offset + v.numel() * v.element_size() <= slot.buffer.numel()
        spans.append((offset, offset + v.numel() * v.element_size()))
    assert all(a_end <= b_start for (_, a_end), (b_start, _) in zip(spans, spans[1:]))      # disjoint
    # values written through one view do not disturb the others
    g = torch.Generator().manual_seed(3)
    want = [torch.randint(0, 200, shape, generator=g).to(dtype) for shape, dtype in SPECS]
    for v, w in zip(views, want):
        v.copy_(w)
    assert all(torch.equal(v, w) for v, w in zip(views, want))
    # and the upload helper carries mixed dtypes and sizes (numpy arrays and tensors) through one slot unchanged
    sources = [want[0].numpy(), want[1], want[2].numpy(), want[3]]
    got = staging.upload(sources, CPU, ring)
    assert [(tuple(t.shape), t.dtype) for t in got] == SPECS
    assert all(torch.equal(t, w) for t, w in zip(got, want))
    staging.upload([np.zeros(s, dtype=w.numpy().dtype) for (s, _), w in zip(SPECS, want)], CPU, ring)       # the other slot
    staging.upload([np.zeros(s, dtype=w.numpy().dtype) for (s, _), w in zip(SPECS, want)], CPU, ring)       # the same slot
    assert all(torch.equal(t, w) for t, w in zip(got, want))                       # a copy, not a view of the slot


def test_generations(log):
    slots = 3
    ring = staging.PinnedRing(slots)
    sources = [[torch.full((5, 9), float(k)) + torch.rand(5, 9), torch.arange(k, k + 6)] for k in range(slots + 1)]
    first = staging.readback(sources[0], ring)
    second = staging.readback(sources[1], ring)
    for k in range(2, slots + 1):
        assert not first.stale
        staging.readback(sources[k], ring)
    # `first` was taken `slots` stagings ago: its slot has been handed out again
    assert first.stale and first.wait() is None
    # `second` was taken `slots - 1` stagings ago: its data are still there
    assert not second.stale
    before = len(log)
    host = second.wait()
    assert log[before:] == [("synchronize", 1)]                                    # the event of its own record
    assert all(torch.equal(h, s) and h.dtype == s.dtype for h, s in zip(host, sources[1]))
    assert all(t is s for t, s in zip(second.tensors, sources[1]))                 # the device tensors are kept alive


def test_stacked_upload(log):
    ring = staging.PinnedRing(2)
    rng = np.random.default_rng(0)
    images = [rng.integers(0, 256, (5, 7, 3), dtype=np.uint8) for _ in range(3)]
    got = staging.upload([images[0], torch.from_numpy(images[1]), images[2]], CPU, ring, stack=True)
    assert tuple(got.shape) == (3, 5, 7, 3) and got.dtype == torch.uint8 and got.is_contiguous()
    assert np.array_equal(got.numpy(), np.stack(images))
    assert [what for what, _ in log] == ["record"]                                 # one slot, one recorded copy
