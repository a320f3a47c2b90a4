"""The one ring of recycled pinned staging buffers behind every host<->device copy of the package's entry points.

What it encodes (NOTES.md, "HOST"): a copy from pageable memory makes the host wait until the stream has drained, so
every copy goes through pinned memory; allocating pinned memory synchronises the device, so the buffers are recycled;
a buffer is handed out again only after the copy that last used it has completed (one blocking event per slot, recorded
on -- and belonging to -- the slot's device); the host side is packed with `np.copyto`, a plain memcpy, because
`torch.stack` / `Tensor.copy_` on more than 32k elements fan out over an OpenMP team that burns a container's CPU quota.

`upload` and `readback` are the interface; callers never touch events or slots.  On a device that is not a GPU the ring
hands out plain memory and events that do nothing, so the same code runs (and is tested) without one.

A ring serves ONE issuing thread (the thread that enqueues the GPU work); loader threads never touch it.  No lock.
"""
import contextlib
import itertools
import math

import numpy as np
import torch


class _NoEvent:
    def record(self, stream=None):
        pass

    def synchronize(self):
        pass


def new_event(device):
    """The event that guards a slot of `device` (the one place events are made: tests substitute a recording fake)."""
    return torch.cuda.Event(blocking=True) if device.type == "cuda" else _NoEvent()     # blocking: waits sleep, not spin


def _spans(specs):
    """(start, end) byte offsets for a list of (shape, torch dtype): each starts at the next multiple of 256, which is
    aligned for every dtype on both sides of the copy."""
    spans, at = [], 0
    for shape, dtype in specs:
        spans.append((at, at + math.prod(shape) * dtype.itemsize))
        at = (spans[-1][1] + 255) & -256
    return spans


def _carve(flat, specs):
    return [flat[a:b].view(dtype).view(tuple(shape)) for (a, b), (shape, dtype) in zip(_spans(specs), specs)]


class _Slot:
    def __init__(self, device):
        self.device, self.buffer, self.event, self.generation = device, None, None, 0

    def views(self, specs):
        """Typed views of the buffer, one per (shape, torch dtype)."""
        return _carve(self.buffer, specs)

    def record(self):
        """Mark the slot busy until what the current stream of its device holds now has run."""
        self.event.record(torch.cuda.current_stream(self.device) if self.device.type == "cuda" else None)


class PinnedRing:
    """`slots` staging buffers per device, handed out round robin (see the module docstring for the contract)."""

    def __init__(self, slots):
        self.slots = slots
        self._rings = {}        # normalised device -> its slots, round robin

    def take(self, device, nbytes):
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:          # `cuda` and `cuda:<current>` are one ring
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._rings:
            self._rings[device] = itertools.cycle([_Slot(device) for _ in range(self.slots)])
        slot = next(self._rings[device])
        if slot.generation:
            slot.event.synchronize()        # the copy that last used this buffer has completed
        slot.generation += 1                # read-back handles of the previous use are stale from here on
        if slot.buffer is None or slot.buffer.numel() < nbytes:
            cap = max(4096, (nbytes + nbytes // 2 + 4095) & -4096)       # headroom: sizes that creep up do not reallocate
            with torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext():
                slot.buffer = torch.empty(cap, dtype=torch.uint8, pin_memory=device.type == "cuda")
                slot.event = slot.event or new_event(device)
        return slot


def upload(arrays, device, ring, stack=False):
    """Host arrays (numpy or CPU tensors, any dtypes and shapes) -> device tensors through one slot of `ring` and ONE
    asynchronous copy.  stack=True: equally shaped arrays -> one contiguous [len(arrays), ...] tensor."""
    srcs = [a.numpy() if torch.is_tensor(a) else np.asarray(a) for a in arrays]
    specs = [(s.shape, torch.from_numpy(np.empty(0, s.dtype)).dtype) for s in srcs]
    if stack:
        specs = [((len(srcs),) + specs[0][0], specs[0][1])]
    total = _spans(specs)[-1][1]
    slot = ring.take(device, total)
    views = slot.views(specs)
    for dst, src in zip(views[0].numpy() if stack else [v.numpy() for v in views], srcs):
        np.copyto(dst, src)
    host = slot.buffer[:total]
    dev = host.to(slot.device, non_blocking=True) if slot.device.type == "cuda" else host.clone()
    slot.record()
    out = _carve(dev, specs)
    return out[0] if stack else out


class ReadBack:
    """Device tensors on their way to a slot.  `wait()` -> their host views (valid until the ring has gone round), or None
    if the slot has been handed out again since (`stale`); `tensors` are the device tensors, kept alive."""

    def __init__(self, tensors, slot, views):
        self.tensors, self._slot, self._generation, self._views = tensors, slot, slot.generation, views

    @property
    def stale(self):
        return self._slot.generation != self._generation

    def wait(self):
        self._slot.event.synchronize()
        return None if self.stale else self._views


def readback(tensors, ring):
    """Device tensors (one device) -> `ReadBack`: one asynchronous copy each into one slot of `ring`, on the current
    stream of their device."""
    specs = [(t.shape, t.dtype) for t in tensors]
    slot = ring.take(tensors[0].device, _spans(specs)[-1][1])
    views = slot.views(specs)
    for v, t in zip(views, tensors):
        v.copy_(t, non_blocking=True)
    slot.record()
    return ReadBack(tensors, slot, views)
