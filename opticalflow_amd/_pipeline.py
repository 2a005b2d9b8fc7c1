"""What every frame front end needs on the host, once: the multiple-of-64 geometry, the capture recipe and the pinned
staging slots.  Nothing here copies a frame, owns device memory or knows what a frame is; the ordering rules a front end keeps
(which stream an upload goes on, who waits for whom) stay in that class's docstring."""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch


def pad64(h: int, w: int) -> Tuple[int, int, int, int]:
    """(Hp, Wp, pad_h, pad_w): h and w rounded up to multiples of 64 and what that adds at the bottom / right."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError("frame size must be positive, got %dx%d" % (h, w))
    hp, wp = (h + 63) // 64 * 64, (w + 63) // 64 * 64
    return hp, wp, hp - h, wp - w


def capture_graph(fn: Callable, device, between: Optional[Callable] = None):
    """(graph, result): `fn()` captured as one HIP graph after exactly one warm-up run of it (plans are built and first-launch
    attributes set there) on a side stream joined with the current stream in both directions.  `between()` runs after the warm-up
    and again after the capture: a stream whose step advances state restores it there.  `result` is what `fn` returned inside the
    capture; the capture itself executes nothing."""
    between = between or (lambda: None)
    cur, side = torch.cuda.current_stream(device), torch.cuda.Stream(device=device)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        fn()
    cur.wait_stream(side)
    between()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        result = fn()
    between()
    return graph, result


class PinnedRing:
    """`slots` sets of pinned host tensors handed out in turn, each guarded by one reused event: a slot is rewritten only after the
    upload that last read it has completed.

    ``acquire((shape, dtype), ...)`` takes the next slot; if it already holds tensors of exactly these specs it waits for the event
    `mark` recorded behind the slot's last upload, otherwise it allocates the slot afresh and forgets that event.  The caller fills
    the tensors, starts its own upload and calls ``mark(stream)`` (default: the current stream), which records the event of the slot
    handed out last and returns it (this upload's until the slot's next `mark`).  ``events``: per slot, None until first marked."""

    def __init__(self, slots: int = 2):
        self._slots, self.events = [None] * slots, [None] * slots
        self._next = self._last = 0

    def acquire(self, *specs) -> Tuple[torch.Tensor, ...]:
        k = self._last = self._next
        self._next = (k + 1) % len(self._slots)
        specs = [(tuple(s), d) for s, d in specs]
        held = self._slots[k]
        if held is not None and [(tuple(t.shape), t.dtype) for t in held] == specs:
            if self.events[k] is not None:
                self.events[k].synchronize()
        else:
            self._slots[k] = tuple(torch.empty(s, dtype=d).pin_memory() for s, d in specs)
            self.events[k] = None
        return self._slots[k]

    def mark(self, stream=None) -> torch.cuda.Event:
        k = self._last
        if self.events[k] is None:
            self.events[k] = torch.cuda.Event()
        self.events[k].record(stream if stream is not None else torch.cuda.current_stream())
        return self.events[k]
