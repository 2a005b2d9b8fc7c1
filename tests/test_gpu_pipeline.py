"""opticalflow_amd._pipeline on the device: capture_graph runs its function exactly once before the capture and `between` on both
sides of it; PinnedRing hands its slots out in turn, reuses them, reallocates one on a change of spec and lets a slot be rewritten
only after the upload marked behind it has completed."""
import pytest
import torch

from opticalflow_amd._pipeline import PinnedRing, capture_graph

pytestmark = pytest.mark.gpu

SPECS = (((2, 5, 7, 3), torch.uint8), ((2, 4), torch.float32))


def test_capture_graph_warms_up_once_and_captures_without_running(gpu_device):
    counter = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    inp = torch.tensor([1.0, 2.0, 3.0], device=gpu_device)
    out = torch.zeros(3, device=gpu_device)
    log = []

    def fn():
        log.append(("fn", torch.cuda.is_current_stream_capturing()))
        counter.add_(1)
        return torch.mul(inp, 2.0, out=out)

    def between():
        log.append(("between", torch.cuda.is_current_stream_capturing()))

    graph, result = capture_graph(fn, gpu_device, between=between)
    torch.cuda.synchronize(gpu_device)
    assert counter.item() == 1                                   # the warm-up ran, the capture executed nothing
    assert log == [("fn", False), ("between", False), ("fn", True), ("between", False)]
    assert result is out
    inp.copy_(torch.tensor([-4.0, 0.5, 7.0]))
    graph.replay()
    torch.cuda.synchronize(gpu_device)
    assert counter.item() == 2
    assert torch.equal(out, 2.0 * inp) and out.tolist() == [-8.0, 1.0, 14.0]


def test_capture_graph_without_between(gpu_device):
    counter = torch.zeros(1, dtype=torch.int64, device=gpu_device)
    graph, result = capture_graph(lambda: counter.add_(1), gpu_device)
    graph.replay()
    graph.replay()
    assert result is counter and counter.item() == 3


@pytest.mark.parametrize("slots,turns", [(2, "aba"), (1, "aaa")])
def test_ring_hands_its_slots_out_in_turn_and_reuses_them(gpu_device, slots, turns):
    ring = PinnedRing(slots=slots)
    assert ring.events == [None] * slots
    got = [ring.acquire(*SPECS) for _ in turns]
    for ts in got:
        assert [(tuple(t.shape), t.dtype) for t in ts] == [(s, d) for s, d in SPECS]
        assert all(t.is_pinned() for t in ts)
    ptrs = [tuple(t.data_ptr() for t in ts) for ts in got]
    assert ptrs[2] == ptrs[0] and (ptrs[1] == ptrs[0]) == (turns == "aaa")
    assert all(x is y for x, y in zip(got[0], got[2]))
    assert ring.events == [None] * slots                         # nothing was marked


def test_ring_reallocates_one_slot_on_a_change_of_spec(gpu_device):
    ring = PinnedRing(slots=2)
    a = ring.acquire(*SPECS)
    b = ring.acquire(*SPECS)
    b[0].fill_(9)
    b[1].fill_(2.5)
    keep = [t.data_ptr() for t in b]
    ring.mark()
    changed = (SPECS[0], ((3, 4), torch.float32))
    a2 = ring.acquire(*changed)                                  # slot a again, with another second spec
    assert [(tuple(t.shape), t.dtype) for t in a2] == [((2, 5, 7, 3), torch.uint8), ((3, 4), torch.float32)]
    assert all(t.is_pinned() for t in a2) and a2[1].data_ptr() != a[1].data_ptr()
    assert ring.events[0] is None and ring.events[1] is not None
    b2 = ring.acquire(*SPECS)                                    # slot b: the same tensors, untouched
    assert [t.data_ptr() for t in b2] == keep and all(x is y for x, y in zip(b, b2))
    assert bool((b2[0] == 9).all()) and bool((b2[1] == 2.5).all())


def test_ring_guards_a_slot_until_its_upload_is_done(gpu_device):
    """Six rounds of acquire, fill, upload, mark on a side stream.  The copies are 210 and 32 bytes, so the upload two rounds back has
    almost certainly finished by the time `acquire` returns whether or not it waited: this states the ring's contract and its data
    path, but it would probably not catch a ring that never synchronised."""
    ring = PinnedRing(slots=2)
    side = torch.cuda.Stream(device=gpu_device)
    rounds = []
    with torch.cuda.stream(side):
        for r in range(6):
            host = ring.acquire(*SPECS)
            if r >= 2:
                assert ring.events[r % 2].query() is True, r      # the upload two rounds back, which read this slot, is done
            for t in host:
                t.fill_(r)
            rounds.append(tuple(t.to(gpu_device, non_blocking=True) for t in host))
            ring.mark(side)
    assert all(e is not None for e in ring.events)
    torch.cuda.synchronize(gpu_device)
    for r, (u8, f32) in enumerate(rounds):
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (2, 5, 7, 3) and bool((u8 == r).all()), r
        assert f32.dtype == torch.float32 and tuple(f32.shape) == (2, 4) and bool((f32 == float(r)).all()), r
