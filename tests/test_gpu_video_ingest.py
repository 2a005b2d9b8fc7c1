"""pwc_video_ingest_u8 on the device (csrc/pwc_video.hip through opticalflow_amd.video.ingest_frames): bit-equal to the NumPy oracle
(tests/video_ingest_oracle.py, tied to the host helpers by tests/test_video_ingest_cpu.py) on the case table, with every byte value in
every channel of every case, both channel orders, a source and a destination batch stride, a source that starts on an odd address,
and inside a captured graph."""
import numpy as np
import pytest
import torch

import video_ingest_oracle as R
from opticalflow_amd import ops, video

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same(got: torch.Tensor, want: np.ndarray) -> bool:
    return tuple(got.shape) == want.shape and got.dtype == torch.float32 and np.array_equal(_bits(got.cpu().numpy()), _bits(want))


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("n,H,W", R.CASES)
def test_kernel_equals_the_oracle(gpu_device, n, H, W, bgr):
    for r, frames in enumerate(R.case_frames(n, H, W)):
        got = video.ingest_frames(torch.from_numpy(frames).to(gpu_device), bgr=bgr)
        assert _same(got, R.ingest(frames, bgr=bgr)), (n, H, W, bgr, r)


def test_one_frame_without_a_batch_dimension(gpu_device):
    frames = R.case_frames(1, 66, 130)[0]
    assert _same(video.ingest_frames(torch.from_numpy(frames[0]).to(gpu_device)), R.ingest(frames))


@pytest.mark.parametrize("bgr", [True, False])
def test_source_batch_stride_and_odd_addresses(gpu_device, bgr):
    """buf[:, 1] of a uint8 [n,2,H,W,3] buffer (frames 3 * 61 * 67 = 12261 bytes apart from their slots' starts: odd), and frames that
    start one, two and three bytes into an allocation: no alignment of the source may be assumed."""
    n, H, W = 3, 61, 67
    frames = R.case_frames(n, H, W)[0]
    want = R.ingest(frames, bgr=bgr)
    buf = torch.empty((n, 2, H, W, 3), dtype=torch.uint8, device=gpu_device)
    buf[:, 0] = torch.from_numpy(255 - frames).to(gpu_device)
    buf[:, 1] = torch.from_numpy(frames).to(gpu_device)
    src = buf[:, 1]
    assert not src.is_contiguous() and src.stride(0) == 2 * H * W * 3
    assert _same(video.ingest_frames(src, bgr=bgr), want)
    for off in (1, 2, 3):
        flat = torch.zeros(off + frames.size, dtype=torch.uint8, device=gpu_device)
        flat[off:] = torch.from_numpy(frames).to(gpu_device).reshape(-1)
        src = flat[off:].view(n, H, W, 3)
        assert src.data_ptr() % 4 == off
        assert _same(video.ingest_frames(src, bgr=bgr), want), off


def test_destination_batch_stride(gpu_device):
    n, H, W = 2, 100, 150
    frames = R.case_frames(n, H, W)[0]
    big = torch.full((n, 2, 3, 128, 192), -7.0, device=gpu_device)
    out = big[:, 1]
    assert out.stride(0) == 2 * 3 * 128 * 192
    got = video.ingest_frames(torch.from_numpy(frames).to(gpu_device), out=out)
    assert got is out and _same(out, R.ingest(frames))
    assert bool((big[:, 0] == -7.0).all())                      # the other slots are untouched


def test_captured_in_a_graph_and_replayed_on_changed_input(gpu_device):
    n, H, W = 2, 5, 7
    sets = R.case_frames(n, H, W)
    raw = torch.from_numpy(sets[0]).to(gpu_device)
    out = torch.zeros((n, 3, 64, 64), device=gpu_device)
    side = torch.cuda.Stream(device=gpu_device)
    side.wait_stream(torch.cuda.current_stream(gpu_device))
    with torch.cuda.stream(side):
        ops.video_ingest(raw, out=out, bgr=True)
    torch.cuda.current_stream(gpu_device).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.video_ingest(raw, out=out, bgr=True)
    for frames in (sets[1], sets[2]):
        raw.copy_(torch.from_numpy(frames).to(gpu_device))
        out.zero_()
        graph.replay()
        assert _same(out, R.ingest(frames))


def test_library_refuses_a_misaligned_destination(gpu_device):
    from opticalflow_amd import PwcHipError
    raw = torch.zeros((1, 5, 7, 3), dtype=torch.uint8, device=gpu_device)
    flat = torch.zeros(1 + 3 * 64 * 64, device=gpu_device)
    with pytest.raises(PwcHipError, match="16-byte aligned"):
        ops.video_ingest(raw, out=flat[1:].view(1, 3, 64, 64))
