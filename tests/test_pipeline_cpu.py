"""The multiple-of-64 geometry of opticalflow_amd._pipeline.pad64 and of the two callers that keep a result of their own
(video.raw_geometry, kitti.pad_to_64), against the expressions written out."""
import pytest
import torch
import torch.nn.functional as F

from opticalflow_amd import kitti, video
from opticalflow_amd._pipeline import pad64

SIZES = [(1, 1), (63, 64), (64, 65), (128, 128), (375, 1242), (436, 1024), (1080, 1920)]


@pytest.mark.parametrize("h,w", SIZES)
def test_pad64_equals_the_written_out_expressions(h, w):
    Hp, Wp, pad_h, pad_w = pad64(h, w)
    assert (Hp, Wp) == ((h + 63) // 64 * 64, (w + 63) // 64 * 64)
    assert (pad_h, pad_w) == ((64 - h % 64) % 64, (64 - w % 64) % 64)
    assert (Hp, Wp) == (h + pad_h, w + pad_w) and Hp % 64 == 0 and Wp % 64 == 0 and 0 <= pad_h < 64 and 0 <= pad_w < 64
    assert all(type(v) is int for v in (Hp, Wp, pad_h, pad_w))


def test_pad64_adds_nothing_at_exact_multiples():
    assert pad64(128, 128) == (128, 128, 0, 0)
    assert pad64(63, 64) == (64, 64, 1, 0)
    assert pad64(64, 65) == (64, 128, 0, 63)


@pytest.mark.parametrize("h,w", [(0, 64), (64, 0), (-1, 5), (5, -64), (0, 0)])
def test_pad64_refuses_non_positive_sizes(h, w):
    with pytest.raises(ValueError, match="positive"):
        pad64(h, w)


def test_raw_geometry_keeps_its_result_and_its_refusal():
    geo = video.raw_geometry(375, 1242)
    assert isinstance(geo, video.RawGeometry)
    assert (geo.height, geo.width) == (384, 1280) and geo.pads == (9, 38) and geo.crop == (87, 282)
    with pytest.raises(ValueError, match="leaves nothing"):
        video.raw_geometry(1, 1)
    with pytest.raises(ValueError, match="positive"):
        video.raw_geometry(0, 64)


def test_pad_to_64_keeps_its_signature_and_result():
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).reshape(2, 3, 5, 7)
    got, ph, pw = kitti.pad_to_64(x)
    assert (ph, pw) == (59, 57)
    assert torch.equal(got, F.pad(x, (0, 57, 0, 59), mode="replicate"))
    y = torch.zeros(1, 6, 64, 128)
    same, ph, pw = kitti.pad_to_64(y)
    assert same is y and (ph, pw) == (0, 0)


class _FakeStream:
    """What video._pushes needs of a stream, without a device."""

    def __init__(self, net, batch, frame_h, frame_w, **kw):
        self.frame_h, self.frame_w, self.pads, self.primed = frame_h, frame_w, (0, 0), None

    def prime(self, frame):
        self.primed = frame

    def push(self, frame):
        return torch.zeros(1, 2, self.frame_h // 4, self.frame_w // 4)


@pytest.mark.parametrize("ingest", ["host", "hip"])
def test_frame_loop_refuses_what_is_no_frame_and_a_size_change(monkeypatch, ingest):
    """Both ingest modes share one loop, so both refuse a frame that is not (H,W,3) before any stream is built, and a frame of
    another size even where it pads to the same multiple of 64 (65x70 after 64x70 both pad to 128x128)."""
    import numpy as np
    monkeypatch.setattr(video, "_HostStream", _FakeStream)
    monkeypatch.setattr(video, "RawFlowStream", _FakeStream)
    with pytest.raises(ValueError, match=r"expected an \(H,W,3\) BGR frame"):
        next(video.flow_video(None, [np.zeros((64, 70), np.uint8)], ingest=ingest))
    with pytest.raises(ValueError, match=r"expected an \(H,W,3\) BGR frame"):
        next(video.flow_video(None, [np.zeros((64, 70, 4), np.uint8)], ingest=ingest))
    frames = [np.zeros((65, 70, 3), np.uint8), np.zeros((65, 70, 3), np.uint8), np.zeros((64, 70, 3), np.uint8)]
    gen = video.flow_video(None, frames, ingest=ingest)
    assert next(gen).shape == (16, 17, 2)
    with pytest.raises(ValueError, match="frame size changed mid-stream"):
        next(gen)
    with pytest.raises(ValueError, match="ingest must be 'host' or 'hip'"):
        next(video.flow_video(None, frames, ingest="cpu"))
