"""Raw-frame ingest of the video tools (csrc/pwc_video.hip, opticalflow_amd.video.ingest_frames / RawFlowStream), what can be said
without a GPU: the NumPy oracle the GPU tests compare against equals the host helpers bit for bit; the division is not a
multiplication; the new entry point is declared, bound, built and exported and checks its arguments before touching memory; the
wrapper refuses what it cannot take before the library loads; the stream's pad / crop arithmetic is the reference's."""
import os
import re

import numpy as np
import pytest
import torch

import video_ingest_oracle as R
from opticalflow_amd import PwcHipError, _lib, ops, video
from opticalflow_amd.kitti import pad_to_64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOL = "pwc_video_ingest_u8"
PWC_EINVAL, PWC_EALIGN = -1, -3                 # include/pwc_hip.h


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("n,H,W", R.CASES)
def test_cases_hold_every_byte_in_every_channel(n, H, W):
    sets = R.case_frames(n, H, W)
    assert all(s.shape == (n, H, W, 3) and s.dtype == np.uint8 for s in sets)
    for c in range(3):
        assert len(np.unique(np.concatenate([s[..., c].ravel() for s in sets]))) == 256
    assert (sets[0][..., 0] != sets[0][..., 2]).all() and (sets[0][..., 0] != sets[0][..., 1]).all()


@pytest.mark.parametrize("n,H,W", R.CASES)
def test_oracle_equals_the_host_helpers(n, H, W):
    """frame_to_tensor + pad_to_64 per frame, bit for bit; without bgr the same on the frame whose channels are already reversed."""
    for frames in R.case_frames(n, H, W)[:4]:
        for bgr in (True, False):
            got = R.ingest(frames, bgr=bgr)
            assert got.shape == (n, 3, R.padded(H), R.padded(W)) and got.dtype == np.float32
            for i in range(n):
                f = frames[i] if bgr else np.ascontiguousarray(frames[i][:, :, ::-1])
                want, ph, pw = pad_to_64(video.frame_to_tensor(f).unsqueeze(0))
                assert (ph, pw) == (R.padded(H) - H, R.padded(W) - W)
                assert np.array_equal(_bits(got[i]), _bits(want[0].numpy())), (i, bgr)


def test_division_is_not_a_multiplication_by_the_reciprocal():
    b = np.arange(256, dtype=np.uint8)
    q = b.astype(np.float32) / 255.0
    assert q.dtype == np.float32
    assert np.array_equal(_bits(q), _bits((b.astype(np.float64) / 255.0).astype(np.float32)))      # the correctly rounded quotient
    m = b.astype(np.float32) * np.float32(1.0 / 255.0)
    assert int((_bits(q) != _bits(m)).sum()) == 126
    assert np.array_equal(_bits(R.ingest(b.reshape(1, 16, 16, 1).repeat(3, axis=3))[0, 0, :16, :16].ravel()), _bits(q))


def test_new_symbol_is_declared_bound_and_exported():
    header = open(os.path.join(REPO, "include", "pwc_hip.h")).read()
    lib = _lib.load()
    assert lib.pwc_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"^int %s\(([^;]*)\);" % NEW_SYMBOL, header, re.M | re.S)
    assert decl, "%s is not declared in include/pwc_hip.h" % NEW_SYMBOL
    assert NEW_SYMBOL in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NEW_SYMBOL][1]) == decl.group(1).count(",") + 1
    assert getattr(lib, NEW_SYMBOL).argtypes == _lib.SIGNATURES[NEW_SYMBOL][1]
    assert "pwc_video.hip" in open(os.path.join(REPO, "opticalflow_amd", "csrc", "Makefile")).read()


def test_library_checks_arguments_before_touching_memory():
    """The argument checks come before any use of the pointers, so they can be exercised with made-up addresses and no device."""
    lib = _lib.load()
    a = 0x10000
    good = dict(src=a + 1, dst=a, n=2, H=5, W=7, bgr=1, sb=105, db=3 * 64 * 64, stream=None)       # in the ABI's argument order
    call = lambda **k: lib.pwc_video_ingest_u8(*{**good, **k}.values())
    for bad in (dict(src=None), dict(dst=None), dict(n=0), dict(H=0), dict(W=0), dict(H=-3), dict(W=(1 << 20) + 1), dict(sb=104),
                dict(db=3 * 64 * 64 - 4), dict(db=0)):
        assert call(**bad) == PWC_EINVAL, bad
    for bad in (dict(dst=a + 4), dict(dst=a + 8), dict(db=3 * 64 * 64 + 2)):
        assert call(**bad) == PWC_EALIGN, bad


def test_wrapper_checks_arguments_before_the_library_loads(monkeypatch):
    def no_load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", no_load)
    u8 = torch.zeros((2, 5, 7, 3), dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8"):
        ops.video_ingest(u8.float())
    with pytest.raises(TypeError, match="tensor"):
        ops.video_ingest(u8.numpy())
    with pytest.raises(ValueError, match="4-D"):
        ops.video_ingest(u8[0])
    with pytest.raises(ValueError, match="3 interleaved channels"):
        ops.video_ingest(torch.zeros((2, 5, 7, 4), dtype=torch.uint8))
    with pytest.raises(ValueError, match="positive"):
        ops.video_ingest(torch.zeros((2, 0, 7, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match="out must be float32"):
        ops.video_ingest(u8, out=torch.zeros((2, 3, 64, 128)))                         # shape: Wp is 64
    with pytest.raises(ValueError, match="out must be float32"):
        ops.video_ingest(u8, out=torch.zeros((2, 3, 64, 64), dtype=torch.float64))     # dtype
    with pytest.raises(ValueError, match="out is on"):
        ops.video_ingest(u8, out=torch.zeros((2, 3, 64, 64), device="meta"))           # device
    with pytest.raises(PwcHipError, match="no CPU fallback"):
        ops.video_ingest(u8, out=torch.zeros((2, 3, 64, 64)))                          # host tensors: no fallback
    with pytest.raises(PwcHipError):
        video.ingest_frames(u8[0])                                                     # [H,W,3] is one frame


def test_raw_geometry_is_the_reference_pad_and_unpad():
    g = video.raw_geometry(120, 250)
    assert (g.height, g.width, g.pads, g.crop) == (128, 256, (8, 6), (24, 58))
    g = video.raw_geometry(100, 150)
    assert (g.height, g.width, g.pads, g.crop) == (128, 192, (28, 42), (4, 6))
    g = video.raw_geometry(1080, 1920)
    assert (g.height, g.width, g.pads, g.crop) == (1088, 1920, (8, 0), (264, 480))
    g = video.raw_geometry(384, 512)
    assert (g.height, g.width, g.pads, g.crop) == (384, 512, (0, 0), (96, 128))
    for H, W in ((120, 250), (100, 150), (118, 190), (720, 1280)):
        g = video.raw_geometry(H, W)
        t, ph, pw = pad_to_64(torch.zeros((1, 3, H, W)))                               # what flow_video's host path computes
        assert (g.height, g.width) == tuple(t.shape[2:]) and g.pads == (ph, pw)
        q = torch.zeros((1, 2, g.height // 4, g.width // 4))
        assert tuple(video._unpad(q, ph, pw).shape[2:]) == g.crop
    for H, W in ((1, 1), (64, 65), (65, 64), (0, 64), (64, -1)):                                 # the crop would be empty / no frame at all
        with pytest.raises(ValueError):
            video.raw_geometry(H, W)


def test_streams_refuse_bad_arguments_without_a_device():
    from opticalflow_amd import PWCDCNet
    net = PWCDCNet()
    with pytest.raises(PwcHipError):
        video.RawFlowStream(net, 1, 120, 250)                                          # the model is on the host
    with pytest.raises(ValueError, match="quiver"):
        video.RawFlowStream(net, 1, 120, 250, vanishing=dict(min_mag=1.0))
    with pytest.raises(ValueError, match="quiver"):
        video.RawFlowStream(net, 1, 120, 250, render=video.RenderSpec(color=True), vanishing={})
    frames = [np.zeros((100, 150, 3), np.uint8)] * 2
    for gen in (video.flow_video, video.flow_video_rendered):
        with pytest.raises(ValueError, match="ingest"):
            next(gen(net, frames, ingest="device"))
    with pytest.raises(ValueError, match="BGR frame"):
        next(video.flow_video(net, [np.zeros((100, 150), np.uint8)], ingest="hip"))
    with pytest.raises(PwcHipError):
        next(video.flow_video_vanishing(net, frames))


def test_strict_video_plan_shares_the_level2_statement():
    """One statement of the half-precision level 2: the stream's plan inherits it and only swaps the fp32 upper part."""
    from opticalflow_amd import engine, engine_strict as S
    assert S.PwcVideoPlanStrict._level2 is S.PwcPlanStrict._level2
    assert S.PwcPlanStrict.UPPER is engine.PwcPlan and S.PwcVideoPlanStrict.UPPER is engine.PwcVideoPlan
    assert "_level2" not in vars(S.PwcVideoPlanStrict) and "__init__" not in vars(S.PwcVideoPlanStrict)
