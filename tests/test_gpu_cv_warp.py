"""cv2.warpPerspective-exact warp on the device (csrc/pwc_cv_warp.hip, opticalflow_amd/cv_warp.py) against the NumPy oracle
(tests/cv_warp_oracle.py, held to a scalar loop and hand-worked vectors by tests/test_cv_warp_cpu.py), bit for bit: the coordinates
are a fixed sequence of float64 products, sums and one division that the build keeps unfused, the pixel is integer arithmetic.  Then
the two captured drivers, TopviewInfer and TopviewStream, against the oracle's warp in front of CvGraphedInfer(mode="topview").  cv2
parity is unpinned."""
import functools

import numpy as np
import pytest
import torch

import cv_resize_oracle as RZ
import cv_warp_oracle as R
from opticalflow_amd import cv_resize, cv_warp, ops

pytestmark = pytest.mark.gpu

H, W = 100, 150                                    # the drivers' frame size: pads to 128 x 192


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


@functools.lru_cache(maxsize=None)
def _ref(name, run):
    n, src, dst, seed = R.WARP_CASES[name]
    M, inverse = R.case_matrices(name)[run]
    want = R.warp_frames(R.make_frames(n, src, seed), M, dst, inverse)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _net(device):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    return net.to(device).eval()


@functools.lru_cache(maxsize=None)
def _stream_frames():
    """Four consecutive raw frames, the script's matrix for their size, and the oracle's warp of each."""
    raw = R.make_frames(4, (H, W), 320)
    M = R.topview_matrix(W, H)
    warped = R.warp_frames(raw, M, (H, W))
    raw.setflags(write=False)
    warped.setflags(write=False)
    return raw, M, warped


@pytest.mark.parametrize("name", sorted(R.WARP_CASES))
def test_warp_equals_the_oracle(gpu_device, name):
    n, src, dst, seed = R.WARP_CASES[name]
    frames = R.make_frames(n, src, seed)
    dev = torch.from_numpy(frames).to(gpu_device)
    h, w = dst
    for run, (M, inverse) in enumerate(R.case_matrices(name)):
        want = _ref(name, run)
        got = cv_warp.warp_frames(dev, M, None if src == dst else dst, inverse_map=inverse)
        assert tuple(got.shape) == (n, h, w, 3) and got.dtype == torch.uint8
        got = got.cpu().numpy()
        assert np.array_equal(got, want), "%s run %d: %d of %d bytes differ" % (name, run, int((got != want).sum()), want.size)

        # out= into one half of a pair buffer; the other half and nothing else is touched
        buf = torch.full((n, 2, h, w, 3), 7, dtype=torch.uint8, device=gpu_device)
        assert cv_warp.warp_frames(dev, M, dst, inverse_map=inverse, out=buf[:, 1]).data_ptr() == buf[:, 1].data_ptr()
        got = buf.cpu().numpy()
        assert np.array_equal(got[:, 1], want) and bool((got[:, 0] == 7).all())

        # a source view with a larger batch stride, into an unaligned destination (the byte-store path whatever the width)
        wide = torch.full((n, 2) + src + (3,), 9, dtype=torch.uint8, device=gpu_device)
        wide[:, 0] = dev
        flat = torch.full((n * h * w * 3 + 1,), 7, dtype=torch.uint8, device=gpu_device)
        out = flat[1:].view(n, h, w, 3)
        cv_warp.warp_frames(wide[:, 0], M, dst, inverse_map=inverse, out=out)
        assert np.array_equal(out.cpu().numpy(), want) and int(flat[0]) == 7

    if name == "identity":
        assert np.array_equal(_ref(name, 0), frames)
    if name == "per_frame":                                                      # each frame is its own matrix's single-matrix warp
        (M, inverse), = R.case_matrices(name)
        for i in range(n):
            one = cv_warp.warp_frames(dev[i:i + 1], M[i], inverse_map=inverse).cpu().numpy()
            assert np.array_equal(one[0], _ref(name, 0)[i])


@pytest.mark.parametrize("name", sorted(R.TIE_CASES))
def test_tie_case_rounds_half_to_even(gpu_device, name):
    """The device result differs from the half-up statement in exactly the bytes the CPU test counted."""
    n, src, dst, seed = R.WARP_CASES[name]
    frames = R.make_frames(n, src, seed)
    (M, inverse), = R.case_matrices(name)
    got = cv_warp.warp_frames(torch.from_numpy(frames).to(gpu_device), M, inverse_map=inverse).cpu().numpy()
    up = R.warp_frames(frames, M, dst, inverse, half_up=True)
    assert int((got != up).sum()) == R.TIE_CASES[name]


def test_two_runs_give_the_same_bytes(gpu_device):
    frames = torch.from_numpy(R.make_frames(2, (150, 201), 330)).to(gpu_device)
    M = R.topview_matrix(201, 150)
    assert torch.equal(cv_warp.warp_frames(frames, M), cv_warp.warp_frames(frames, M))


def test_library_refuses_bad_arguments(gpu_device):
    src = torch.full((2, 8, 8, 3), 200, dtype=torch.uint8, device=gpu_device)
    out = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu_device)
    mats = torch.zeros(20, dtype=torch.float64, device=gpu_device)
    mats[:9] = torch.eye(3, dtype=torch.float64).reshape(9)
    mats[9:18] = mats[:9]
    lib = ops._lib.load()
    good = dict(src=src.data_ptr(), dst=out.data_ptr(), n=2, H=8, W=8, h=8, w=8, mat=mats.data_ptr(), ms=0, sb=192, db=192, stream=None)
    call = lambda **k: lib.pwc_cv_warp_perspective_u8(*{**good, **k}.values())
    for bad in (dict(src=None), dict(dst=None), dict(mat=None), dict(H=0), dict(w=0), dict(W=32768), dict(h=32768), dict(n=0),
                dict(sb=191), dict(db=191), dict(ms=5), dict(mat=mats.data_ptr() + 4)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert not out.any()                                                         # nothing was written
    assert call() == 0 and call(ms=9) == 0
    assert torch.equal(out, src)


def test_warp_frames_refuses_what_it_cannot_take(gpu_device):
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu_device)
    nan = np.eye(3)
    nan[0, 1] = np.nan
    for call in (lambda: cv_warp.warp_frames(frames.cpu(), np.eye(3)), lambda: cv_warp.warp_frames(frames.float(), np.eye(3)),
                 lambda: cv_warp.warp_frames(frames, np.ones((3, 3))), lambda: cv_warp.warp_frames(frames, nan),
                 lambda: cv_warp.warp_frames(frames, nan, inverse_map=True), lambda: cv_warp.warp_frames(frames, np.zeros((3, 3, 3)) + np.eye(3)),
                 lambda: cv_warp.warp_frames(frames, np.eye(3), out=torch.zeros((2, 8, 9, 3), dtype=torch.uint8, device=gpu_device)),
                 lambda: cv_warp.warp_frames(frames, np.eye(3), out=torch.zeros((2, 8, 8, 3), device=gpu_device)),
                 lambda: cv_warp.warp_frames(frames, np.eye(3), out=torch.zeros((2, 8, 16, 3), dtype=torch.uint8, device=gpu_device)[:, :, ::2])):
        with pytest.raises(ValueError):
            call()
    # prepare() makes the matrix resident once: the same tensor serves every later call
    M = R.topview_matrix(8, 8)
    assert cv_warp.prepare(M, gpu_device).data_ptr() == cv_warp.prepare(M.tolist(), gpu_device).data_ptr()
    assert cv_warp.prepare(M, gpu_device).data_ptr() != cv_warp.prepare(M, gpu_device, inverse_map=True).data_ptr()


def test_topview_infer(gpu_device):
    net = _net(gpu_device)
    raw, M, warped = _stream_frames()
    pairs = raw.reshape(2, 2, H, W, 3)
    wpairs = warped.reshape(2, 2, H, W, 3)
    dev = torch.from_numpy(pairs.copy()).to(gpu_device)
    pipe = cv_warp.TopviewInfer(net, H, W, gpu_device, M, batch=2)
    got = pipe(dev).clone()
    assert tuple(got.shape) == (2, 2, H, W) and bool(torch.isfinite(got).all())
    # the warped frames and the network's input are the oracles', bit for bit
    assert np.array_equal(pipe.warped.cpu().numpy(), wpairs)
    assert tuple(pipe.x_in.shape) == (2, 6, 128, 192)
    assert np.array_equal(_bits(pipe.x_in), RZ.ingest_pairs(wpairs, (128, 192), flip=True).view(np.int32))
    # the flow is CvGraphedInfer(mode="topview")'s on the oracle's warped frames
    plain = cv_resize.CvGraphedInfer(net, H, W, gpu_device, batch=2, mode="topview")
    want = plain(torch.from_numpy(wpairs.copy()).to(gpu_device)).clone()
    assert np.array_equal(_bits(got), _bits(want))
    # a second replay equals the first; fewer pairs than the batch
    assert np.array_equal(_bits(pipe(dev)), _bits(got))
    assert np.array_equal(_bits(pipe(dev[1:])), _bits(want[1:]))
    with pytest.raises(ValueError):
        pipe(dev[:, :, :50])


def test_topview_stream(gpu_device):
    net = _net(gpu_device)
    raw, M, warped = _stream_frames()
    dev = torch.from_numpy(raw.copy()).to(gpu_device)
    pipe = cv_warp.TopviewInfer(net, H, W, gpu_device, M, batch=1)
    stream = cv_warp.TopviewStream(net, H, W, gpu_device, M)
    with pytest.raises(ValueError):
        stream.push(dev[0])                                                      # not primed
    stream.prime(dev[0])
    for k in range(1, 4):
        flow = stream.push(dev[k])
        assert tuple(flow.shape) == (1, 2, H, W)
        want = pipe(torch.stack([dev[k - 1], dev[k]]))
        assert np.array_equal(_bits(flow), _bits(want)), k
        assert np.array_equal(stream.warped_current.cpu().numpy(), warped[k])
        assert np.array_equal(pipe.warped[0, 1].cpu().numpy(), warped[k])
