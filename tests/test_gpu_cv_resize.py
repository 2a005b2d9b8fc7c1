"""cv2.resize-exact ingest and flow exit on the device (csrc/pwc_cv_resize.hip, opticalflow_amd/cv_resize.py) against the NumPy oracle
(tests/cv_resize_oracle.py, held to harness.cv2_resize_linear by tests/test_cv_resize_cpu.py), bit for bit: the 8-bit path is integer
arithmetic behind a table, the float path a fixed sequence of float32 multiplies and adds that the build keeps unfused.  NaN is
compared by position (a CPU and the GPU give 0 x inf different payloads).  cv2 parity is unpinned."""
import functools

import numpy as np
import pytest
import torch

import cv_resize_oracle as R
from opticalflow_amd import cv_resize, harness, ops

pytestmark = pytest.mark.gpu


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


@functools.lru_cache(maxsize=None)
def _frame_ref(name, flip, norm):
    n, src, dst, seed = R.FRAME_CASES[name]
    mean, std = (R.IMAGENET_MEAN, R.IMAGENET_STD) if norm else (None, None)
    want = R.ingest(R.make_frames(n, src, seed), dst, flip, mean, std)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def _net(device):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    return net.to(device).eval()


@pytest.mark.parametrize("name", sorted(R.FRAME_CASES))
def test_frames_equal_the_oracle(gpu_device, name):
    n, src, dst, seed = R.FRAME_CASES[name]
    frames = R.make_frames(n, src, seed)
    dev = torch.from_numpy(frames).to(gpu_device)
    h, w = dst
    size = None if harness.padded_size(*src) == dst else dst                     # the default size where it is the case's
    norm = cv_resize.byte_lut(R.IMAGENET_MEAN, R.IMAGENET_STD)
    for flip in (True, False):
        got = cv_resize.resize_frames(dev, size, flip_channels=flip)
        assert tuple(got.shape) == (n, 3, h, w)
        want = _frame_ref(name, flip, False)
        assert np.array_equal(_bits(got), want.view(np.int32)), "%d of %d differ" % (int((_bits(got) != want.view(np.int32)).sum()), want.size)
        got = cv_resize.resize_frames(dev, dst, flip_channels=flip, lut=norm)
        assert np.array_equal(_bits(got), _frame_ref(name, flip, True).view(np.int32))

    # the pair layout through out_group: frames [first halves, second halves] with group = n fill [n,6,h,w]
    both = torch.cat([dev, dev.flip(0)])
    x = torch.zeros((n, 6, h, w), dtype=torch.float32, device=gpu_device)
    ops.cv_resize_frames(both, dst, cv_resize._axis(src[1], w, gpu_device), cv_resize._axis(src[0], h, gpu_device),
                         cv_resize._lut(None, gpu_device), x, True, n)
    want = _frame_ref(name, True, False)
    assert np.array_equal(_bits(x[:, :3]), want.view(np.int32)) and np.array_equal(_bits(x[:, 3:]), want[::-1].view(np.int32))
    # ... and pairs [n,2,H,W,3] in one launch
    pairs = torch.stack([dev, dev.flip(0)], dim=1).contiguous()
    xp = cv_resize.ingest_pairs(pairs, size=dst)
    assert np.array_equal(_bits(xp), _bits(x))

    # channel slices of a wider tensor; the rest stays untouched
    buf = torch.full((n, 8, h, w), 7.0, dtype=torch.float32, device=gpu_device)
    cv_resize.resize_frames(dev, dst, flip_channels=True, lut=norm, out=buf[:, :3])
    cv_resize.resize_frames(dev, dst, flip_channels=False, out=buf[:, 3:6])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :3].view(np.int32), _frame_ref(name, True, True).view(np.int32))
    assert np.array_equal(got[:, 3:6].view(np.int32), _frame_ref(name, False, False).view(np.int32))
    assert bool((got[:, 6:] == 7.0).all())


@pytest.mark.parametrize("name", sorted(R.TIE_CASES))
def test_tie_cases_round_half_to_even(gpu_device, name):
    """The device result differs from the half-up statement in exactly the bytes the CPU test counted."""
    n, src, dst, seed = R.FRAME_CASES[name]
    frames = R.make_frames(n, src, seed)
    got = cv_resize.resize_frames(torch.from_numpy(frames).to(gpu_device), dst, flip_channels=False).cpu().numpy()
    up = R.ingest(frames, dst, flip=False, half_up=True)
    assert int((got != up).sum()) == R.TIE_CASES[name]


@pytest.mark.parametrize("name", sorted(R.FLOW_CASES))
def test_flow_equals_the_oracle(gpu_device, name):
    n, src, dst, seed = R.FLOW_CASES[name]
    flow = R.make_flow(n, src, seed, specials=name == R.SPECIALS_CASE)
    dev = torch.from_numpy(flow).to(gpu_device)
    wide = torch.full((n, 3) + tuple(src), 7.0, dtype=torch.float32, device=gpu_device)   # a batch stride larger than the tensor
    wide[:, :2] = dev
    fu, fv = R.script_factors(dst, src)
    for gain in (20.0, 1.0):
        want = R.flow_exit(flow, dst, gain, fu, fv)
        for layout in ("chw", "hwc"):
            w = np.ascontiguousarray(want.transpose(0, 2, 3, 1)) if layout == "hwc" else want
            got = cv_resize.resize_flow(dev, dst, gain=gain, layout=layout)
            assert tuple(got.shape) == w.shape
            assert R.same_bits_nan_by_position(got.cpu().numpy(), w), (gain, layout)
            assert R.same_bits_nan_by_position(cv_resize.resize_flow(wide[:, :2], dst, gain=gain, layout=layout).cpu().numpy(), w)
        plain = R.flow_exit(flow, dst, gain, 1.0, 1.0)
        assert R.same_bits_nan_by_position(cv_resize.resize_flow(dev, dst, gain=gain, scale_vectors=False).cpu().numpy(), plain)
    if name == R.SPECIALS_CASE:                                                  # equal sizes: a copy, the specials stay where they are
        got = cv_resize.resize_flow(dev, dst, gain=1.0, scale_vectors=False).cpu().numpy()
        assert R.same_bits_nan_by_position(got, flow)
        assert np.signbit(got[0, 0, 1, 2]) and got[0, 0, 1, 2] == 0 and np.isposinf(got[0, 1, 3, 5]) and np.isneginf(got[-1, 0, 7, 11])
        assert int(np.isnan(got).sum()) == 1 and int(np.isinf(got).sum()) == 2
    if name == "harness":                                                        # the bound tests/test_harness.py uses for this geometry
        got = cv_resize.resize_flow(dev, dst, gain=20.0, layout="hwc").cpu().numpy()[0]
        real = np.stack([R.real_bilinear(flow[0, c].astype(np.float64) * 20.0, dst) for c in range(2)], axis=-1)
        real[:, :, 0] *= dst[1] / (4.0 * src[1])
        real[:, :, 1] *= dst[0] / (4.0 * src[0])
        assert np.abs(got - real).max() < 2e-4


def test_library_refuses_bad_arguments(gpu_device):
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device=gpu_device)
    xt, yt = cv_resize._axis(8, 64, gpu_device), cv_resize._axis(8, 64, gpu_device)
    lut = cv_resize._lut(None, gpu_device)
    lib = ops._lib.load()
    out = torch.zeros((2, 3, 64, 64), device=gpu_device)
    args = lambda o, bs, g: (frames.data_ptr(), o, 2, 8, 8, 64, 64, xt[0].data_ptr(), xt[1].data_ptr(), yt[0].data_ptr(), yt[1].data_ptr(),
                             lut.data_ptr(), 1, bs, g, None)
    assert lib.pwc_cv_resize_frames_u8(*args(out.data_ptr(), 3 * 64 * 64 - 1, 2)) != 0      # batch stride smaller than the tensor
    assert lib.pwc_cv_resize_frames_u8(*args(out.data_ptr(), 3 * 64 * 64, 0)) != 0          # group
    assert lib.pwc_cv_resize_frames_u8(*args(None, 3 * 64 * 64, 2)) != 0                    # null
    assert lib.pwc_cv_resize_frames_u8(*args(out.data_ptr() + 2, 3 * 64 * 64, 2)) != 0      # alignment
    torch.cuda.synchronize()
    assert not out.any()                                                         # nothing was launched
    flow = torch.zeros((1, 2, 4, 4), device=gpu_device)
    with pytest.raises(ValueError):
        cv_resize.resize_flow(flow, (8, 8), out=torch.zeros((1, 2, 8, 9), device=gpu_device))
    with pytest.raises(ValueError):
        cv_resize.ingest_pairs(frames.view(1, 2, 8, 8, 3), out=torch.zeros((1, 6, 64, 128), device=gpu_device)[..., :64])


def test_two_runs_give_the_same_bits(gpu_device):
    frames = torch.from_numpy(R.make_frames(2, (150, 201), 301)).to(gpu_device)
    assert np.array_equal(_bits(cv_resize.resize_frames(frames)), _bits(cv_resize.resize_frames(frames)))
    flow = torch.from_numpy(R.make_flow(2, (48, 64), 302)).to(gpu_device)
    a, b = cv_resize.resize_flow(flow, (150, 201), gain=20.0, layout="hwc"), cv_resize.resize_flow(flow, (150, 201), gain=20.0, layout="hwc")
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("mode", ["script", "topview"])
def test_graphed_pipeline(gpu_device, mode):
    net = _net(gpu_device)
    H, W = 100, 150
    pairs = R.make_frames(4, (H, W), 310).reshape(2, 2, H, W, 3)
    dev = torch.from_numpy(pairs).to(gpu_device)
    gain, layout = (20.0, "hwc") if mode == "script" else (1.0, "chw")
    pipe = cv_resize.CvGraphedInfer(net, H, W, gpu_device, batch=2, mode=mode)
    got = pipe(dev).clone()
    assert tuple(got.shape) == ((2, H, W, 2) if mode == "script" else (2, 2, H, W)) and bool(torch.isfinite(got).all())
    # the replay equals the eager composition, bit for bit, and a second replay the first
    with torch.no_grad():
        x = cv_resize.ingest_pairs(dev)
        flow2 = net(x)
        want = cv_resize.resize_flow(flow2, (H, W), gain=gain, layout=layout)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(pipe(dev)), _bits(got))
    # its input tensor is the oracle's, its output the oracle's exit applied to the downloaded flow2
    assert tuple(pipe.x_in.shape) == (2, 6, 128, 192)
    assert np.array_equal(_bits(pipe.x_in), R.ingest_pairs(pairs, (128, 192), flip=True).view(np.int32))
    q = pipe.flow_quarter.cpu().numpy()
    assert q.shape == (2, 2, 32, 48) and np.array_equal(q.view(np.int32), _bits(flow2))
    exit_ = R.flow_exit(q, (H, W), gain, W / 192.0, H / 128.0, hwc=layout == "hwc")
    assert np.array_equal(_bits(got), exit_.view(np.int32))
    # fewer pairs than the batch
    assert np.array_equal(_bits(pipe(dev[1:])), _bits(got[1:]))
    if mode == "script":
        # estimate_flow through the kernels against the torch chain: the bar of test_estimate_flow_end_to_end (the inputs differ by one
        # ulp for 126 byte values)
        im1, im2 = torch.from_numpy(pairs[0, 0]), torch.from_numpy(pairs[0, 1])
        hip = harness.estimate_flow(net, im1, im2, prepost="hip")
        tor = harness.estimate_flow(net, im1, im2, prepost="torch")
        assert tuple(hip.shape) == (H, W, 2)
        mad = (hip - tor).abs().mean().item()
        print("estimate_flow hip vs torch: mean |d| %.3e" % mad)
        assert mad < 1e-3
        # an alpha channel is dropped
        rgba = torch.cat([im1, torch.full((H, W, 1), 255, dtype=torch.uint8)], dim=2)
        assert np.array_equal(_bits(harness.estimate_flow(net, rgba, im2, prepost="hip")), _bits(hip))
