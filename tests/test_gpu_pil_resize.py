"""Pillow-exact resize on the device against the Pillow-made fixture (tests/golden/g17_pil_resize.npz) and the NumPy oracle, bit for
bit: the 8-bit path is integer arithmetic; the float path is a fixed sequence of IEEE double multiplies and adds (the build keeps
them unfused), one double -> float rounding per pass and one float multiply."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import pil_resize_oracle as R
from opticalflow_amd import ops, pil_resize

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("g17_pil_resize.npz")


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).view(np.int32)


@pytest.mark.parametrize("name", sorted(R.FRAME_CASES))
def test_frames_equal_pillow(gpu_device, golden, name):
    n, src, dst, seed = R.FRAME_CASES[name]
    frames = R.make_frames(n, src, seed)
    assert R.digest(frames) == str(golden["frame_%s_sha" % name])
    want8 = golden["frame_%s_u8" % name]
    dev = torch.from_numpy(frames).to(gpu_device)
    h, w = dst

    out, u8 = pil_resize.resize_frames(dev, dst, R.IMAGENET_MEAN, R.IMAGENET_STD, return_u8=True)
    assert tuple(out.shape) == (n, 3, h, w) and tuple(u8.shape) == (n, h, w, 3)
    got8 = u8.cpu().numpy()
    assert np.array_equal(got8, want8), "%d of %d bytes differ from Pillow" % (int((got8 != want8).sum()), want8.size)
    want = R.normalise(want8, R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert np.array_equal(_bits(out), want.view(np.int32))
    if name == R.NORM_CASE:
        assert np.array_equal(_bits(out), golden["frame_%s_norm" % name].view(np.int32))

    plain = pil_resize.resize_frames(dev, dst)                                  # ToTensor only
    assert np.array_equal(_bits(plain), R.normalise(want8).view(np.int32))

    buf = torch.zeros((n, 8, h, w), dtype=torch.float32, device=gpu_device)     # the two halves of a wider network input
    pil_resize.resize_frames(dev, dst, R.IMAGENET_MEAN, R.IMAGENET_STD, out=buf[:, :3])
    pil_resize.resize_frames(dev, dst, out=buf[:, 3:6])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:, :3].view(np.int32), want.view(np.int32))
    assert np.array_equal(got[:, 3:6].view(np.int32), R.normalise(want8).view(np.int32))
    assert not got[:, 6:].any()


@pytest.mark.parametrize("name", sorted(R.FLOW_CASES))
def test_flow_equals_pillow(gpu_device, golden, name):
    B, src, dst, seed = R.FLOW_CASES[name]
    flow = R.make_flow(B, src, seed)
    assert R.digest(flow) == str(golden["flow_%s_sha" % name])
    want = golden["flow_%s_f32" % name]
    dev = torch.from_numpy(flow).to(gpu_device)
    got = pil_resize.resize_flow(dev, dst, scale_vectors=False)
    assert tuple(got.shape) == (B, 2) + tuple(dst)
    assert np.array_equal(_bits(got), want.view(np.int32)), "%d elements differ" % int((_bits(got) != want.view(np.int32)).sum())
    scaled = want.copy()                                                        # inference.py:187-188 on the fixture's planes
    scaled[:, 0] *= (dst[1] / src[1])
    scaled[:, 1] *= (dst[0] / src[0])
    assert np.array_equal(_bits(pil_resize.resize_flow(dev, dst)), scaled.view(np.int32))
    # a batch stride larger than the tensor: the flow as the first two channels of a wider one
    wide = torch.full((B, 3) + tuple(src), 7.0, dtype=torch.float32, device=gpu_device)
    wide[:, :2] = dev
    assert np.array_equal(_bits(pil_resize.resize_flow(wide[:, :2], dst, scale_vectors=False)), want.view(np.int32))


def test_two_runs_give_the_same_bits(gpu_device):
    frames = torch.from_numpy(R.make_frames(2, (150, 201), 301)).to(gpu_device)
    a, a8 = pil_resize.resize_frames(frames, (70, 67), R.IMAGENET_MEAN, R.IMAGENET_STD, return_u8=True)
    b, b8 = pil_resize.resize_frames(frames, (70, 67), R.IMAGENET_MEAN, R.IMAGENET_STD, return_u8=True)
    assert torch.equal(a8, b8) and np.array_equal(_bits(a), _bits(b))
    flow = torch.from_numpy(R.make_flow(2, (40, 64), 302)).to(gpu_device)
    assert np.array_equal(_bits(pil_resize.resize_flow(flow, (61, 77))), _bits(pil_resize.resize_flow(flow, (61, 77))))


def test_out_of_range_scale_raises(gpu_device):
    # 129 -> 16 is the first length past a downscale of 8 whose 16 rows of coefficients (ksize 19) no longer fit a tile's slice
    frames = torch.zeros((1, 129, 8, 3), dtype=torch.uint8, device=gpu_device)
    assert ops.pil_resize_supported((128, 8), (16, 8)) and not ops.pil_resize_supported((129, 8), (16, 8))
    with pytest.raises(ValueError, match="supported range"):
        pil_resize.resize_frames(frames, (16, 8))
    with pytest.raises(ValueError, match="supported range"):
        pil_resize.resize_flow(torch.zeros((1, 2, 4, 513), device=gpu_device), (4, 64))
    # the library refuses it too when the wrapper's check is bypassed
    xt = pil_resize._axis_tables(8, 8, True, gpu_device)
    yt = pil_resize._axis_tables(129, 16, True, gpu_device)
    out = torch.empty((1, 3, 16, 8), device=gpu_device)
    with pytest.raises(ops.PwcHipError, match="supported"):
        ops.pil_resize_frames(frames, (16, 8), xt, yt, pil_resize._lut(None, None, gpu_device), out)


def test_frame_ingest_pairs_equal_per_frame_resize(gpu_device):
    f = R.make_frames(6, (90, 75), 303)
    ing = pil_resize.FrameIngest((40, 52), R.IMAGENET_MEAN, R.IMAGENET_STD, device=gpu_device, batch=3)
    for first, second in ((f[:3], f[3:]), ([f[4], f[0]], [f[1], f[5]])):         # a full batch, then a short one from a list
        img1, img2 = ing.pairs(first, second)
        B = len(first)
        assert tuple(img1.shape) == (B, 3, 40, 52) and tuple(img1._base.shape) == (B, 6, 40, 52)
        for frames, img in ((first, img1), (second, img2)):
            for i in range(B):
                one = pil_resize.resize_frames(torch.from_numpy(np.asarray(frames[i])[None]).to(gpu_device), (40, 52),
                                               R.IMAGENET_MEAN, R.IMAGENET_STD)
                assert np.array_equal(_bits(img[i]), _bits(one[0]))
    with pytest.raises(ValueError):
        ing.pairs([f[0]], [np.zeros((90, 76, 3), np.uint8)])


def test_resize_runs_inside_a_captured_graph(gpu_device):
    src, dst = (94, 311), (96, 320)
    frames = torch.from_numpy(R.make_frames(2, src, 304)).to(gpu_device)
    flow = torch.from_numpy(R.make_flow(2, (24, 80), 305)).to(gpu_device)
    eager_x = pil_resize.resize_frames(frames, dst, R.IMAGENET_MEAN, R.IMAGENET_STD)        # also makes the tables resident
    eager_f = pil_resize.resize_flow(flow, src)
    x = torch.zeros_like(eager_x)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pil_resize.resize_frames(frames, dst, R.IMAGENET_MEAN, R.IMAGENET_STD, out=x)
        up = pil_resize.resize_flow(flow, src)
    x.zero_()
    up.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(x), _bits(eager_x)) and np.array_equal(_bits(up), _bits(eager_f))
    # new contents of the captured inputs, same graph
    frames.copy_(torch.from_numpy(R.make_frames(2, src, 306)).to(gpu_device))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(x), _bits(pil_resize.resize_frames(frames, dst, R.IMAGENET_MEAN, R.IMAGENET_STD)))


def test_infer_resized_equals_the_hand_composed_chain(gpu_device):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(gpu_device).eval()
    src, size = (94, 311), (128, 320)
    f1 = torch.from_numpy(R.make_frames(2, src, 307)).to(gpu_device)
    f2 = torch.from_numpy(R.make_frames(2, src, 308)).to(gpu_device)
    got = pil_resize.infer_resized(net, f1, f2, size, R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert tuple(got.shape) == (2, 2, 94, 311) and bool(torch.isfinite(got).all())
    with torch.no_grad():
        x = torch.cat([pil_resize.resize_frames(f1, size, R.IMAGENET_MEAN, R.IMAGENET_STD),
                       pil_resize.resize_frames(f2, size, R.IMAGENET_MEAN, R.IMAGENET_STD)], 1)
        want = pil_resize.resize_flow(net(x), src)
    assert np.array_equal(_bits(got), _bits(want))
    # the input the model saw is Pillow's: the oracle on the host makes the same bytes
    want8 = np.stack([R.resize_u8(f, size) for f in f1.cpu().numpy()])
    assert np.array_equal(_bits(x[:, :3]), R.normalise(want8, R.IMAGENET_MEAN, R.IMAGENET_STD).view(np.int32))
