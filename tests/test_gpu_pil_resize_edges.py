"""Pillow-exact resize on the device at its edges, against the Pillow-made fixture tests/golden/g20_pil_resize_edges.npz (and the
NumPy oracle, which equals it): near-8 downscales over several tiles, strong upscales, outputs narrower than a quad, sources and
outputs that are not 4- or 16-byte aligned, ragged groups, special float values, Image.resize's rule for an unchanged axis and its
vertical-first order for tall sources.  Every comparison is equality of bytes or of float32 bit patterns; only a NaN's sign and
payload are left open.  Outputs are written into canary-filled buffers that are compared whole."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import pil_resize_oracle as R
from opticalflow_amd import ops, pil_resize

pytestmark = pytest.mark.gpu

MEAN, STD = R.IMAGENET_MEAN, R.IMAGENET_STD
TALL_FRAMES = ("tall", "tall_upx", "tall_edge_in")


@pytest.fixture(scope="module")
def golden():
    return load_golden("g20_pil_resize_edges.npz")


@pytest.fixture(scope="module")
def g17():
    return load_golden("g17_pil_resize.npz")


def _np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _bits(t):
    return np.ascontiguousarray(_np(t)).view(np.int32)


def _same_bits(got, want):
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), "%d of %d elements differ" % (int((_bits(got) != _bits(want)).sum()), want.size)


def _same_but_nan(got, want):
    """NaN at the same places, every other element bit-equal (so -0.0 is not +0.0); a NaN's sign and payload are not compared."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "NaN at %d places, Pillow has %d; %d places differ" % (int(gn.sum()), int(wn.sum()), int((gn != wn).sum()))
    assert np.array_equal(_bits(got)[~gn], _bits(want)[~wn]), "%d elements differ" % int((_bits(got)[~gn] != _bits(want)[~wn]).sum())


def _frame_case(golden, g17, name):
    """(frames uint8 [n,H,W,3], target, Pillow's bytes) of a named case of g20, or of g17."""
    if name in R.FRAME_EDGE_CASES:
        n, src, dst, seed = R.FRAME_EDGE_CASES[name]
        return R.make_frames(n, src, seed), dst, golden["frame_%s_u8" % name]
    n, src, dst, seed = R.FRAME_CASES[name]
    return R.make_frames(n, src, seed), dst, g17["frame_%s_u8" % name]


def _plane_case(golden, name):
    n, c, src, dst, seed = R.PLANE_EDGE_CASES[name]
    return R.make_planes(n, c, src, seed), dst, golden["plane_%s_f32" % name]


def _scaled(want, factors):
    """The per-channel factor as the kernel applies it: rounded to float32, the product in float32."""
    out = want.copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for c, f in enumerate(factors):
            out[:, c] *= np.float32(f)
    return out


def _single_launch_frames(dev, dst, mean=None, std=None, out=None, out_u8=None, group=None):
    """ops.pil_resize_frames itself: one launch, horizontal first, whatever the sizes."""
    n, H, W, _ = dev.shape
    h, w = dst
    d = dev.device
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=d)
    return ops.pil_resize_frames(dev, dst, pil_resize._axis_tables(W, w, True, d), pil_resize._axis_tables(H, h, True, d),
                                 pil_resize._lut(mean, std, d), out, out_u8, group)


def _single_launch_planes(x, dst, out=None):
    h, w = x.shape[2:]
    return ops.pil_resize_planes(x, dst, pil_resize._axis_tables(w, dst[1], False, x.device),
                                 pil_resize._axis_tables(h, dst[0], False, x.device), None, out)


# ------------------------------------------------------------------ named cases
@pytest.mark.parametrize("name", sorted(R.FRAME_EDGE_CASES))
def test_frames_equal_pillow(gpu_device, golden, name):
    n, src, dst, seed = R.FRAME_EDGE_CASES[name]
    frames = R.make_frames(n, src, seed)
    assert R.digest(frames) == str(golden["frame_%s_sha" % name])
    want8 = golden["frame_%s_u8" % name]
    dev = torch.from_numpy(frames).to(gpu_device)
    out, u8 = pil_resize.resize_frames(dev, dst, MEAN, STD, return_u8=True)
    got8 = u8.cpu().numpy()
    assert got8.shape == want8.shape
    assert np.array_equal(got8, want8), "%d of %d bytes differ from Pillow" % (int((got8 != want8).sum()), want8.size)
    _same_bits(out, R.normalise(want8, MEAN, STD))
    _same_bits(pil_resize.resize_frames(dev, dst), R.normalise(want8))                  # ToTensor only


@pytest.mark.parametrize("name", sorted(R.PLANE_EDGE_CASES))
def test_planes_equal_pillow(gpu_device, golden, name):
    n, c, src, dst, seed = R.PLANE_EDGE_CASES[name]
    x = R.make_planes(n, c, src, seed)
    assert R.digest(x) == str(golden["plane_%s_sha" % name])
    want = golden["plane_%s_f32" % name]
    dev = torch.from_numpy(x).to(gpu_device)
    if name == "chan5":                                    # channels 1..5 of a wider tensor: a batch stride and a start of their own
        wide = torch.full((n, 7) + src, 7.0, dtype=torch.float32, device=gpu_device)
        wide[:, 1:6] = dev
        dev = wide[:, 1:6]
    _same_bits(pil_resize.resize_planes(dev, dst), want)
    if name == "chan3":
        _same_bits(pil_resize.resize_planes(dev, dst, R.CHAN3_FACTORS), _scaled(want, R.CHAN3_FACTORS))
    if c == 2:
        _same_bits(pil_resize.resize_flow(dev, dst, scale_vectors=False), want)
        _same_bits(pil_resize.resize_flow(dev, dst), _scaled(want, (dst[1] / src[1], dst[0] / src[0])))
    else:
        factors = tuple(0.5 + ch for ch in range(c))
        _same_bits(pil_resize.resize_planes(dev, dst, factors), _scaled(want, factors))


@pytest.mark.parametrize("name", sorted(R.PLANE_SPECIAL_CASES))
def test_special_values_equal_pillow(gpu_device, golden, name):
    src, dst, seed = R.PLANE_SPECIAL_CASES[name]
    x = R.make_special(src, seed)
    assert R.digest(x) == str(golden["special_%s_sha" % name])
    want = golden["special_%s_f32" % name]
    dev = torch.from_numpy(x).to(gpu_device)
    _same_but_nan(pil_resize.resize_planes(dev, dst), want)
    _same_but_nan(pil_resize.resize_flow(dev, dst, scale_vectors=False), want)
    _same_but_nan(pil_resize.resize_flow(dev, dst), _scaled(want, (dst[1] / src[1], dst[0] / src[0])))
    if name == "identity":                                 # Pillow copies: the negative zero is still one, the NaN is alone
        got = _np(pil_resize.resize_planes(dev, dst))
        assert got[0, 0, 5, 7] == 0 and np.signbit(got[0, 0, 5, 7]) and int(np.isnan(got).sum()) == 1


# ------------------------------------------------------------------ the axis sweep
@pytest.mark.parametrize("O", R.SWEEP_OUT)
def test_axis_sweep(gpu_device, golden, O):
    bad = []
    for i, (o, src, dst) in enumerate(R.AXIS_SWEEP):
        if o != O:
            continue
        assert golden["sweep_geometry"][i].tolist() == list(src + dst)
        frame, plane = R.sweep_inputs(i)
        want8 = R.resize_u8(frame[0], dst)[None]
        out, u8 = pil_resize.resize_frames(torch.from_numpy(frame).to(gpu_device), dst, MEAN, STD, return_u8=True)
        got8 = u8.cpu().numpy()
        if got8.shape != want8.shape or not np.array_equal(got8, want8):
            bad.append(("u8", src, dst, int((got8 != want8).sum()) if got8.shape == want8.shape else -1))
        elif not np.array_equal(_bits(out), _bits(R.normalise(want8, MEAN, STD))):
            bad.append(("u8 normalised", src, dst, int((_bits(out) != _bits(R.normalise(want8, MEAN, STD))).sum())))
        if not np.array_equal(R.digest_bytes(got8[0]), golden["sweep_u8_sha"][i]):
            bad.append(("u8 digest", src, dst, -1))
        wantf = R.resize_f32(plane, dst)
        gotf = _np(pil_resize.resize_planes(torch.from_numpy(plane[None, None]).to(gpu_device), dst))[0, 0]
        if gotf.shape != wantf.shape or not np.array_equal(_bits(gotf), _bits(wantf)):
            bad.append(("f32", src, dst, int((_bits(gotf) != _bits(wantf)).sum()) if gotf.shape == wantf.shape else -1))
        if not np.array_equal(R.digest_bytes(gotf), golden["sweep_f32_sha"][i]):
            bad.append(("f32 digest", src, dst, -1))
    for b in bad:
        print("sweep O=%d: %s %s -> %s: %d elements differ" % ((O,) + b))
    assert not bad, bad[:10]


# ------------------------------------------------------------------ downscales beyond 8 to outputs shorter than a tile
@pytest.mark.parametrize("src,dst", [((126, 8), (14, 8)),          # 14 rows of ksize 19: the most a tile's vertical slice holds
                                     ((8, 512), (8, 32)),          # 32 columns of ksize 33: 1056 of the 1088 horizontal entries
                                     ((72, 8), (8, 8)), ((130, 29), (10, 3)), ((33, 130), (1, 2))])
def test_beyond_eight_to_short_outputs(gpu_device, src, dst):
    """narrow3 and to_one of the fixture need a downscale above 8; these are the corners of the range that admits them, against the
    oracle (which equals Pillow at such scales: test_oracle_equals_live_pillow_sweep goes to 40 -> 1)."""
    assert ops.pil_resize_supported(src, dst) and max(src[0] / dst[0], src[1] / dst[1]) > 8
    frames = R.make_frames(2, src, 801)
    want8 = np.stack([R.resize_u8(f, dst) for f in frames])
    _canary_run(torch.from_numpy(frames).to(gpu_device), dst, want8, 1, 1, 1, gpu_device)
    x = R.make_planes(1, 2, src, 802)
    _same_bits(pil_resize.resize_planes(torch.from_numpy(x).to(gpu_device), dst), R.resize_planes(x, dst))


# ------------------------------------------------------------------ groups that do not divide n
@pytest.mark.parametrize("name", ["group_ragged", "group_vec"])
def test_group_that_does_not_divide_n(gpu_device, golden, name):
    n, src, dst, seed = R.FRAME_EDGE_CASES[name]
    group, (h, w) = 2, dst
    assert n % group == 1
    dev = torch.from_numpy(R.make_frames(n, src, seed)).to(gpu_device)
    want = R.normalise(golden["frame_%s_u8" % name], MEAN, STD)
    halves = (n + group - 1) // group
    out = torch.full((group, 3 * halves, h, w), float("nan"), dtype=torch.float32, device=gpu_device)
    u8 = torch.full((n, h, w, 3), 0xA5, dtype=torch.uint8, device=gpu_device)
    _single_launch_frames(dev, dst, MEAN, STD, out=out, out_u8=u8, group=group)
    expect = np.full((group, 3 * halves, h, w), np.nan, np.float32)
    for f in range(n):
        expect[f % group, 3 * (f // group): 3 * (f // group) + 3] = want[f]
    assert np.isnan(expect[1, 3 * (halves - 1):]).all()                    # the slot no frame maps to
    _same_bits(out, expect)
    assert np.array_equal(u8.cpu().numpy(), golden["frame_%s_u8" % name])


# ------------------------------------------------------------------ misaligned source
@pytest.mark.parametrize("name", ["ragged", "near8", "up_thin"])
def test_source_not_dword_aligned(gpu_device, golden, g17, name):
    frames, dst, want8 = _frame_case(golden, g17, name)
    aligned, aligned8 = pil_resize.resize_frames(torch.from_numpy(frames).to(gpu_device), dst, MEAN, STD, return_u8=True)
    assert np.array_equal(aligned8.cpu().numpy(), want8)
    for off in (1, 2, 3):
        buf = torch.full((frames.size + 8,), 0xFF, dtype=torch.uint8, device=gpu_device)
        view = buf[off:off + frames.size].view(frames.shape)
        view.copy_(torch.from_numpy(frames))
        assert view.is_contiguous() and view.data_ptr() % 4 == off
        out, u8 = pil_resize.resize_frames(view, dst, MEAN, STD, return_u8=True)
        assert torch.equal(u8, aligned8), "offset %d: %d bytes differ" % (off, int((u8 != aligned8).sum()))
        _same_bits(out, aligned)


# ------------------------------------------------------------------ misaligned and strided outputs, canaries around every slice
def _canary_run(dev, dst, want8, off, extra, off8, gpu_device):
    """One launch into out at element offset `off` with batch stride 3hw + extra of a NaN buffer and bytes at offset `off8` of an
    0xA5 buffer; both buffers are compared whole."""
    n, (h, w) = dev.shape[0], dst
    bs = 3 * h * w + extra
    buf = torch.full((off + n * bs + 8,), float("nan"), dtype=torch.float32, device=gpu_device)
    out = buf.as_strided((n, 3, h, w), (bs, h * w, w, 1), off)
    buf8 = torch.full((off8 + want8.size + 8,), 0xA5, dtype=torch.uint8, device=gpu_device)
    u8 = buf8[off8:off8 + want8.size].view(want8.shape)
    _single_launch_frames(dev, dst, MEAN, STD, out=out, out_u8=u8)
    want = R.normalise(want8, MEAN, STD)
    expect = np.full(buf.shape, np.nan, np.float32)
    for f in range(n):
        expect[off + f * bs: off + f * bs + 3 * h * w] = want[f].reshape(-1)
    expect8 = np.full(buf8.shape, 0xA5, np.uint8)
    expect8[off8:off8 + want8.size] = want8.reshape(-1)
    got, got8 = _bits(buf), buf8.cpu().numpy()
    assert np.array_equal(got, _bits(expect)), "out offset %d, stride + %d: %d elements differ, %d of them outside the slice" % (
        off, extra, int((got != _bits(expect)).sum()), int(((got != _bits(expect)) & np.isnan(expect)).sum()))
    assert np.array_equal(got8, expect8), "bytes offset %d: %d differ, %d of them outside the slice" % (
        off8, int((got8 != expect8).sum()), int(((got8 != expect8)[:off8]).sum() + ((got8 != expect8)[off8 + want8.size:]).sum()))


@pytest.mark.parametrize("name", ["tile_exact", "group_vec"])
def test_quad_width_outputs_off_their_alignment(gpu_device, golden, g17, name):
    frames, dst, want8 = _frame_case(golden, g17, name)
    assert dst[1] % 4 == 0
    dev = torch.from_numpy(frames).to(gpu_device)
    for off, extra, off8 in ((0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 0, 3), (0, 1, 0), (1, 1, 3), (3, 1, 1), (4, 0, 0), (4, 4, 2)):
        _canary_run(dev, dst, want8, off, extra, off8, gpu_device)


@pytest.mark.parametrize("name", ["ragged", "group_ragged", "narrow3", "to_one"])
def test_ragged_width_outputs_stay_inside_their_slice(gpu_device, golden, g17, name):
    frames, dst, want8 = _frame_case(golden, g17, name)
    assert dst[1] in (67, 21, 3, 1)
    dev = torch.from_numpy(frames).to(gpu_device)
    for off, extra, off8 in ((0, 0, 0), (1, 0, 1), (2, 1, 2), (3, 0, 3)):
        _canary_run(dev, dst, want8, off, extra, off8, gpu_device)


@pytest.mark.parametrize("name", ["down_tiles", "tile_over", "tiny_up", "chan3", "to_one"])
def test_planes_one_float_into_their_buffers(gpu_device, golden, name):
    x, dst, want = _plane_case(golden, name)
    sbuf = torch.full((x.size + 9,), 7.0, dtype=torch.float32, device=gpu_device)
    src = sbuf[1:1 + x.size].view(x.shape)
    src.copy_(torch.from_numpy(x))
    dbuf = torch.full((want.size + 9,), float("nan"), dtype=torch.float32, device=gpu_device)
    out = dbuf[1:1 + want.size].view(want.shape)
    assert src.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 4
    _single_launch_planes(src, dst, out=out)
    expect = np.full(dbuf.shape, np.nan, np.float32)
    expect[1:1 + want.size] = want.reshape(-1)
    got = _bits(dbuf)
    assert np.array_equal(got, _bits(expect)), "%d elements differ, %d of them outside the slice" % (
        int((got != _bits(expect)).sum()), int(((got != _bits(expect)) & np.isnan(expect)).sum()))
    assert bool((sbuf[0] == 7.0).item()) and bool((sbuf[1 + x.size:] == 7.0).all().item())


# ------------------------------------------------------------------ the tall regime
@pytest.mark.parametrize("name", TALL_FRAMES)
def test_tall_frames_take_pillows_order(gpu_device, golden, name):
    n, src, dst, seed = R.FRAME_EDGE_CASES[name]
    assert pil_resize.vertical_first(src, dst)
    dev = torch.from_numpy(R.make_frames(n, src, seed)).to(gpu_device)
    want8 = golden["frame_%s_u8" % name]
    out, u8 = pil_resize.resize_frames(dev, dst, MEAN, STD, return_u8=True)
    assert np.array_equal(u8.cpu().numpy(), want8), "%d bytes differ from Pillow" % int((u8.cpu().numpy() != want8).sum())
    _same_bits(out, R.normalise(want8, MEAN, STD))
    buf = torch.zeros((n, 8) + dst, dtype=torch.float32, device=gpu_device)             # into a channel slice, as infer_resized does
    pil_resize.resize_frames(dev, dst, MEAN, STD, out=buf[:, 3:6])
    _same_bits(buf[:, 3:6], R.normalise(want8, MEAN, STD))
    assert not _np(buf[:, :3]).any() and not _np(buf[:, 6:]).any()
    # ops.pil_resize_frames itself is single-order: one launch gives the horizontal-first bytes, which are not Pillow's here
    one8 = torch.empty((n,) + dst + (3,), dtype=torch.uint8, device=gpu_device)
    _single_launch_frames(dev, dst, out_u8=one8)
    assert np.array_equal(one8.cpu().numpy(), np.stack([R.resize_u8(f, dst, tall_rule=False) for f in _np(dev)]))
    assert not np.array_equal(one8.cpu().numpy(), want8)


@pytest.mark.parametrize("name", ["tall", "tall_edge_in"])
def test_tall_planes_take_pillows_order(gpu_device, golden, name):
    x, dst, want = _plane_case(golden, name)
    assert pil_resize.vertical_first(x.shape[2:], dst)
    dev = torch.from_numpy(x).to(gpu_device)
    _same_bits(pil_resize.resize_planes(dev, dst), want)
    _same_bits(pil_resize.resize_flow(dev, dst), _scaled(want, (dst[1] / x.shape[3], dst[0] / x.shape[2])))
    one = _single_launch_planes(dev, dst)
    _same_bits(one, R.resize_planes(x, dst, tall_rule=False))
    assert not np.array_equal(_bits(one), _bits(want))


def test_outside_the_tall_regime_is_the_single_launch(gpu_device, golden):
    for name in ("tall_edge_out", "tall_no_down"):
        n, src, dst, seed = R.FRAME_EDGE_CASES[name]
        assert not pil_resize.vertical_first(src, dst)
        dev = torch.from_numpy(R.make_frames(n, src, seed)).to(gpu_device)
        out, u8 = pil_resize.resize_frames(dev, dst, MEAN, STD, return_u8=True)
        one8 = torch.empty_like(u8)
        one = _single_launch_frames(dev, dst, MEAN, STD, out_u8=one8)
        assert torch.equal(u8, one8) and np.array_equal(u8.cpu().numpy(), golden["frame_%s_u8" % name])
        _same_bits(out, one)
    x, dst, want = _plane_case(golden, "tall_edge_out")
    dev = torch.from_numpy(x).to(gpu_device)
    _same_bits(pil_resize.resize_planes(dev, dst), _single_launch_planes(dev, dst))
    _same_bits(pil_resize.resize_planes(dev, dst), want)


def test_tall_through_frame_ingest_and_a_captured_graph(gpu_device, golden):
    n, src, dst, seed = R.FRAME_EDGE_CASES["tall"]
    first = R.make_frames(1, src, seed)
    second = R.make_frames(1, src, seed + 1000)
    want1 = R.normalise(golden["frame_tall_u8"], MEAN, STD)
    want2 = R.normalise(R.resize_u8(second[0], dst)[None], MEAN, STD)
    ing = pil_resize.FrameIngest(dst, MEAN, STD, device=gpu_device, batch=1)
    img1, img2 = ing.pairs(first, second)
    assert tuple(img1._base.shape) == (1, 6) + dst
    _same_bits(img1, want1)
    _same_bits(img2, want2)

    x, _, wantp = _plane_case(golden, "tall")
    frames = torch.from_numpy(first).to(gpu_device)
    planes = torch.from_numpy(x).to(gpu_device)
    pil_resize.prepare(src, dst, gpu_device, True, MEAN, STD)                          # the tables of both launches, resident
    pil_resize.prepare(src, dst, gpu_device, False)
    torch.cuda.synchronize()
    out = torch.zeros((1, 3) + dst, dtype=torch.float32, device=gpu_device)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        pil_resize.resize_frames(frames, dst, MEAN, STD, out=out)
        up = pil_resize.resize_planes(planes, dst)
    out.zero_()
    up.zero_()
    g.replay()
    torch.cuda.synchronize()
    _same_bits(out, want1)
    _same_bits(up, wantp)
    frames.copy_(torch.from_numpy(second))                                            # new contents of the captured input, same graph
    g.replay()
    torch.cuda.synchronize()
    _same_bits(out, want2)
