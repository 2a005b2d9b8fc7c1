"""The launch audit's comparators (tests/launch_audit.py) must catch realistic kernel bugs: each mutation of a small synthetic launch,
built with torch on the CPU, fails its bound, and the unmutated result passes.  No GPU."""
import torch
import torch.nn.functional as F

import launch_audit as LA


def _conv_case(seed=5, B=2, cin=32, cout=16, H=16, W=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


def _fp32_conv(x, w, b, act=True):
    y = F.conv2d(x, w, b, padding=1)
    return F.leaky_relu(y, LA.LEAKY) if act else y


def _passes(got, ref, s, rel):
    return LA.worst(LA.bounded_ratio(got, ref, s, rel))[0] <= 1.0


def test_clean_fp32_convolution_passes_every_conv_bound():
    x, w, b = _conv_case()
    ref, s = LA.conv_ref(x, w, b)
    got = _fp32_conv(x, w, b)
    for rel in (LA.REL_DIRECT, LA.REL_WINO2, LA.REL_WINO4):
        assert _passes(got, ref, s, rel)
    assert _passes(LA.split2(got), LA.split2(ref), LA.split2(s), LA.REL_WINO4)


def test_dropped_input_channel_of_one_cin_slice_fails():
    x, w, b = _conv_case()
    ref, s = LA.conv_ref(x, w, b)
    xm = x.clone()
    xm[:, 19] = 0                          # the fourth channel of the second 16-channel slice never accumulated
    r, _, chans = LA.worst(LA.bounded_ratio(_fp32_conv(xm, w, b), ref, s, LA.REL_WINO4))
    assert r > 1 and len(chans) > 0


def test_one_tile_edge_pixel_off_by_ten_bounds_fails():
    x, w, b = _conv_case()
    ref, s = LA.conv_ref(x, w, b)
    got = _fp32_conv(x, w, b)
    got[1, 5, 7, 31] += 10 * LA.REL_WINO4 * s[1, 5, 7, 31].item()   # last row and column of an 8 x 32 tile
    r, idx, chans = LA.worst(LA.bounded_ratio(got, ref, s, LA.REL_WINO4))
    assert r > 1 and idx == (1, 5, 7, 31) and chans == [5]


def test_swapped_lattice_images_fail():
    x, w, b = _conv_case()
    ref, s = LA.conv_ref(x, w, b)
    got = LA.split2(_fp32_conv(x, w, b))
    assert _passes(got, LA.split2(ref), LA.split2(s), LA.REL_WINO4)
    got = got[[0, 2, 1, 3, 4, 5, 6, 7]]
    assert not _passes(got, LA.split2(ref), LA.split2(s), LA.REL_WINO4)
    # the nested unsplit restatement is exact and inverts split2
    t = torch.randn(1, 3, 16, 32)
    lat = LA.split2(LA.split2(LA.split2(t)))
    assert torch.equal(LA.unsplit(lat, 3), t)
    assert not torch.equal(LA.unsplit(lat[[1, 0] + list(range(2, 64))], 3), t)


def test_shifted_correlation_plane_fails():
    g = torch.Generator().manual_seed(8)
    c1, c2 = torch.randn(1, 8, 12, 40, generator=g), torch.randn(1, 8, 12, 40, generator=g)
    ref, s = LA.corr_ref(c1, c2)
    got = ref.float()
    assert _passes(got, ref, s, LA.REL_CORR)
    got[:, 30] = torch.roll(got[:, 30], 1, dims=-1)
    r, _, chans = LA.worst(LA.bounded_ratio(got, ref, s, LA.REL_CORR))
    assert r > 1 and chans == [30]


def test_missing_bias_of_one_channel_fails():
    x, w, b = _conv_case()
    ref, s = LA.conv_ref(x, w, b, act=False)
    bm = b.clone()
    bm[9] = 0
    r, _, chans = LA.worst(LA.bounded_ratio(_fp32_conv(x, w, bm, act=False), ref, s, LA.REL_DIRECT))
    assert r > 1 and chans == [9]


def test_warp_taps_restatement_matches_the_oracle_and_counts_threshold_pixels():
    """the float32 taps (the kernel's arithmetic) blended in float64 agree with oracle.warp to float32 coordinate rounding"""
    from oracle import pwc_oracle as O
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 5, 9, 40, generator=g)
    flo = torch.randn(2, 2, 9, 40, generator=g) * 3
    for align, thr in ((False, 0.9999), (True, 0.999)):
        taps = LA.warp_taps(flo, 2.5, align, thr)
        got = LA.warp_apply(x, taps)
        ref = O.warp(x.double(), flo.double() * 2.5, align_corners=align, mask_threshold=thr)
        keep = ~LA.near_threshold(taps, thr)
        assert ((got - ref).abs() * keep.unsqueeze(1)).max().item() < 1e-4
        assert taps[4].any() and not taps[4].all()


def test_exact_comparator_rejects_any_change():
    t = torch.randn(2, 3, 4, 8)
    assert LA.worst(LA.bounded_ratio(t, t.double(), torch.zeros_like(t), 0.0))[0] == 0.0
    u = t.clone()
    u[0, 0, 0, 0] = torch.nextafter(u[0, 0, 0, 0], torch.tensor(10.0))
    assert LA.worst(LA.bounded_ratio(u, t.double(), torch.zeros_like(t), 0.0))[0] == float("inf")
    assert LA.pick_images(4, 0) == list(range(4))
    p = LA.pick_images(64, 3)
    assert p[0] == 0 and p[-1] == 63 and len(p) == 4 and p == LA.pick_images(64, 3)
