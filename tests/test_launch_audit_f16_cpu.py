"""The half-precision launch audit's comparators (tests/launch_audit_f16.py) must catch realistic kernel bugs: each mutation of a
small synthetic launch, restated with torch on the CPU, fails its bound, and the unmutated restatement passes.  No GPU."""
import torch
import torch.nn.functional as F

import launch_audit_f16 as A

LEAKY = A.LA.LEAKY


def _case(seed=5, B=2, cin=64, cout=24, H=16, W=64):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, H, W, generator=g).half().float()           # the kernels' inputs are halves
    w = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    return x, w, b


def _kernel_conv(x, weff, b, act=True):
    """the kernel's arithmetic: exact products, accumulation, the fp32 value before the store (float64 here: within REL_F16 S of
    the fp32 sum)"""
    y = F.conv2d(x.double(), weff.double(), b.double(), padding=1)
    return F.leaky_relu(y, LEAKY) if act else y


def _ratio(got, ref, s, **kw):
    return A.worst(A.half_ratio(got, ref, s, **kw))


def _round_toward_zero(v: torch.Tensor) -> torch.Tensor:
    h = v.float().clamp(-A.HALF_MAX, A.HALF_MAX).half()
    over = h.double().abs() > v.abs()
    step = torch.nextafter(h, torch.zeros_like(h))
    return torch.where(over, step, h)


def test_clean_restatement_passes_and_rtz_store_fails():
    x, w, b = _case()
    weff = A.sat_half(w).double()
    ref, s = A.LA.conv_ref(x, weff, b)
    v = _kernel_conv(x, weff, b)
    assert _ratio(A.sat_half(v.float()), ref, s)[0] <= 1.0
    assert _ratio(v.float(), ref, s, half_out=False)[0] <= 1.0
    assert _ratio(_round_toward_zero(v), ref, s)[0] > 1.0


def test_one_value_one_half_ulp_past_the_rounding_fails():
    x, w, b = _case()
    weff = A.sat_half(w).double()
    ref, s = A.LA.conv_ref(x, weff, b)
    got = A.sat_half(_kernel_conv(x, weff, b).float())
    i = (1, 7, 9, 31)
    away = torch.tensor(float("inf") if got[i] > ref[i] else float("-inf"), dtype=torch.float16)
    got[i] = torch.nextafter(got[i], away)                               # one half ulp further from the true value
    r, idx, chans = _ratio(got, ref, s)
    assert r > 1.0 and idx == i and chans == [7]


def test_dropped_small_channel_group_fails():
    x, w, b = _case()
    w[:, 40:48] *= 1e-2                                                  # a channel group that contributes little
    weff = A.sat_half(w).double()
    ref, s = A.LA.conv_ref(x, weff, b)
    xm = x.clone()
    xm[:, 40:48] = 0                                                     # ... never accumulated
    assert _ratio(A.sat_half(_kernel_conv(xm, weff, b).float()), ref, s)[0] > 1.0


def test_split_layer_with_plain_half_filters_fails():
    x, w, b = _case()
    weff = A.split_filters(w)
    assert bool(((weff - w.double()).abs() <= A.SPLIT_REL * w.double().abs() + A.SPLIT_ABS).all())
    ref, s = A.LA.conv_ref(x, weff, b, act=False)
    good = _kernel_conv(x, weff, b, act=False)
    plain = _kernel_conv(x, A.sat_half(w).double(), b, act=False)
    for out_f32 in (True, False):
        rnd = (lambda t: t.float()) if out_f32 else (lambda t: A.sat_half(t.float()))
        assert _ratio(rnd(good), ref, s, half_out=not out_f32)[0] <= 1.0
        assert _ratio(rnd(plain), ref, s, half_out=not out_f32)[0] > 1.0
    # plain half filters are not ~22-bit filters
    assert not bool(((A.sat_half(w).double() - w.double()).abs() <= A.SPLIT_REL * w.double().abs() + A.SPLIT_ABS).all())


def test_garbage_in_a_pad_lane_fails():
    t = torch.zeros(2, 3, 4, 8, 8, dtype=torch.float16)
    assert A._pad_lanes_zero(t, 20)
    t[1, 2, 3, 5, 4] = float("nan")                                      # channel 20 of C = 20: a pad lane
    assert not A._pad_lanes_zero(t, 20)
    assert A._pad_lanes_zero(t, 24)


def test_store_one_group_past_the_output_slice_fails():
    arena = torch.zeros(2, 9, 4, 16, 8, dtype=torch.float16)
    out = arena[:, 3:5]
    g = A._Guard([out])
    out.fill_(1.5)
    assert g.stray() == 0
    g = A._Guard([out])
    arena[:, 3:6] = 1.5                                                  # the tile writes one channel group too many
    assert g.stray() == 2 * 4 * 16 * 8
    head = torch.zeros(2, 2, 4, 16, 8)                                   # fp32 outputs are watched word by word too
    g = A._Guard([head[:, 0:1]])
    head[0, 1, 3, 15, 7] = 1.1
    assert g.stray() == 2


def test_lo_as_half_x_minus_hi_fails():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 7, generator=g) * 3
    hi = A.sat_half(x)
    lo = A.sat_half(x - hi.float())
    assert bool((lo != 0).any())
    wrong = (x.half() - hi).half()                                       # half(x) - hi: the residual is lost
    assert not torch.equal(wrong.view(torch.int16), lo.view(torch.int16))
    # hi + lo carries x to ~22 bits (down to the subnormal step of lo)
    assert bool(((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -22 * x.double().abs() + A.T16).all())


def test_swapped_deconvolution_tap_fails():
    g = torch.Generator().manual_seed(6)
    flow = torch.randn(2, 2, 6, 10, generator=g) * 3
    dw, db = torch.randn(2, 2, 4, 4, generator=g), torch.randn(2, generator=g)
    ref = F.conv_transpose2d(flow.double(), dw.double(), db.double(), stride=2, padding=1)
    s = F.conv_transpose2d(flow.double().abs(), dw.double().abs(), db.double().abs(), stride=2, padding=1)
    up = A.entry_up_flow(flow, dw, db)
    assert A.worst(A.LA.bounded_ratio(up, ref, s, A.LA.REL_DECONV))[0] <= 1.0
    assert A.worst(A.LA.bounded_ratio(A.entry_up_flow(flow, dw, db, swap_tap=True), ref, s, A.LA.REL_DECONV))[0] > 1.0
    # the flow group compares sat_half(up_flow32) bit for bit
    assert torch.equal(A.sat_half(up).view(torch.int16), A.sat_half(up.clone()).view(torch.int16))
    # the pixel shuffle of upfeat's phases: channel co*4 + py*2 + px lands at (2Y + py, 2X + px)
    ph = torch.randn(1, 1, 3, 4, 8, generator=g)
    f = A.feat_shuffle(ph)
    for co in range(2):
        for py in range(2):
            for px in range(2):
                assert torch.equal(f[0, co, py::2, px::2], ph[0, 0, :, :, co * 4 + py * 2 + px])


def test_pyramid1_stage_with_replicate_padding_fails():
    g = torch.Generator().manual_seed(9)
    img = torch.rand(1, 3, 32, 64, generator=g)
    shapes = ((16, 3, 2), (16, 16, 1), (16, 16, 1), (32, 16, 2))
    layers = [(A.sat_half(torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5).float(),
               torch.randn(co, generator=g) * 0.02, st) for co, ci, st in shapes]
    ref, allow = A.pyr1_chain(img, layers)
    # the kernel: halves between the stages, exact products, each stage rounded once
    t = img.half().float()
    for w, b, st in layers:
        t = A.sat_half(F.leaky_relu(F.conv2d(t.float(), w.float(), b.float(), stride=st, padding=1), LEAKY)).float()
    assert A.worst(A.LA.bounded_ratio(t, ref, allow, 1.0))[0] <= 1.0
    t = img.half().float()
    for k, (w, b, st) in enumerate(layers):
        src = F.pad(t.float(), (1, 1, 1, 1), mode="replicate") if k == 2 else F.pad(t.float(), (1, 1, 1, 1))
        t = A.sat_half(F.leaky_relu(F.conv2d(src, w.float(), b.float(), stride=st), LEAKY)).float()
    r, idx, _ = A.worst(A.LA.bounded_ratio(t, ref, allow, 1.0))
    assert r > 1.0 and (idx[2] in (0, ref.shape[2] - 1) or idx[3] in (0, ref.shape[3] - 1))     # at the map's border


def test_saturation_is_required_exactly():
    ref = torch.tensor([70000.0, -1e6, 1.0], dtype=torch.float64)
    s = ref.abs()
    good = torch.tensor([65504.0, -65504.0, 1.0]).half()
    assert A.worst(A.half_ratio(good, ref, s))[0] <= 1.0
    assert A.worst(A.half_ratio(torch.tensor([65472.0, -65504.0, 1.0]).half(), ref, s))[0] == float("inf")
