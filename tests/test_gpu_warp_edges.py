"""The warp family on the lattice, at the border, on the mask threshold and at wild flows (fields and references: tests/warp_cases.py,
held to their conditions by tests/test_warp_cases_cpu.py).

The device states the coordinate, tap and mask arithmetic of PWCDCNet.warp five times (make_taps, make_taps8, the inline copies of
warp_bwd_kernel and warp_corr81_bwd_kernel, window_origin_from).  Every statement is a fixed list of single-rounded float32
operations, so launch_audit.warp_taps decides every mask bit and every tap weight: masks are compared EXACTLY here, on every pixel,
and the warp of a ones tensor bit for bit.  Every test runs all fields of one (shape, configuration); the failures of all fields
are collected and reported together."""
import pytest
import torch
import torch.nn.functional as F

import launch_audit as LA
import warp_cases as WC
from oracle import pwc_oracle as O

pytestmark = pytest.mark.gpu

HALF_EPS = 2.0 ** -11            # one rounding to half precision, relative
REL_GRAD = 1.0e-5                # per element, against the sum of the absolute values of the element's terms


@pytest.fixture(scope="module")
def dev(gpu_device):
    from opticalflow_amd import _lib
    _lib.load()
    return gpu_device


def _cases(shapes):
    return [pytest.param(s, c, id="%s-%s" % (WC.shape_id(s), WC.cfg_id(c))) for s in shapes for c in WC.CONFIGS]


class Failures:
    def __init__(self):
        self.items = []

    def check(self, ok, what, *args):
        if not bool(ok):
            self.items.append(what % args if args else what)

    def bound(self, got, ref, scale, rel, what, extra=None):
        """|got - ref| <= rel * scale (+ extra) on every element; a zero bound demands an exact zero"""
        err = (got.double().cpu() - ref.double()).abs()
        lim = rel * scale.double() + (extra if extra is not None else 0.0)
        bad = ~(err <= lim)
        if bool(bad.any()):
            idx = tuple(int(i) for i in torch.nonzero(bad)[0])
            worst = float((err / lim.clamp_min(1e-300))[bad].max())
            self.items.append("%s: %d elements out of bound, first %s got %.9g ref %.9g bound %.3g (worst ratio %.3g)"
                              % (what, int(bad.sum()), idx, float(got.cpu()[idx]), float(ref[idx]), float(lim[idx]), worst))

    def done(self):
        assert not self.items, "\n".join(self.items)


def _mask_report(got, want, knife):
    bad = torch.nonzero(got != want)
    return "%d pixels differ, first %s (of them on the knife edge: %d)" % (len(bad), bad[:4].tolist(), int((knife & (got != want)).sum()))


def _strided(t, dev, pad_channels=3, offset=0):
    """a copy of t on the device as a batch-strided slice of a larger buffer (arena slice), optionally starting `offset` elements
    into the allocation"""
    B, C, H, W = t.shape
    stride = (C + pad_channels) * H * W
    buf = torch.full((B * stride + offset + 8,), 7.0, dtype=t.dtype, device=dev)
    view = torch.as_strided(buf, (B, C, H, W), (stride, H * W, W, 1), storage_offset=offset)
    view.copy_(t.to(dev))
    return view, buf


def _check_warp_output(f, name, how, out, ones_out, x, t, cfg, rel_half=0.0):
    """out = warp(x), ones_out = warp(ones) from the device against the reference taps t"""
    mask, m32 = t[4], WC.msum32(t)
    knife = WC.knife(t, cfg[2])
    got_ones = ones_out.float().cpu()
    want_ones = m32 if rel_half == 0.0 else m32.half().float()
    gmask = got_ones[:, 0] != 0
    f.check(torch.equal(gmask, mask), "%s %s: mask: %s", name, how, _mask_report(gmask, mask, knife))
    f.check(torch.equal(got_ones, want_ones.unsqueeze(1).expand_as(got_ones)), "%s %s: warp(ones) is not the float32 mask sum bit for bit (%d elements)",
            name, how, int((got_ones != want_ones.unsqueeze(1)).sum()))
    o = out.float().cpu()
    f.check(bool(torch.isfinite(o).all()), "%s %s: non-finite output", name, how)
    f.check(torch.equal(o != 0, mask.unsqueeze(1).expand_as(o)), "%s %s: zero pattern of warp(x), x >= 0.5, is not the mask (%d elements)",
            name, how, int(((o != 0) != mask.unsqueeze(1)).sum()))
    ref, scale = WC.forward(x, t), WC.forward(x.abs(), t)
    f.bound(o, ref, scale, LA.REL_WARP, "%s %s: values" % (name, how), extra=rel_half * ref.abs())


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_WARP))
def test_warp_fp32(dev, shape, cfg):
    """ops.warp, float32, dense and through arena slices (larger batch stride, destination one element into its allocation: the
    scalar-store path also at W % 4 == 0)."""
    from opticalflow_amd import ops
    s, align, thr = cfg
    B, C, H, W = shape
    f = Failures()
    x = WC.positive(shape, 21)
    ones = torch.ones(shape)
    xd, od = x.to(dev), ones.to(dev)
    xs, _ = _strided(x, dev)
    for name in WC.FIELDS:
        flo = WC.field(name, shape, cfg)
        t = WC.field_taps(name, shape, cfg)
        fd = flo.to(dev)
        _check_warp_output(f, name, "dense", ops.warp(xd, fd, s, align, thr), ops.warp(od, fd, s, align, thr), x, t, cfg)
        fs, _ = _strided(flo, dev, pad_channels=1)
        out, obuf = _strided(torch.zeros(shape), dev, pad_channels=2, offset=1)
        ones_out, _ = _strided(torch.zeros(shape), dev, pad_channels=2, offset=1)
        ops.warp(xs, fs, s, align, thr, out=out)
        ops.warp(od, fs, s, align, thr, out=ones_out)
        _check_warp_output(f, name, "strided", out, ones_out, x, t, cfg)
        stride = (C + 2) * H * W
        gaps = torch.cat([obuf[:1]] + [obuf[1 + b * stride + C * H * W: 1 + (b + 1) * stride] for b in range(B - 1)]
                         + [obuf[1 + (B - 1) * stride + C * H * W:]])                 # before, between and after the images, to the buffer's end
        f.check(bool((gaps == 7.0).all()), "%s strided: the warp wrote outside its destination", name)
        if name == "zero" and align:
            # the identity: every pixel kept, and the output is x up to the float32 rounding of the sample coordinate itself
            # (|ix - x| = dev <= 1e-5, tests/test_warp_cases_cpu.py), which moves dev of the weight to a neighbouring tap
            ix, iy = WC.sample_coords(t)
            devi = max(float((ix - ix.round()).abs().max()), float((iy - iy.round()).abs().max()))
            o = ops.warp(xd, fd, s, align, thr).cpu()
            f.check(bool(t[4].all()) and bool((o != 0).all()), "zero: align_corners does not keep every pixel")
            f.bound(o, x, torch.full_like(x, 4 * 1.5), devi, "zero: identity", extra=LA.REL_WARP * x.abs())
    f.done()


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_WARP))
def test_warp_fp16_storage(dev, shape, cfg):
    """ops.warp on half tensors: the coordinates are float32 in the kernel -- the same masks, exactly; values within one
    half-precision rounding of forward() on the half inputs.  The flow is the field built FOR half storage (steered over halves,
    field(half=True)): rounding the float32 field would move every sample point by up to 2^-11 of its flow and leave nothing on the
    border or the threshold.  What a half flow can still hold is asserted in tests/test_warp_cases_cpu.py: with align_corners both
    sides of the threshold and all four border classes; without it (a flow of x / (W - 1) px is needed to reach the border, which a
    half does not resolve to 1e-4 px) nothing within reach of the threshold -- there only level_entry, whose flow chain is float32,
    puts make_taps8 on the knife edge."""
    from opticalflow_amd import ops
    s, align, thr = cfg
    f = Failures()
    x = WC.positive(shape, 22).half()
    ones = torch.ones(shape).half()
    for name in WC.FIELDS:
        flo = WC.field(name, shape, cfg, half=True).half()
        t = WC.taps(flo.float(), cfg)
        fd = flo.to(dev)
        _check_warp_output(f, name, "fp16", ops.warp(x.to(dev), fd, s, align, thr), ops.warp(ones.to(dev), fd, s, align, thr), x.float(), t, cfg,
                           rel_half=HALF_EPS)
    f.done()


def _to_c8(x):
    """[B,C,H,W] float -> [B,ceil(C/8),H,W,8] half on the CPU, zero channel padding, no saturation (Inf and NaN pass)"""
    B, C, H, W = x.shape
    g = (C + 7) // 8
    p = torch.zeros(B, g * 8, H, W, dtype=torch.float16)
    p[:, :C] = x.half()
    return p.view(B, g, 8, H, W).permute(0, 1, 3, 4, 2).contiguous()


def _from_c8(x, C):
    B, g, H, W, _ = x.shape
    return x.permute(0, 1, 4, 2, 3).reshape(B, g * 8, H, W)[:, :C].float()


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_C8))
def test_warp_c8(dev, shape, cfg):
    """ops_f16.warp_c8: make_taps8, the second statement of the taps, under the requirements of fp16 storage.  The c8 operands are
    laid out on the CPU, so +-Inf and NaN reach the kernel as they are.  The flow group is half: the fields are those built for half
    storage (see test_warp_fp16_storage for what they hold)."""
    from opticalflow_amd import ops_f16 as F16
    s, align, thr = cfg
    B, C, H, W = shape
    f = Failures()
    x = WC.positive(shape, 23).half().float()
    xd, od = _to_c8(x).to(dev), _to_c8(torch.ones(shape)).to(dev)
    for name in WC.FIELDS:
        flo = WC.field(name, shape, cfg, half=True).half()
        t = WC.taps(flo.float(), cfg)
        group = torch.zeros(B, 8, H, W)
        group[:, 2:4] = flo.float()                                      # (u, v) at channels 2, 3 of the group
        gd = _to_c8(group).to(dev)
        out = _from_c8(F16.warp_c8(xd, gd, C, flo_channel=2, flow_scale=s, align_corners=align, mask_threshold=thr).cpu(), C)
        ones_out = _from_c8(F16.warp_c8(od, gd, C, flo_channel=2, flow_scale=s, align_corners=align, mask_threshold=thr).cpu(), C)
        _check_warp_output(f, name, "c8", out, ones_out, x, t, cfg, rel_half=HALF_EPS)
    f.done()


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_ENTRY))
def test_level_entry_identity_deconvolution(dev, shape, cfg):
    """ops_f16.level_entry and level_entry_correlation with a deconvolution whose filter is the identity phase: the up-flow IS the
    constructed field (weights 0 / 1, bias 0 -- asserted on the CPU against conv_transpose2d and on the device by reading back the
    flow group), so the fields reach make_taps8 through the fp32 flow chain unrounded."""
    from opticalflow_amd import ops_f16 as F16
    s, align, thr = cfg
    B, C, H, W = shape
    g = (C + 7) // 8
    f = Failures()
    x = WC.positive(shape, 24).half().float()
    c1 = WC.signed(shape, 25).half().float()
    c1d, xd, od = _to_c8(c1).to(dev), _to_c8(x).to(dev), _to_c8(torch.ones(shape)).to(dev)
    dw, db = WC.identity_deconv()
    featp = torch.zeros(B, 1, H // 2, W // 2, 8, device=dev)
    for name in WC.FIELDS:
        low, up = WC.entry_flow(name, shape, cfg)
        assert torch.equal(F.conv_transpose2d(low, dw, db, stride=2, padding=1), up)
        t = WC.taps(up, cfg)
        head = torch.zeros(B, 1, H // 2, W // 2, 8)
        head[:, 0, :, :, 0:2] = low.permute(0, 2, 3, 1)
        head[:, 0, :, :, 2:] = 99.0                                      # must be ignored
        head = head.to(dev)
        outs = []
        for src in (xd, od):
            c1_dst = torch.zeros_like(c1d)
            fg = torch.zeros(B, 1, H, W, 8, dtype=torch.float16, device=dev)
            warped = torch.zeros_like(xd)
            F16.level_entry(c1d, src, head, featp, dw.to(dev), db.to(dev), C, c1_dst=c1_dst, flow_group=fg, out=warped,
                            flow_scale=s, align_corners=align, mask_threshold=thr)
            outs.append(_from_c8(warped.cpu(), C))
            got_up = fg[:, 0, :, :, 0:2].cpu().permute(0, 3, 1, 2).float()
            f.check(torch.equal(got_up, up.clamp(-65504.0, 65504.0).half().float()), "%s: the flow group is not the field (saturated, rounded to half)", name)
            f.check(torch.equal(c1_dst, c1d), "%s: c1 copy", name)
        _check_warp_output(f, name, "entry", outs[0], outs[1], x, t, cfg, rel_half=HALF_EPS)
        # the fused level entry + cost volume (level_corr81_c8_kernel's own call of make_taps8): bit-identical to the two calls
        c1_dst = torch.zeros_like(c1d)
        fg = torch.zeros(B, 1, H, W, 8, dtype=torch.float16, device=dev)
        one = torch.zeros(B, 11, H, W, 8, dtype=torch.float16, device=dev)
        F16.level_entry_correlation(c1d, xd, head, featp, dw.to(dev), db.to(dev), C, c1_dst=c1_dst, flow_group=fg, out=one,
                                    flow_scale=s, align_corners=align, mask_threshold=thr, leaky_slope=0.1)
        two = F16.correlation_c8(c1d, _to_c8(outs[0]).to(dev), C, leaky_slope=0.1)
        f.check(bool(torch.isfinite(two).all()), "%s: non-finite cost volume", name)
        f.check(torch.equal(one, two), "%s: level_entry_correlation differs from level_entry + correlation_c8 in %d elements", name, int((one != two).sum()))
    f.done()


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_WARP))
def test_warp_backward(dev, shape, cfg):
    """ops.warp_backward, fixed-point and float atomics: grad_flo and grad_x within 1e-5 of grads() per element against the sum of
    absolute values, on EVERY pixel -- lattice, border and threshold pixels included, nothing masked out of the comparison.  Masked
    and wild pixels have exactly zero grad_flo and scatter nothing (their bound is zero).

    The fixed-point path adds one term to the bound of grad_x, derived from its number format: a contribution g * w is rounded to
    an integer multiple of 2^(e - 40), e = floor(log2 max|grad_out|), i.e. by at most 2^(e - 41) <= 2^-41 max|grad_out|, whatever
    its own size -- an element that only receives weights of 2^-23 (a sample point one ulp inside the border) has a sum of absolute
    values of that order, against which 1e-5 is below the format's step.  n contributions: n * 2^-41 * max|grad_out|."""
    from opticalflow_amd import ops
    s, align, thr = cfg
    f = Failures()
    x = WC.signed(shape, 31)
    go = WC.signed(shape, 32)
    xd, gd = x.to(dev), go.to(dev)
    gmax = float(go.abs().max())
    for name in WC.FIELDS:
        flo = WC.field(name, shape, cfg)
        t = WC.field_taps(name, shape, cfg)
        fd = flo.to(dev)
        rx, rf, sx, sf = WC.grads(x, t, go, cfg)
        live = (t[0], t[1], [(w != 0).float() for w in t[2]], t[3], t[4], t[5])
        count = WC.grads(x, live, torch.ones_like(go), cfg)[2]                       # contributions per element of grad_x
        gx, gf = ops.warp_backward(xd, fd, gd, s, align, thr, deterministic=True)
        f.check(bool(torch.isfinite(gx).all() and torch.isfinite(gf).all()), "%s fixed: non-finite gradient", name)
        f.bound(gf, rf, sf, REL_GRAD, "%s fixed: grad_flo" % name)
        f.bound(gx, rx, sx, REL_GRAD, "%s fixed: grad_x" % name, extra=count * 2.0 ** -41 * gmax)
        hx, hf = ops.warp_backward(xd, fd, gd, s, align, thr, deterministic=True)
        f.check(torch.equal(gx, hx) and torch.equal(gf, hf), "%s fixed: not bit-identical on a second run", name)
        ax, af = ops.warp_backward(xd, fd, gd, s, align, thr, deterministic=False)
        f.bound(af, rf, sf, REL_GRAD, "%s atomics: grad_flo" % name)
        f.bound(ax, rx, sx, REL_GRAD, "%s atomics: grad_x" % name)
        f.check(torch.equal(af, gf), "%s: grad_flo differs between the two paths", name)
        dead = (~t[4]).unsqueeze(1).expand_as(rf)
        f.check(not bool(gf.cpu()[dead].any()) and not bool(af.cpu()[dead].any()), "%s: a masked pixel has a non-zero grad_flo", name)
        if name == "converge":                                                      # hundreds of contributions on one element
            f.check(int(count.max()) >= min(100, shape[2] * shape[3] // 2), "converge: only %d contributions", int(count.max()))
            f.bound(ax, gx.double().cpu(), sx, REL_GRAD, "converge: the two paths' grad_x", extra=count * 2.0 ** -41 * gmax)
    f.done()


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_FUSED))
def test_warp_correlation_fused_forward(dev, request, shape, cfg):
    """ops.warp_correlation under every value of warpcorr_window and once with corr_pipe on (corr_small_tiles 0): torch.equal to
    ops.correlation(c1, ops.warp(c2, flo)) on every field -- wild flows and the tile_centre fields, which put wild, far and
    threshold values on the pixel that places the LDS window, included -- and within REL_CORR of the float64 cost volume of
    forward().  Which kernel ran cannot be observed: the library reports no route for this entry.  By its dispatch
    (pwc_corr.hip, warp_corr81_pipe_fits) 32 channels take the window kernel unless warpcorr_window is 0, 13 and 8 channels the
    round-2 kernel under every value; the test runs all values and asserts none.  corr_pipe selects the kernel of the PLAIN
    correlation, not of the fused entry: under it the two-kernel result is computed again and must not change (at these tile
    counts corr_pipe_min_tiles keeps it on the same kernel; the pass pins that the option does not leak into the fused one)."""
    from opticalflow_amd import ops, _lib
    s, align, thr = cfg
    B, C, H, W = shape
    f = Failures()
    saved = {k: _lib.get_option(k) for k in ("corr_small_tiles", "warpcorr_window", "corr_pipe")}
    request.addfinalizer(lambda: [_lib.set_option(k, v) for k, v in saved.items()])
    _lib.set_option("corr_small_tiles", 0)
    c1, c2 = WC.signed(shape, 41), WC.signed(shape, 42)
    c1d, c2d = c1.to(dev), c2.to(dev)
    for name in WC.FIELDS_FUSED:
        flo = WC.field(name, shape, cfg)
        t = WC.field_taps(name, shape, cfg)
        fd = flo.to(dev)
        _lib.set_option("warpcorr_window", saved["warpcorr_window"])
        _lib.set_option("corr_pipe", saved["corr_pipe"])
        warped = ops.warp(c2d, fd, s, align, thr)
        two = ops.correlation(c1d, warped, 4, 1, 4, 1, 1, 1.0, leaky_slope=0.1)
        f.check(bool(torch.isfinite(two).all()), "%s: the two-kernel cost volume of finite features is not finite", name)
        w2, w2a = WC.forward(c2, t), WC.forward(c2.abs(), t)
        ref, _ = LA.corr_ref(c1, w2, False, True)
        _, sc = LA.corr_ref(c1.abs(), w2a, False, False)
        f.bound(two, ref, sc, LA.REL_CORR, "%s two kernels: cost volume" % name)
        for mode, pipe in ((0, 0), (1, 0), (2, 0), (saved["warpcorr_window"], 1)):
            _lib.set_option("warpcorr_window", mode)
            _lib.set_option("corr_pipe", pipe)
            assert _lib.get_option("warpcorr_window") == mode
            how = "warpcorr_window %d corr_pipe %d" % (mode, pipe)
            if pipe:
                again = ops.correlation(c1d, ops.warp(c2d, fd, s, align, thr), 4, 1, 4, 1, 1, 1.0, leaky_slope=0.1)
                f.check(torch.equal(again, two), "%s %s: warp + correlation changed in %d elements", name, how, int((again != two).sum()))
            got = ops.warp_correlation(c1d, c2d, fd, s, align, thr, leaky_slope=0.1)
            f.check(got is not None, "%s %s: the fused entry declined", name, how)
            if got is None:
                continue
            f.check(torch.equal(got, two), "%s %s: differs from warp + correlation in %d elements (non-finite: %d)", name, how,
                    int((got != two).sum()), int((~torch.isfinite(got)).sum()))
            f.bound(got, ref, sc, LA.REL_CORR, "%s %s: cost volume" % (name, how))
    # a width the fused entry declines: nothing launched, the caller takes the two operators
    odd = (B, C, H, W - 1)
    assert ops.warp_correlation(c1d[..., :-1].contiguous(), c2d[..., :-1].contiguous(), torch.zeros(B, 2, H, W - 1, device=dev)) is None, odd
    f.done()


def _fused_reference(c1, c2, t, gy, y_gpu, cfg):
    """float64 gradients of leaky(corr(c1, w2)), w2 = warp(c2): autograd through corr_ref's correlation for the cost volume (the
    LeakyReLU branch of each element from the kernel's own forward output, as the kernel takes it), grads() for the warp step.
    Beside each the same sums over absolute values."""
    w2 = WC.forward(c2, t)
    a = c1.double().requires_grad_(True)
    w = w2.clone().requires_grad_(True)
    xv = O.correlation(a, w, 4, 1, 4, 1, 1, 1)
    pos = y_gpu.cpu() > 0
    torch.where(pos, xv, 0.1 * xv).backward(gy.double())
    g1, gw2 = a.grad, w.grad
    aa = c1.double().abs().requires_grad_(True)
    wa = WC.forward(c2.abs(), t).requires_grad_(True)
    xa = O.correlation(aa, wa, 4, 1, 4, 1, 1, 1)
    torch.where(pos, xa, 0.1 * xa).backward(gy.double().abs())
    s1, sw2 = aa.grad, wa.grad
    g2, gf, _, _ = WC.grads(c2, t, gw2, cfg)
    _, _, s2, sf = WC.grads(c2, t, sw2, cfg)
    return (g1, g2, gf), (s1, s2, sf)


@pytest.mark.parametrize("shape,cfg", _cases(WC.SHAPES_FUSED))
def test_warp_correlation_fused_backward(dev, shape, cfg):
    """ops.warp_correlation_backward, fused and as the composition: the three gradients within 1e-5 per element (against the sums
    of absolute values carried through the correlation and the warp) of float64 autograd through the cost volume with grads() for
    the warp step, on the fields AS BUILT -- no pixel moved away from a tap boundary or the threshold.  fused=True is bit-identical
    on a second run.

    grad_c2 is a fixed-point scatter in both forms; its format adds, as in test_warp_backward, n contributions times half a step:
    the fused kernel's step is 2^(e - 39) with e = floor(log2 M), M = 81 max|grad_y| max|c1| (pwc_warp_corr_bwd.hip), the
    composition's 2^(e' - 40) with e' = floor(log2 max|gw2|) <= e."""
    from opticalflow_amd import ops
    s, align, thr = cfg
    f = Failures()
    c1, c2 = WC.signed(shape, 51), WC.signed(shape, 52)
    B, C, H, W = shape
    gy = WC.signed((B, 81, H, W), 53)
    c1d, c2d, gyd = c1.to(dev), c2.to(dev), gy.to(dev)
    M = 81.0 * float(gy.abs().max()) * float(c1.abs().max())
    for name in WC.FIELDS_FUSED:
        flo = WC.field(name, shape, cfg)
        t = WC.field_taps(name, shape, cfg)
        fd = flo.to(dev)
        y = ops.correlation(c1d, ops.warp(c2d, fd, s, align, thr), 4, 1, 4, 1, 1, 1.0, leaky_slope=0.1)
        (r1, r2, rf), (s1, s2, sf) = _fused_reference(c1, c2, t, gy, y, cfg)
        live = (t[0], t[1], [(w != 0).float() for w in t[2]], t[3], t[4], t[5])
        count = WC.grads(c2, live, torch.ones_like(c2), cfg)[2]
        for fused in (True, False):
            how = "fused" if fused else "composition"
            g1, g2, gf = ops.warp_correlation_backward(c1d, c2d, fd, y, gyd, s, align, thr, 1.0, False, 0.1, fused=fused)
            f.check(all(bool(torch.isfinite(g).all()) for g in (g1, g2, gf)), "%s %s: non-finite gradient", name, how)
            f.bound(g1, r1, s1, REL_GRAD, "%s %s: grad_c1" % (name, how))
            f.bound(g2, r2, s2, REL_GRAD, "%s %s: grad_c2" % (name, how), extra=count * 2.0 ** -40 * M)
            f.bound(gf, rf, sf, REL_GRAD, "%s %s: grad_flo" % (name, how))
            if fused:
                h1, h2, hf = ops.warp_correlation_backward(c1d, c2d, fd, y, gyd, s, align, thr, 1.0, False, 0.1, fused=True)
                f.check(torch.equal(g1, h1) and torch.equal(g2, h2) and torch.equal(gf, hf), "%s fused: not bit-identical on a second run", name)
    f.done()
