"""Training path: pwc_warp_corr81_bwd (fused warp + correlation + LeakyReLU backward), ops.WarpCorrelationFunction and
PWCDCNet(trainable=True), against autograd of the CPU oracle in float64 (oracle.warp / correlation / leaky_relu, pwc_forward)."""
import pytest
import torch

from conftest import seeded_rand
from oracle import pwc_oracle as O

pytestmark = pytest.mark.gpu

THR_DC, THR_OLD = 0.9999, 0.999


@pytest.fixture(scope="module")
def dev(gpu_device):
    from opticalflow_amd import _lib
    _lib.load()
    return gpu_device


def _smooth_flow(B, H, W, seed, amp):
    """Low-frequency flow: a bilinear upsampling of a 4x4-cell random field."""
    coarse = seeded_rand((B, 2, max(2, H // 8), max(2, W // 8)), seed, -amp, amp)
    return torch.nn.functional.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).contiguous()


def _rough_flow(B, H, W, seed):
    """tools/bench_warpcorr.py's rough flow: independent 3-px noise per 8-px cell on top of a smooth field."""
    cells = seeded_rand((B, 2, (H + 7) // 8, (W + 7) // 8), seed, -3.0, 3.0)
    noise = cells.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :H, :W]
    return (_smooth_flow(B, H, W, seed + 1, 2.0) + noise).contiguous()


def _away_from_edges(flo, scale, align, thr):
    """Move the few pixels whose sample coordinate sits within 1e-4 of a tap boundary (the bilinear gradient jumps there, and
    fp32 and fp64 may pick different cells) or whose mask sum sits within 1e-5 of the threshold by a small flow offset."""
    B, _, H, W = flo.shape
    f = flo.clone()
    for _ in range(4):
        u = torch.arange(W, dtype=torch.float64).view(1, 1, W) + f[:, 0].double() * scale
        v = torch.arange(H, dtype=torch.float64).view(1, H, 1) + f[:, 1].double() * scale
        if align:
            ix, iy = u, v
        else:
            ix, iy = u * W / max(W - 1, 1) - 0.5, v * H / max(H - 1, 1) - 0.5
        near = lambda t: (t - t.round()).abs() < 1e-4                         # noqa: E731
        wx = torch.where((ix >= 0) & (ix <= W - 1), torch.ones_like(ix), 1 - (ix - ix.clamp(0, W - 1)).abs()).clamp(0, 1)
        wy = torch.where((iy >= 0) & (iy <= H - 1), torch.ones_like(iy), 1 - (iy - iy.clamp(0, H - 1)).abs()).clamp(0, 1)
        bad = near(ix) | near(iy) | ((wx * wy - thr).abs() < 1e-5)
        if not bool(bad.any()):
            break
        f[:, 0][bad] += 3e-3 / scale
        f[:, 1][bad] += 2e-3 / scale
    return f


def _oracle_grads(c1, c2, flo, gy, y_gpu, scale, align, thr, normalize):
    """float64 autograd of leaky(corr(c1, warp(c2, scale * flo))); the LeakyReLU branch of each element is taken from the
    kernel's own forward output (ties at x == 0 are rounding noise, not semantics)."""
    a = c1.double().requires_grad_(True)
    b = c2.double().requires_grad_(True)
    f = flo.double().requires_grad_(True) if flo is not None else None
    w = O.warp(b, f * scale, align_corners=align, mask_threshold=thr) if f is not None else b
    x = O.correlation(a, w, 4, 1, 4, 1, 1, 1, normalize=normalize)
    y = torch.where(y_gpu.cpu() > 0, x, 0.1 * x)
    y.backward(gy.double())
    return a.grad, b.grad, (f.grad if f is not None else None)


def _close(got, ref, rel, what):
    err = (got.double().cpu() - ref).abs().max().item()
    bound = rel * ref.abs().max().item()
    assert err <= bound, "%s: max err %.3e > %.3e (max|ref| %.3e)" % (what, err, bound, ref.abs().max().item())


CASES = [
    # (shape, flow kind, scale, align_corners, normalize, mask threshold)
    ((2, 32, 56, 128), "smooth", 5.0, False, False, THR_DC),
    ((2, 32, 56, 128), "rough", 5.0, True, True, THR_OLD),
    ((2, 32, 56, 128), "oob", 2.5, False, True, THR_DC),
    ((1, 16, 7, 9), "smooth", 1.25, True, False, THR_OLD),
    ((1, 16, 7, 9), "rough", 0.625, False, True, THR_DC),
    ((2, 8, 20, 30), "rough", 2.5, False, False, THR_DC),        # W % 4 != 0: the forward takes warp + correlation
    ((1, 16, 7, 9), None, 1.0, False, False, THR_DC),           # flo = None: level 6
    ((2, 32, 24, 64), None, 1.0, False, True, THR_DC),
]


def _inputs(shape, kind, scale, align, thr, seed):
    B, C, H, W = shape
    c1 = seeded_rand(shape, seed, -1, 1)
    c2 = seeded_rand(shape, seed + 1, -1, 1)
    gy = seeded_rand((B, 81, H, W), seed + 2, -1, 1)
    flo = None
    if kind == "smooth":
        flo = _smooth_flow(B, H, W, seed + 3, 4.0 / scale)
    elif kind == "rough":
        flo = _rough_flow(B, H, W, seed + 3) / scale
    elif kind == "oob":                                         # large flows: many samples leave the image (mask 0 there)
        flo = _smooth_flow(B, H, W, seed + 3, 0.8 * W / scale)
    if flo is not None:
        flo = _away_from_edges(flo, scale, align, thr)
    return c1, c2, flo, gy


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-s%g-a%d-n%d-t%g" % ("x".join(map(str, c[0])), c[1], c[2], c[3], c[4], c[5]))
def test_fused_backward_matches_oracle_autograd(dev, case):
    from opticalflow_amd import ops
    shape, kind, scale, align, normalize, thr = case
    c1, c2, flo, gy = _inputs(shape, kind, scale, align, thr, 300)
    d = [t.to(dev) if t is not None else None for t in (c1, c2, flo, gy)]
    y = ops.WarpCorrelationFunction.apply(d[0], d[1], d[2], scale, align, thr, 1.0, normalize, 0.1)
    g1, g2, gf = ops.warp_correlation_backward(d[0], d[1], d[2], y, d[3], scale, align, thr, 1.0, normalize, 0.1)
    r1, r2, rf = _oracle_grads(c1, c2, flo, gy, y, scale, align, thr, normalize)
    _close(g1, r1, 1e-5, "grad_c1")
    _close(g2, r2, 1e-5, "grad_c2")
    if flo is None:
        assert gf is None
    else:
        _close(gf, rf, 1e-5, "grad_flo")
    # bit-reproducible, and the composition it replaces (warp_fwd -> mask -> corr_bwd -> warp_bwd) agrees
    h1, h2, hf = ops.warp_correlation_backward(d[0], d[1], d[2], y, d[3], scale, align, thr, 1.0, normalize, 0.1)
    assert torch.equal(g1, h1) and torch.equal(g2, h2) and (gf is None or torch.equal(gf, hf))
    k1, k2, kf = ops.warp_correlation_backward(d[0], d[1], d[2], y, d[3], scale, align, thr, 1.0, normalize, 0.1, fused=False)
    _close(g1, k1.double().cpu(), 1e-6, "grad_c1 vs composition")
    _close(g2, k2.double().cpu(), 1e-6, "grad_c2 vs composition")
    if gf is not None:
        _close(gf, kf.double().cpu(), 1e-6, "grad_flo vs composition")


def test_fused_backward_unsplit_launch_matches_composition(dev):
    """A launch of >= 1024 tiles keeps all channel chunks in one workgroup (smaller ones spread them over grid.y, the cases
    above): same gradients as the composition of the existing operators, bit-reproducible."""
    from opticalflow_amd import ops
    c1, c2, flo, gy = (t.to(dev) for t in _inputs((4, 32, 128, 512), "rough", 5.0, False, THR_DC, 600))
    y = ops.WarpCorrelationFunction.apply(c1, c2, flo, 5.0, False, THR_DC, 1.0, True, 0.1)
    g = ops.warp_correlation_backward(c1, c2, flo, y, gy, 5.0, False, THR_DC, 1.0, True, 0.1)
    h = ops.warp_correlation_backward(c1, c2, flo, y, gy, 5.0, False, THR_DC, 1.0, True, 0.1)
    k = ops.warp_correlation_backward(c1, c2, flo, y, gy, 5.0, False, THR_DC, 1.0, True, 0.1, fused=False)
    for a, b, r, n in zip(g, h, k, ("grad_c1", "grad_c2", "grad_flo")):
        assert torch.equal(a, b), n
        _close(a, r.double().cpu(), 1e-6, n + " vs composition")


def test_autograd_function_gradients_and_non_finite_fallback(dev):
    """WarpCorrelationFunction through torch.autograd.grad, and a non-finite upstream gradient: no fixed-point form, the call
    falls back to float atomics for grad_c2 and the Inf / NaN stay where they belong (image 0 only)."""
    from opticalflow_amd import ops
    c1, c2, flo, gy = _inputs((2, 32, 24, 64), "smooth", 2.5, False, THR_DC, 400)
    a, b, f = (t.to(dev).requires_grad_(True) for t in (c1, c2, flo))
    y = ops.WarpCorrelationFunction.apply(a, b, f, 2.5, False, THR_DC, 1.0, True, 0.1)
    ga, gb, gf = torch.autograd.grad(y, (a, b, f), gy.to(dev))
    r1, r2, rf = _oracle_grads(c1, c2, flo, gy, y.detach(), 2.5, False, THR_DC, True)
    _close(ga, r1, 1e-5, "grad_c1")
    _close(gb, r2, 1e-5, "grad_c2")
    _close(gf, rf, 1e-5, "grad_flo")
    gi = gy.to(dev).clone()
    gi[0, 40, 10, 20] = float("inf")
    h1, h2, hf = ops.warp_correlation_backward(a.detach(), b.detach(), f.detach(), y.detach(), gi, 2.5, False, THR_DC, 1.0, True, 0.1)
    assert not bool(torch.isfinite(h2[0]).all()) and bool(torch.isfinite(h2[1]).all())
    assert bool(torch.isfinite(h1[1]).all()) and bool(torch.isfinite(hf[1]).all())
    # the float-atomic mode still computes the finite image right (its upstream gradient there is gy's)
    _close(h1[1], r1[1], 1e-5, "grad_c1, finite image, float-atomic mode")
    _close(h2[1], r2[1], 1e-5, "grad_c2, finite image, float-atomic mode")
    _close(hf[1], rf[1], 1e-5, "grad_flo, finite image, float-atomic mode")
    z1, z2, zf = ops.warp_correlation_backward(a.detach(), b.detach(), f.detach(), y.detach(), torch.zeros_like(gi), 2.5, False,
                                               THR_DC, 1.0, True, 0.1)
    assert not bool(z1.any()) and not bool(z2.any()) and not bool(zf.any())


def _net(cls, dev, seed=0):
    from opticalflow_amd.weights import synthetic_state_dict
    net = cls(trainable=True)
    sd = synthetic_state_dict(net.manifest(), seed=seed, gain=0.85, bias_std=0.02)
    net.load_state_dict(sd)
    return net.to(dev).train(), sd


LEVEL_W = (1.0, 0.5, 0.25, 0.125, 0.0625)


@pytest.mark.parametrize("variant", ["dc", "old"])
@pytest.mark.parametrize("shape", [(1, 6, 64, 64), (2, 6, 128, 192)])
def test_trainable_network_gradients_match_oracle(dev, variant, shape):
    from opticalflow_amd import PWCDCNet, PWCDCNet_old
    cls, fwd = (PWCDCNet, O.pwc_forward) if variant == "dc" else (PWCDCNet_old, O.pwc_forward_old)
    net, sd = _net(cls, dev)
    x = seeded_rand(shape, 500)
    xd = x.to(dev).requires_grad_(True)
    flows = net(xd)
    assert isinstance(flows, tuple) and len(flows) == 5 and all(f.requires_grad for f in flows)
    with torch.no_grad():                                        # the inference plan's training-mode tuple
        plan_flows = net(x.to(dev))
    for got, ref in zip(flows, plan_flows):
        assert O.epe(got.detach().cpu(), ref.cpu()) < 1e-5
    loss = sum(w * f.abs().mean() for w, f in zip(LEVEL_W, flows))
    loss.backward()

    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    ref = fwd(sd64, x64, all_levels=True)
    sum(w * f.abs().mean() for w, f in zip(LEVEL_W, ref)).backward()
    _close(xd.grad, x64.grad, 1e-3, "x.grad")
    named = dict(net.named_parameters())
    checked = 0
    for k, p in named.items():
        r = sd64[k].grad
        if r is None:                                            # deconv2 is never used (PWCNet.py:124)
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        _close(p.grad, r, 1e-3, k)
        checked += 1
    assert checked >= len(named) - 2


def test_autocast_forward_backward_finite(dev):
    from opticalflow_amd import PWCDCNet
    net, _ = _net(PWCDCNet, dev)
    x = seeded_rand((2, 6, 64, 128), 510).to(dev)
    with torch.autocast("cuda", torch.float16):
        flows = net(x)
        loss = sum(w * f.float().abs().mean() for w, f in zip(LEVEL_W, flows))
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert len(grads) > 100 and all(bool(torch.isfinite(g).all()) for g in grads)


def test_training_loop_lowers_loss_and_eval_sees_new_weights(dev):
    from opticalflow_amd import PWCDCNet
    net, _ = _net(PWCDCNet, dev)
    x = seeded_rand((1, 6, 64, 128), 520).to(dev)
    target = seeded_rand((1, 2, 16, 32), 521, -1, 1).to(dev)
    net.eval()
    before = net(x)                                              # builds an inference plan with the initial weights
    net.train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    losses = []
    for _ in range(5):
        opt.zero_grad()
        flow2 = net(x)[0]
        loss = (flow2 - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    net.eval()
    after = net(x)
    assert not torch.equal(after, before)                        # the plan was rebuilt from the updated parameters
    fresh = PWCDCNet()
    fresh.load_state_dict(net.state_dict())
    assert torch.equal(after, fresh.to(dev).eval()(x))


def test_trainable_off_paths_unchanged(dev):
    """trainable=True changes nothing outside training-mode grad calls; fp16 precision refuses to train."""
    import warnings
    from opticalflow_amd import PWCDCNet
    net, sd = _net(PWCDCNet, dev)
    x = seeded_rand((1, 6, 64, 64), 530).to(dev)
    with torch.no_grad():
        a = net(x)
    assert len(a) == 5 and not a[0].requires_grad
    ref = PWCDCNet()
    ref.load_state_dict(sd)
    ref = ref.to(dev).eval()
    assert torch.equal(net.eval()(x), ref(x))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = net.train()(x)
    assert out[0].requires_grad and not any("inference-only" in str(m.message) for m in w)
    n16 = PWCDCNet(precision="fp16", trainable=True)
    n16.load_state_dict(sd)
    with pytest.raises(NotImplementedError):
        n16.to(dev).train()(x)


# ---- per-element bounds at the network's own channel counts and launch splits --------------------------------------------------
# per element, against the same gradient computed from |c1|, |c2|, |gy| and |slope|: the a-priori bound n x 2^-24 of a float32 sum
# of n terms, n ~ 90 (81 displacements + the four-tap blend + the scatter)
REL_BWD = 6e-6


def _taps_grads(c1, c2, flo, gy, y_gpu, scale, align, thr, normalize, absolute=False):
    """float64 autograd of leaky(corr(c1, warp(c2))) whose tap cells, weights and mask come from the kernel's float32 sample
    coordinates (launch_audit.warp_taps): the backward is discontinuous at cell boundaries, where float64 coordinates could send a
    gradient to a different cell.  Returns (grad_c1, grad_c2, grad_flo); grad_flo = sum_c gw2 d w2 / d(ix, iy) d(ix, iy) / d flo
    with the bilinear factors of the same float32 taps.  absolute: everything on |c1|, |c2|, |gy| with |slope| and |d w2 / d ix|
    -- the sum of |terms| of each gradient."""
    import launch_audit as LA
    f = (lambda t: t.double().abs()) if absolute else (lambda t: t.double())
    a, b = f(c1).requires_grad_(True), f(c2).requires_grad_(True)
    taps = LA.warp_taps(flo, scale, align, thr) if flo is not None else None
    w = LA.warp_apply(b, taps) if flo is not None else b
    if flo is not None:
        w.retain_grad()
    x = O.correlation(a, w, 4, 1, 4, 1, 1, 1, normalize=normalize)
    y = torch.where(y_gpu.cpu() > 0, x, 0.1 * x)
    y.backward(f(gy))
    if flo is None:
        return a.grad, b.grad, None
    x0, y0, _, _, mask, (ax1, ay1, ok) = taps
    B, C, H, W = c2.shape
    flat = b.detach().reshape(B, C, H * W)
    v = []
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        idx = ((y0 + dy).clamp(0, H - 1) * W + (x0 + dx).clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
        v.append(torch.gather(flat, 2, idx).reshape(B, C, H, W) * (ok[k] & mask).double().unsqueeze(1))
    ax1, ay1 = ax1.double().unsqueeze(1), ay1.double().unsqueeze(1)
    sgn = (lambda t: t.abs()) if absolute else (lambda t: t)
    if absolute:
        dix = (1 - ay1) * (v[1] + v[0]) + ay1 * (v[3] + v[2])
        diy = (1 - ax1) * (v[2] + v[0]) + ax1 * (v[3] + v[1])
    else:
        dix = (1 - ay1) * (v[1] - v[0]) + ay1 * (v[3] - v[2])
        diy = (1 - ax1) * (v[2] - v[0]) + ax1 * (v[3] - v[1])
    fx = 1.0 if align else W / max(W - 1, 1)
    fy = 1.0 if align else H / max(H - 1, 1)
    gw = sgn(w.grad)
    sc = abs(scale) if absolute else scale
    gf = torch.stack(((gw * dix).sum(1) * fx * sc, (gw * diy).sum(1) * fy * sc), 1)
    return a.grad, b.grad, gf


def _contributions(flo, scale, align, thr):
    """per source element of c2: how many (pixel, tap) pairs of the scatter add into it (same count for every channel)"""
    import launch_audit as LA
    x0, y0, w = LA.warp_taps(flo, scale, align, thr)[:3]
    B, _, H, W = flo.shape
    n = torch.zeros(B, H * W, dtype=torch.float64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        idx = ((y0 + dy).clamp(0, H - 1) * W + (x0 + dx).clamp(0, W - 1)).reshape(B, -1)
        n.scatter_add_(1, idx, (w[k] != 0).double().reshape(B, -1))
    return n.view(B, 1, H, W)


def _check_per_element(c1, c2, flo, gy, y, g1, g2, gf, scale, align, thr, normalize, what, images=None):
    """grad_c1, grad_c2 and grad_flo per element against the float64 gradients of _taps_grads (REL_BWD x sum of |terms|; grad_c2 also
    gets the fixed-point allowance the kernel documents: contributions x 2^-40 x M, M = 81 max|g| max|c1|).  The mask decisions are
    the kernel's own (same float32 arithmetic), so no pixel near the threshold needs to be left out.
    images: the images checked (every image is its own problem; the fixed-point scale M is the whole launch's).
    Returns the worst error / bound of grad_c1 and grad_c2."""
    import launch_audit as LA
    c1, c2, gy = c1.cpu(), c2.cpu(), gy.cpu()
    flo = flo.cpu() if flo is not None else None
    cs = 1.0 / c1.shape[1] if normalize else 1.0
    m = 81 * gy.abs().max().item() * cs * c1.abs().max().item()
    if images is not None:
        sel = lambda t: t[images].cpu() if t is not None else None          # noqa: E731
        c1, c2, flo, gy, y, g1, g2, gf = (sel(t) for t in (c1, c2, flo, gy, y, g1, g2, gf))
    r1, r2, rf = _taps_grads(c1, c2, flo, gy, y, scale, align, thr, normalize)
    s1, s2, sf = _taps_grads(c1, c2, flo, gy, y, scale, align, thr, normalize, absolute=True)
    allow = _contributions(flo, scale, align, thr) * 2.0 ** -40 * m if flo is not None else torch.zeros(1)
    q1 = LA.worst(LA.bounded_ratio(g1.cpu(), r1, s1, REL_BWD))[0]
    q2 = LA.worst(LA.bounded_ratio(g2.cpu(), r2, s2 + allow / REL_BWD, REL_BWD))[0]
    print("%s: grad_c1 error/bound %.3f, grad_c2 %.3f" % (what, q1, q2))
    assert q1 <= 1.0 and q2 <= 1.0, (what, q1, q2)
    if flo is not None:
        qf = LA.worst(LA.bounded_ratio(gf.cpu(), rf, sf, REL_BWD))[0]
        print("%s: grad_flo error/bound %.3f" % (what, qf))
        assert qf <= 1.0, (what, qf)
    return q1, q2


NET_CASES = [
    # (id, shape, flow kind, scale, normalize)
    ("l6-c196-tail", (4, 196, 5, 14), None, 1.0, False),        # level 6 of 320x896: 13 chunks of 16, the last of 4 channels
    ("l5-c128", (4, 128, 10, 28), "smooth", 0.625, False),      # level 5 of train.py's shape
    ("l4-c96", (4, 96, 20, 56), "rough", 1.25, True),           # level 4
    ("l3-ny3-of-4", (16, 64, 56, 128), "smooth", 2.5, False),   # level 3 at batch 16, 448x1024: 448 tiles -> ny = 3 of 4 chunks
    ("arena-views", (2, 32, 24, 64), "rough", 5.0, False),      # c1 / c2 / gy batch-strided channel slices of larger tensors
    ("heavy-gy", (2, 32, 24, 64), "smooth", 5.0, False),        # one element of gy 1e4 x the rest
    ("collapse", (1, 32, 16, 64), "collapse", 5.0, False),      # every pixel of an 8 x 32 tile samples one source pixel
]


@pytest.mark.parametrize("case", NET_CASES, ids=[c[0] for c in NET_CASES])
def test_fused_backward_network_channel_counts_per_element(dev, case):
    from opticalflow_amd import ops
    cid, shape, kind, scale, normalize = case
    B, C, H, W = shape
    thr = THR_DC
    if kind == "collapse":
        c1, c2, _, gy = _inputs(shape, None, scale, False, thr, 700)
        # pixel (x, y) of tile (tx, ty) samples (x, y) + scale * flo = the tile's centre + 0.25 (one source cell, all four taps)
        yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        cx, cy = (xx // 32) * 32 + 16.25, (yy // 8) * 8 + 4.25              # sample coordinate ix = px W / (W - 1) - 0.5
        flo = torch.stack((((cx + 0.5) * (W - 1) / W - xx) / scale, ((cy + 0.5) * (H - 1) / H - yy) / scale)).unsqueeze(0).contiguous()
        flo = _away_from_edges(flo, scale, False, thr)
    else:
        c1, c2, flo, gy = _inputs(shape, kind, scale, False, thr, 700 + C)
    if cid == "heavy-gy":
        gy[1, 40, 11, 20] = 1e4
    nchunk = (C + 15) // 16
    tiles = B * ((W + 31) // 32) * ((H + 7) // 8)
    ny = 1 if tiles >= 1024 else min((1024 + tiles - 1) // tiles, nchunk)
    if cid == "l6-c196-tail":
        assert nchunk == 13 and C - 16 * (nchunk - 1) == 4
    if cid == "l3-ny3-of-4":
        assert (tiles, ny, nchunk) == (448, 3, 4)        # one y-slice walks chunks 0 and 3: its grad_flo partials span two chunks
    d = [t.to(dev) if t is not None else None for t in (c1, c2, flo, gy)]
    if cid == "arena-views":
        big = [torch.randn(B, 2 * C + 7, H, W, device=dev), torch.randn(B, 3 * C, H, W, device=dev), torch.randn(B, 170, H, W, device=dev)]
        big[0][:, 5:5 + C] = d[0]
        big[1][:, C:2 * C] = d[1]
        big[2][:, 81:162] = d[3]
        d[0], d[1], d[3] = big[0][:, 5:5 + C], big[1][:, C:2 * C], big[2][:, 81:162]
        assert not d[0].is_contiguous() and not d[3].is_contiguous()
    y = ops.WarpCorrelationFunction.apply(d[0], d[1], d[2], scale, False, thr, 1.0, normalize, 0.1)
    g = ops.warp_correlation_backward(d[0], d[1], d[2], y, d[3], scale, False, thr, 1.0, normalize, 0.1)
    _check_per_element(c1, c2, flo, gy, y, *g, scale, False, thr, normalize, cid, images=[0, 6, B - 1] if B > 4 else None)
    h = ops.warp_correlation_backward(d[0], d[1], d[2], y, d[3], scale, False, thr, 1.0, normalize, 0.1)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(g, h))
    k = ops.warp_correlation_backward(d[0], d[1], d[2], y, d[3], scale, False, thr, 1.0, normalize, 0.1, fused=False)
    for a, r, n in zip(g, k, ("grad_c1", "grad_c2", "grad_flo")):
        if a is not None:
            _close(a, r.double().cpu(), 1e-6, n + " vs composition")


def test_training_step_train_shape_every_cost_volume_launch(dev, monkeypatch):
    """One training step of PWCDCNet(trainable=True) at train.py's 4 x 6 x 320 x 896: every pwc_warp_corr81_bwd launch (five levels)
    recorded with its inputs and checked per element (_check_per_element) from those inputs, on the first and the last image."""
    from opticalflow_amd import PWCDCNet, ops
    net, _ = _net(PWCDCNet, dev)
    x = seeded_rand((4, 6, 320, 896), 540).to(dev)
    real = ops.warp_correlation_backward
    calls = []

    def spy(c1, c2, flo, y, grad_y, flow_scale=1.0, align_corners=False, mask_threshold=0.9999, corr_multiply=1.0,
            normalize=False, leaky_slope=0.1, fused=True):
        ins = [t.detach().cpu() if t is not None else None for t in (c1, c2, flo, y, grad_y)]
        out = real(c1, c2, flo, y, grad_y, flow_scale, align_corners, mask_threshold, corr_multiply, normalize, leaky_slope, fused)
        torch.cuda.synchronize()
        calls.append((ins, [t.cpu() if t is not None else None for t in out], (flow_scale, align_corners, mask_threshold, normalize)))
        return out
    monkeypatch.setattr(ops, "warp_correlation_backward", spy)
    flows = net(x)
    sum(w * f.abs().mean() for w, f in zip(LEVEL_W, flows)).backward()
    monkeypatch.undo()
    assert sorted(c[0][0].shape[1] for c in calls) == [32, 64, 96, 128, 196]
    for (c1, c2, flo, y, gy), (g1, g2, gf), (scale, align, thr, normalize) in calls:
        _check_per_element(c1, c2, flo, gy, y, g1, g2, gf, scale, align, thr, normalize, "train step C=%d" % c1.shape[1], images=[0, 3])
