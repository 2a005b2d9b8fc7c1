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
