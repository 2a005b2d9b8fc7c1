"""GPU checks of the fused proxy-label loss (csrc/pwc_proxy_loss.hip) against the reference's own float64 results (g8 fixture)
and, per element, against the fp64 oracle of tests/proxy_loss_oracle.py at training sizes.  Every size here is a multiple of the
16 x 64 tile or leaves a 32-column tail, every flow is at a quarter of the image (or at its size), C = 3 and the operands are dense;
tests/test_gpu_proxy_loss_edges.py runs the same oracle off those sizes: one- and two-pixel tile tails, the 2 x 2 extremes,
non-integer ratios, one and four channels, batch-strided operands, and the gradient per term (tests/proxy_loss_cases.py)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import proxy_loss_oracle as O

pytestmark = pytest.mark.gpu


def _case(z, name, dev):
    pfx = "base" if name.startswith("base") or name == "masked" else name
    img1, img2 = (torch.from_numpy(z[pfx + k]).to(dev) for k in ("/img1", "/img2"))
    flow = torch.from_numpy(z[name + "/flow"]).to(dev)
    mask = torch.from_numpy(z[name + "/mask"]).to(dev) if name + "/mask" in z.files else None
    ap, asm, fund = (float(v) for v in z[name + "/cfg"])
    return flow, img1, img2, mask, ap, asm, "fundamental" if fund else "pseudo"


def _hip(flow, img1, img2, mask=None, ap=1.0, asm=0.1, variant="pseudo", grad_out=(1.0, 0.0, 0.0)):
    from opticalflow_amd.losses import ProxyLabelLoss
    f = flow.detach().clone().requires_grad_(True)
    out = ProxyLabelLoss(ap, asm, variant=variant, route="hip")(f, img1, img2, mask)
    g = sum(c * t for c, t in zip(grad_out, out) if c != 0.0)
    g.backward()
    return torch.stack([t.detach() for t in out]), f.grad


@pytest.mark.parametrize("name", ["base_pseudo", "base_fund", "odd", "same", "clamp", "masked"])
def test_hip_matches_reference_g8(gpu_device, name):
    z = load_golden("g8_proxy_loss.npz")
    flow, img1, img2, mask, ap, asm, variant = _case(z, name, gpu_device)
    out, g = _hip(flow, img1, img2, mask, ap, asm, variant)
    ref = z[name + "/loss"]
    np.testing.assert_allclose(out.cpu().double().numpy(), ref, rtol=1e-5, atol=0)
    gr = z[name + "/grad_flow"]
    err = np.abs(g.cpu().double().numpy() - gr).max()
    assert err <= 1e-4 * np.abs(gr).max(), (name, err, np.abs(gr).max())


def _images(B, C, H, W, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.sin(0.07 * xx + 0.05 * yy)[None, None] + 0.5 * (xx > W / 3).float()[None, None]
    img1 = (base + 0.3 * torch.rand(B, C, H, W, generator=gen)).clamp(-1, 2) * 1.5 - 0.6
    img2 = torch.roll(img1, shifts=(2, -3), dims=(2, 3)) + 0.05 * torch.randn(B, C, H, W, generator=gen)
    return img1.to(dev), img2.to(dev)


def _flow(B, h, w, seed, rough, dev):
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    f = torch.stack((3 * torch.sin(4 * xx + yy), 2 * torch.cos(3 * yy - xx)))[None].repeat(B, 1, 1, 1)
    if rough:
        f = f + 4.0 * torch.randn(B, 2, h, w, generator=gen)
    return f.to(dev)


def _check_oracle(flow, img1, img2, mask=None, ap=1.0, asm=0.1, variant="pseudo", grad_out=(1.0, 0.0, 0.0)):
    out, g = _hip(flow, img1, img2, mask, ap, asm, variant, grad_out)
    ref, gr = O.proxy_loss64(flow, img1, img2, mask, ap, asm, 1e-12 if variant == "fundamental" else 0.0, grad_out)
    np.testing.assert_allclose(out.double().cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-7)
    gmax = gr.abs().max().item()
    err = (g.double() - gr).abs().max().item()
    assert err <= 1e-4 * gmax, (err, gmax)
    return out, g


@pytest.mark.parametrize("shape", [(4, 3, 384, 512), (2, 3, 448, 1024)])
@pytest.mark.parametrize("rough", [False, True])
def test_oracle_training_sizes(gpu_device, shape, rough):
    B, C, H, W = shape
    img1, img2 = _images(B, C, H, W, 1, gpu_device)
    _check_oracle(_flow(B, H // 4, W // 4, 2, rough, gpu_device), img1, img2)


def test_oracle_zero_flow(gpu_device):
    img1, img2 = _images(4, 3, 384, 512, 3, gpu_device)
    _check_oracle(torch.zeros(4, 2, 96, 128, device=gpu_device), img1, img2)


@pytest.mark.parametrize("variant", ["pseudo", "fundamental"])
@pytest.mark.parametrize("mask_kind", [None, "bool", "float4d", "none_true"])
def test_variants_and_masks(gpu_device, variant, mask_kind):
    B, C, H, W = 2, 3, 96, 160
    img1, img2 = _images(B, C, H, W, 4, gpu_device)
    flow = _flow(B, 24, 40, 5, True, gpu_device)
    gen = torch.Generator().manual_seed(6)
    mask = None
    if mask_kind == "bool":
        mask = (torch.rand(B, H, W, generator=gen) > 0.3).to(gpu_device)
    elif mask_kind == "float4d":
        mask = torch.rand(B, 1, H, W, generator=gen).to(gpu_device)
    elif mask_kind == "none_true":
        mask = torch.zeros(B, H, W, dtype=torch.bool, device=gpu_device)    # all false: denominator 1, photo 0
    out, _ = _check_oracle(flow, img1, img2, mask, 0.8, 0.25, variant)
    if mask_kind == "none_true":
        assert out[1].item() == 0.0


@pytest.mark.parametrize("grad_out", [(0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.5, -2.0, 3.0)])
def test_upstream_gradients(gpu_device, grad_out):
    img1, img2 = _images(2, 3, 64, 96, 7, gpu_device)
    _check_oracle(_flow(2, 16, 24, 8, True, gpu_device), img1, img2, None, 1.3, 0.05, "pseudo", grad_out)


def test_autocast_low_precision_flow(gpu_device):
    from opticalflow_amd.losses import ProxyLabelLoss
    img1, img2 = _images(2, 3, 64, 96, 9, gpu_device)
    for dt in (torch.bfloat16, torch.float16):
        f = _flow(2, 16, 24, 10, False, gpu_device).to(dt).requires_grad_(True)
        with torch.autocast("cuda", dtype=dt):
            total, photo, smooth = ProxyLabelLoss()(f, img1, img2)
        assert total.dtype == torch.float32 and photo.dtype == torch.float32
        total.backward()
        assert f.grad is not None and f.grad.dtype == dt
        ref, gr = O.proxy_loss64(f.detach().float(), img1, img2)           # the oracle on the rounded flow
        assert abs(total.item() - ref[0].item()) <= 1e-5 * abs(ref[0].item())
        # the fp32 gradient, cast back to the flow's dtype: its rounding (eps/2 relative) on top of the fp32 bound
        fi = torch.finfo(dt)
        bound = 1e-4 * gr.abs().max() + fi.eps * gr.abs() + fi.tiny * fi.eps      # last term: fp16 subnormal spacing
        assert ((f.grad.double() - gr).abs() <= bound).all(), dt


def test_deterministic(gpu_device):
    img1, img2 = _images(4, 3, 384, 512, 11, gpu_device)
    flow = _flow(4, 96, 128, 12, True, gpu_device)
    mask = torch.rand(4, 384, 512, device=gpu_device)
    a = _hip(flow, img1, img2, mask, variant="fundamental")
    b = _hip(flow, img1, img2, mask, variant="fundamental")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_decline_routes_match_torch(gpu_device):
    from opticalflow_amd import ops
    from opticalflow_amd.losses import ProxyLabelLoss
    img1, img2 = _images(2, 3, 64, 96, 13, gpu_device)
    flow = _flow(2, 16, 24, 14, True, gpu_device)
    cases = [(flow, img1.clone().requires_grad_(True), img2),                 # image requires grad
             (_flow(2, 80, 24, 15, True, gpu_device), img1, img2),            # H < h
             (_flow(2, 1, 24, 16, True, gpu_device), img1, img2),             # h < 2
             (flow[:, :, :1, :1], img1[:, :, :1, :1], img2[:, :, :1, :1])]    # tiny maps
    cases += [(flow.half(), img1, img2),                                       # fp16 flow outside autocast
              (flow, img1, img2.double()),                                    # float64 img2 with a float32 img1
              (flow.bfloat16(), img1.bfloat16(), img2.bfloat16())]
    for f, a, b in cases:
        assert not ProxyLabelLoss(route="hip")._hip_applies(f, a, b, None)
        fh = f.detach().clone().requires_grad_(True)
        ft = f.detach().clone().requires_grad_(True)
        th = ProxyLabelLoss(route="hip")(fh, a, b)
        tt = ProxyLabelLoss(route="torch")(ft, a, b)
        for x, y in zip(th, tt):
            assert torch.equal(x, y) or (torch.isnan(x) and torch.isnan(y))
    assert ops.proxy_loss_supported(flow, img1, img2)


def test_memory_peak(gpu_device):
    from opticalflow_amd import ops
    from opticalflow_amd.losses import ProxyLabelLoss
    B, C, H, W = 4, 3, 384, 512
    img1, img2 = _images(B, C, H, W, 17, gpu_device)
    flow = _flow(B, 96, 128, 18, True, gpu_device)
    peaks = {}
    for route in ("hip", "torch"):
        f = flow.clone().requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        total, _, _ = ProxyLabelLoss(route=route)(f, img1, img2)
        total.backward()
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - base
        del total, f
    ws = ops.proxy_loss_workspace_bytes(B, C, H, W, 96, 128)
    gflow = B * 2 * 96 * 128 * 4
    print("proxy loss fwd+bwd peak above inputs: hip %.1f MiB, torch %.1f MiB (workspace %.1f MiB)"
          % (peaks["hip"] / 2 ** 20, peaks["torch"] / 2 ** 20, ws / 2 ** 20))
    assert peaks["hip"] <= gflow + ws + 16 * 2 ** 20


def test_training_step_both_routes(gpu_device):
    """One train_pseudo step (train_pseudo.py:245-262) at 4x6x384x512: flow2 of PWCDCNet(trainable=True), the loss by both
    routes on the same forward graph (so only the loss's gradient differs), parameter gradients compared per tensor; then one
    SGD step with the HIP route lowers the loss."""
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.losses import ProxyLabelLoss
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(gpu_device).train()
    img1, img2 = _images(4, 3, 384, 512, 19, gpu_device)
    x = torch.cat((img1, img2), dim=1)
    params = [p for p in net.parameters() if p.requires_grad]
    flow2 = net(x)[0]
    grads, losses = {}, {}
    for route in ("hip", "torch"):
        total, _, _ = ProxyLabelLoss(route=route)(flow2, img1, img2)
        grads[route] = torch.autograd.grad(total, params, retain_graph=True, allow_unused=True)
        losses[route] = total.item()
    # the reference expression in float64 on the same flow2 (torch route, float64 images): the yardstick of both fp32 routes
    f64 = flow2.detach().double().requires_grad_(True)
    t64, _, _ = ProxyLabelLoss(route="torch")(f64, img1.double(), img2.double())
    (g64,) = torch.autograd.grad(t64, f64)
    grads["fp64"] = torch.autograd.grad(flow2, params, grad_outputs=g64.float(), retain_graph=True, allow_unused=True)
    assert abs(losses["hip"] - losses["torch"]) <= 1e-5 * abs(losses["torch"])

    def worst(r, s):
        w = 0.0
        for a, b in zip(grads[r], grads[s]):
            assert (a is None) == (b is None)
            if a is not None and b.norm().item() > 0:
                w = max(w, (a - b).norm().item() / b.norm().item())
        return w

    w_ht, w_h64, w_t64 = worst("hip", "torch"), worst("hip", "fp64"), worst("torch", "fp64")
    print("train step, worst per-tensor relative difference of the parameter gradients: hip vs torch %.2e, hip vs fp64 %.2e, "
          "torch vs fp64 %.2e" % (w_ht, w_h64, w_t64))
    # Why not 1e-4 between the routes: both float32 routes sit ~1e-3 (norm-wise, worst tensor) from the float64 expression.
    # The first layers' gradients sum every pixel's contribution with heavy cancellation, and each route's float32 sample
    # points (~3e-5 px at x ~ 500) move those contributions.  Measured on grad_flow itself (2x3x384x512, this file's image
    # recipe, CPU): the torch route in float32 differs from float64 by 3.2e-3 norm-wise and by 8.7e-2 of max|g| on its worst
    # element; float64 at the kernel's float32 sample points differs from float64 by 3.3e-3.  On the parameters (this test,
    # five runs): hip vs fp64 1.3-3.5e-3, torch vs fp64 1.0-2.8e-3, hip vs torch 5.0-8.1e-4.  They move from run to run:
    # flow2 comes from convolutions whose algorithms are not bit-reproducible, and every floor / kink decision a tiny change
    # of flow2 flips moves a whole pixel's contribution.  So: the fused route within twice the reference chain's own distance
    # to float64, and the two routes within 1.5e-3 of each other (about twice the largest difference measured).
    assert w_h64 <= max(2.0 * w_t64, 1e-4), (w_ht, w_h64, w_t64)
    assert w_ht <= 1.5e-3, (w_ht, w_h64, w_t64)
    opt = torch.optim.SGD(net.parameters(), lr=1e-4)
    net.zero_grad(set_to_none=True)
    total, _, _ = ProxyLabelLoss(route="hip")(net(x)[0], img1, img2)
    total.backward()
    opt.step()
    after, _, _ = ProxyLabelLoss(route="hip")(net(x)[0], img1, img2)
    assert after.item() < total.item()


@pytest.mark.parametrize("C", [2, 3])
def test_warp_image_against_oracle(gpu_device, C):
    from opticalflow_amd.losses import ProxyLabelLoss, warp_image
    img, _ = _images(2, C, 96, 160, 20, gpu_device)
    flow = _flow(2, 24, 40, 21, True, gpu_device)
    full = _flow(2, 96, 160, 22, True, gpu_device)                           # flows at image resolution (train_pseudo.py:178-193)
    amax = img.abs().max().item()
    w64 = warp_image(img.double(), flow.double())                             # float64 stays on the torch composition
    assert w64.dtype == torch.float64
    assert (w64 - O.warp_image64(img, flow)).abs().max().item() <= 1e-4 * img.abs().max().item()
    for f in (flow, full):
        out = warp_image(img, f)
        # against the float32 restatement of the kernel's arithmetic: the same operations in the same order
        assert (out - O.warp32(img, f)).abs().max().item() <= 1e-6 * amax
        # against fp64 at the kernel's sample points: what fp32 coordinates (~1e-6 px on 10 px flows) leave at image slopes ~1
        assert (out.double() - O.warp_image64(img, f)).abs().max().item() <= 1e-4 * amax
    assert torch.equal(ProxyLabelLoss().warp(img, flow), warp_image(img, flow))
