"""The supervised losses of train.py / train2.py on the MI355X: the HIP route against the reference's own float64 results (g10)
and against the fp64 oracle at the bench sizes and at KITTI 375x1242 with a 94x311 prediction.  Bounds: losses rtol 1e-5,
gradients 1e-4 x max|g|.  Also: masks (all zero, u8 vs f32, [B,1,H,W] vs [B,H,W]), the regularisers, autocast, bit-identical
reruns, the torch fallback, and one train.py step of PWCDCNet(trainable=True) against the torch loss."""
import numpy as np
import pytest
import torch

from conftest import load_golden
import supervised_loss_oracle as O
from test_supervised_loss_cpu import FLOW_CASES, MS_CASES, _flow_case, _ms_case

pytestmark = pytest.mark.gpu


def _close_loss(got, want):
    np.testing.assert_allclose(float(got), float(want), rtol=1e-5, atol=1e-9)


def _close_grad(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-4 * max(np.abs(want).max(), 1e-30))


def _route(loss):
    """'hip' when the 0-dim loss is an element of one of the fused autograd Functions' outputs, else 'torch'."""
    fn = loss.grad_fn
    nxt = fn.next_functions[0][0] if fn is not None and fn.next_functions else None
    return "hip" if nxt is not None and type(nxt).__name__ in ("FlowLossFunctionBackward", "MultiscaleLossFunctionBackward") else "torch"


def _f(t, dev):
    return None if t is None else t.float().to(dev)


@pytest.mark.parametrize("name", FLOW_CASES)
def test_flow_loss_matches_g10(gpu_device, name):
    from opticalflow_amd import losses
    z = load_golden("g10_supervised_loss.npz")
    pred, gt, mask, want, gwant = _flow_case(z, name)
    p = _f(pred, gpu_device).requires_grad_(True)
    g, m = _f(gt, gpu_device), _f(mask, gpu_device)
    if name.startswith("epe"):
        with torch.no_grad():
            _close_loss(losses.compute_epe(p, g, m).item(), want)
        return
    loss = losses.MaskedCharbonnier()(p, g, m)
    assert _route(loss) == "hip"
    loss.backward()
    _close_loss(loss.item(), want)
    _close_grad(p.grad.cpu(), gwant)


@pytest.mark.parametrize("name", MS_CASES)
def test_multiscale_matches_g10(gpu_device, name):
    from opticalflow_amd import losses
    z = load_golden("g10_supervised_loss.npz")
    preds, images, gt, mask, w, lp, ls, want, gwant = _ms_case(z, name)
    ps = [_f(p, gpu_device).requires_grad_(True) for p in preds]
    loss = losses.supervised_multiscale_loss(ps, _f(images, gpu_device), _f(gt, gpu_device), _f(mask, gpu_device), w=w,
                                             lambda_photo=lp, lambda_smooth=ls)
    assert _route(loss) == "hip"
    loss.backward()
    _close_loss(loss.item(), want)
    for p, gw in zip(ps, gwant):
        _close_grad(p.grad.cpu(), gw)


# (B, H, W, h, w): train.py's 4x320x896 with flow2 80x224, KITTI full frames with a 94x311 prediction, 16x448x1024
FLOW_SIZES = ((4, 320, 896, 80, 224), (1, 375, 1242, 94, 311), (16, 448, 1024, 112, 256))


@pytest.mark.parametrize("B,H,W,h,w", FLOW_SIZES)
def test_flow_loss_vs_oracle_at_training_sizes(gpu_device, B, H, W, h, w):
    from opticalflow_amd import losses
    g = torch.Generator().manual_seed(H + w)
    pred = torch.randn(B, 2, h, w, generator=g) * 3
    gt = torch.randn(B, 2, H, W, generator=g) * 8
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.4).float()
    lo, go = O.flow_loss(pred.numpy(), gt.numpy(), mask.numpy())
    p = pred.to(gpu_device).requires_grad_(True)
    loss = losses.MaskedCharbonnier()(p, gt.to(gpu_device), mask.to(gpu_device))
    loss.backward()
    _close_loss(loss.item(), lo)
    _close_grad(p.grad.cpu(), go)
    with torch.no_grad():
        e = losses.compute_epe(p, gt.to(gpu_device), mask[:, 0].to(gpu_device))
    _close_loss(e.item(), O.flow_loss(pred.numpy(), gt.numpy(), mask.numpy(), eps=0.0, rule="raw")[0])


def _pwc_sizes(H, W):
    return [(H // s, W // s) for s in (4, 8, 16, 32, 64)]


# train2.py's five levels at 4x384x768, and the same level ratios at 16x448x1024 and 4x320x896
@pytest.mark.parametrize("B,H,W", ((4, 384, 768), (16, 448, 1024), (4, 320, 896)))
def test_multiscale_vs_oracle_at_training_sizes(gpu_device, B, H, W):
    from opticalflow_amd import losses
    g = torch.Generator().manual_seed(W)
    preds = [torch.randn(B, 2, h, w, generator=g) * 2 for h, w in _pwc_sizes(H, W)]
    gt = torch.randn(B, 2, H, W, generator=g) * 10
    mask = (torch.rand(B, H, W, generator=g) > 0.3).float()
    lo, go = O.multiscale_loss([p.numpy() for p in preds], None, gt.numpy(), mask.numpy())
    ps = [p.to(gpu_device).requires_grad_(True) for p in preds]
    loss = losses.supervised_multiscale_loss(tuple(ps), None, gt.to(gpu_device), mask.to(gpu_device))
    loss.backward()
    _close_loss(loss.item(), lo)
    for p, gw in zip(ps, go):
        _close_grad(p.grad.cpu(), gw)


def test_multiscale_regularisers_vs_oracle(gpu_device):
    """lambda_photo / lambda_smooth > 0 with a raw mask; flows drawn continuous, so no sample point sits on an integer."""
    from opticalflow_amd import losses
    B, H, W = 2, 128, 256
    g = torch.Generator().manual_seed(5)
    preds = [torch.randn(B, 2, h, w, generator=g) * 1.7 + 0.31 for h, w in _pwc_sizes(H, W)]
    gt = torch.randn(B, 2, H, W, generator=g) * 4
    mask = torch.rand(B, H, W, generator=g)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    images = torch.stack([torch.sin(0.11 * (c + 1) * xx + 0.07 * yy + c) for c in range(6)]).expand(B, 6, H, W).contiguous()
    images = images + 0.1 * torch.randn(B, 6, H, W, generator=g)
    lo, go = O.multiscale_loss([p.numpy() for p in preds], images.numpy(), gt.numpy(), mask.numpy(), None, 0.4, 0.2)
    ps = [p.to(gpu_device).requires_grad_(True) for p in preds]
    loss = losses.supervised_multiscale_loss(ps, images.to(gpu_device), gt.to(gpu_device), mask.to(gpu_device),
                                             lambda_photo=0.4, lambda_smooth=0.2)
    assert _route(loss) == "hip"
    loss.backward()
    _close_loss(loss.item(), lo)
    for p, gw in zip(ps, go):
        _close_grad(p.grad.cpu(), gw)


def _flow_inputs(dev, B=2, H=64, W=96, h=16, w=24, seed=3):
    g = torch.Generator().manual_seed(seed)
    pred = (torch.randn(B, 2, h, w, generator=g) * 2).to(dev)
    gt = (torch.randn(B, 2, H, W, generator=g) * 5).to(dev)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.5).to(dev)
    return pred, gt, mask


def test_all_zero_mask_uses_the_clamp(gpu_device):
    from opticalflow_amd import losses, ops
    pred, gt, mask = _flow_inputs(gpu_device)
    zero = torch.zeros_like(mask, dtype=torch.float32)
    p = pred.clone().requires_grad_(True)
    loss = losses.MaskedCharbonnier()(p, gt, zero)
    loss.backward()
    assert loss.item() == 0.0 and torch.count_nonzero(p.grad).item() == 0
    out = ops.sup_flow_loss(pred, gt, zero)
    assert out[1].item() == 1.0                         # max(sum valid, 1)
    # one multiscale level whose nearest mask is all zero: that level contributes 0, the others do not
    m2 = torch.ones(2, 64, 96, device=gpu_device)
    m2[:, ::16, :] = 0.0
    preds = [pred.clone().requires_grad_(True), torch.randn(2, 2, 4, 6, device=gpu_device).requires_grad_(True)]
    out = ops.MultiscaleLossFunction.apply(gt, m2, None, (0.32, 0.08), 0.0, 0.0, *preds)
    assert out[1 + 2 + 1].item() == 1.0 and out[2].item() == 0.0       # level 1 (rows 0, 16, 32, 48 of the mask): clamp
    lo, go = O.multiscale_loss([p.detach().cpu().numpy() for p in preds], None, gt.cpu().numpy(), m2.cpu().numpy(), [0.32, 0.08])
    out[0].backward()
    _close_loss(out[0].item(), lo)
    assert torch.count_nonzero(preds[1].grad).item() == 0


def test_u8_vs_f32_and_mask_layouts_agree(gpu_device):
    from opticalflow_amd import losses
    pred, gt, mask = _flow_inputs(gpu_device)
    crit = losses.MaskedCharbonnier()
    res = []
    for m in (mask, mask.float(), mask.to(torch.uint8), mask[:, 0], mask[:, 0].float(), mask[:, 0].to(torch.uint8)):
        p = pred.clone().requires_grad_(True)
        loss = crit(p, gt, m)
        loss.backward()
        res.append((loss.detach(), p.grad))
    for loss, grad in res[1:]:
        assert torch.equal(loss, res[0][0]) and torch.equal(grad, res[0][1])
    preds = [pred.clone(), pred[:, :, ::2, ::2].contiguous()]
    ms = [losses.supervised_multiscale_loss(preds, None, gt, m) for m in (mask, mask.float(), mask[:, 0].to(torch.uint8))]
    assert torch.equal(ms[0], ms[1]) and torch.equal(ms[0], ms[2])


def test_fp16_inputs_under_autocast(gpu_device):
    from opticalflow_amd import losses
    pred, gt, mask = _flow_inputs(gpu_device)
    p16 = pred.half().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        loss = losses.MaskedCharbonnier()(p16, gt.half(), mask)
    assert loss.dtype == torch.float32
    loss.backward()
    assert p16.grad.dtype == torch.float16
    lo, go = O.flow_loss(p16.detach().float().cpu().numpy(), gt.half().float().cpu().numpy(), mask.cpu().numpy())
    _close_loss(loss.item(), lo)
    np.testing.assert_allclose(p16.grad.float().cpu().numpy(), go, rtol=0, atol=2e-3 * np.abs(go).max())   # fp16 gradient
    ps = [p16, p16[:, :, ::2, ::2]]
    with torch.autocast("cuda", dtype=torch.float16):
        ms = losses.supervised_multiscale_loss(ps, None, gt.half(), mask)
    assert ms.dtype == torch.float32 and _route(ms) == "hip"


def test_bit_identical_reruns(gpu_device):
    from opticalflow_amd import losses
    pred, gt, mask = _flow_inputs(gpu_device, B=4, H=320, W=896, h=80, w=224)
    outs = []
    for _ in range(2):
        p = pred.clone().requires_grad_(True)
        ps = [p, p[:, :, ::2, ::2], p[:, :, ::4, ::4]]
        images = torch.sin(torch.arange(4 * 6 * 320 * 896, device=gpu_device, dtype=torch.float32).reshape(4, 6, 320, 896) * 1e-3)
        a = losses.MaskedCharbonnier()(p, gt, mask)
        b = losses.supervised_multiscale_loss(ps, images, gt, mask[:, 0], lambda_photo=0.3, lambda_smooth=0.2)
        (a + b).backward()
        outs.append((a.detach(), b.detach(), p.grad.clone()))
    assert all(torch.equal(x, y) for x, y in zip(outs[0], outs[1]))


def test_falls_back_to_torch_when_gt_requires_grad(gpu_device):
    from opticalflow_amd import losses
    pred, gt, mask = _flow_inputs(gpu_device)
    g = gt.clone().requires_grad_(True)
    p = pred.clone().requires_grad_(True)
    loss = losses.MaskedCharbonnier()(p, g, mask)
    assert _route(loss) == "torch"
    loss.backward()
    assert g.grad is not None and torch.count_nonzero(g.grad).item() > 0
    hip = losses.MaskedCharbonnier()(pred, gt, mask)
    _close_loss(loss.item(), hip.item())
    ms = losses.supervised_multiscale_loss([p], None, g, mask)
    assert _route(ms) == "torch"
    ms.backward()
    assert g.grad is not None
    # float64 and CPU tensors: the torch route too
    assert losses.MaskedCharbonnier()(pred.double(), gt.double(), mask).dtype == torch.float64
    assert losses.compute_epe(pred.cpu(), gt.cpu()).device.type == "cpu"


def test_train_step_hip_vs_torch_loss(gpu_device):
    """One train.py step (train.py:55-72) at 4x6x320x896: flow2 of PWCDCNet(trainable=True), MaskedCharbonnier on its
    upsampling by both routes on the same forward graph, parameter gradients compared per tensor: within 1.5e-3 relative (the
    bound the proxy-loss step test needed: both fp32 routes sit about 1e-3 from float64 on these gradients)."""
    from opticalflow_amd import PWCDCNet, losses
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(gpu_device).train()
    g = torch.Generator().manual_seed(11)
    x = (torch.rand(4, 6, 320, 896, generator=g) * 4.7 - 2.1).to(gpu_device)
    gt = (torch.randn(4, 2, 320, 896, generator=g) * 3).to(gpu_device)
    valid = (torch.rand(4, 1, 320, 896, generator=g) > 0.3).float().to(gpu_device)
    params = [p for p in net.parameters() if p.requires_grad]
    flow2 = net(x)[0]
    grads, vals = {}, {}
    for route in ("hip", "torch"):
        loss = losses.MaskedCharbonnier(route=route)(flow2, gt, valid)
        assert _route(loss) == route
        grads[route] = torch.autograd.grad(loss, params, retain_graph=True, allow_unused=True)
        vals[route] = loss.item()
    assert abs(vals["hip"] - vals["torch"]) <= 1e-5 * abs(vals["torch"])
    worst = 0.0
    for a, b in zip(grads["hip"], grads["torch"]):
        assert (a is None) == (b is None)
        if a is not None and b.norm().item() > 0:
            worst = max(worst, (a - b).norm().item() / b.norm().item())
    print("train.py step: worst per-tensor relative difference of the parameter gradients, hip vs torch loss %.2e" % worst)
    assert worst <= 1.5e-3
