"""GPU checks of csrc/pwc_proxy_loss.hip off the aligned training sizes of tests/test_gpu_proxy_loss.py: the ragged cases of
tests/proxy_loss_cases.py (one-pixel and two-pixel tile tails, flows at image size, the 2 x 2 extremes, ratios of 3.4, 3.82, 65
and just under 1, h = H with w < W, one and four channels) against the fp64 oracle (tests/proxy_loss_oracle.py), through the
comparators that tests/test_proxy_loss_cases_cpu.py shows can fail.  The gradient is checked for three upstream gradients -- photo
only, total, smooth only -- so that no term hides behind another's scale.  Every bound is one the project already asserts for the
same quantity (rtol 1e-5 / atol 1e-7 on the losses, 1e-4 max|g| on the gradient, 1e-6 / 1e-4 max|img| on the warp) or is derived
in proxy_loss_cases.py (4 x 2^-24 max|g| on the smoothness gradient); each test prints the worst error / bound it saw (`pytest -s`).

Worst error / bound seen on an MI355X (2026-10-20, kernels as of e35b48a; none within a factor of 4 of its bound):
  (total, photo, smooth)          8.9e-3  (under-tile-same, rough)      bound rtol 1e-5 + atol 1e-7
  gradient, photo only            2.0e-2  (near-1, rough)               bound 1e-4 max|g|
  gradient, total                 1.7e-2  (near-1, rough)               bound 1e-4 max|g|
  gradient, smooth only           0.20    (same-3-tiles, rough)         bound 4 x 2^-24 max|g|
  warp vs float32 restatement     0       (every case: equal bits)      bound 1e-6 max|img|
  warp vs fp64                    1.4e-3  (coarse-2x2, rough)           bound 1e-4 max|img|
  exact zeros (oob flows, all-off masks), equal bits across mask dtypes / shapes, strided and dense operands, two calls, and
  autograd against ops.proxy_loss_backward: all held.

That the file bites was shown on scratch builds of the kernel with one arithmetic change each (never committed):
  backward window as if the halo were 1 (outer ring of dL/dmap zero)   19 tests here fail; 21 of test_gpu_proxy_loss.py fail too
  first_user's estimate + 2 rows / columns late, no walk               15 here, 20 there
  first_user's estimate as it is, without the two walks               none, here or there: the estimate starts 2 early and the
                                                                      extra rows / columns weigh 0: the sums do not change,
                                                                      the walks only save work
  bs_1 = bs_2 = C H W whatever the caller's batch stride              test_batch_strided_operands (both cases) only; none there
  weights 0.85 / 3 and 0.15 / 3 whatever C                            the c1 and c4 cases only; none there
"""
import numpy as np
import pytest
import torch

import proxy_loss_cases as PC
import proxy_loss_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
AP, AS = 1.0, 0.1           # the default alphas, as the oracle results of proxy_loss_cases.oracle


def _report(what, value):
    print("[proxy-edges] %s: worst error / bound = %.3e" % (what, value))


def _bits(t):
    return t.detach().cpu().contiguous().numpy().tobytes()


def _strided(t, dev, extra=37):
    """Device view of t [B,...] (float32) whose batch stride is larger than a sample; the gap is NaN, so a kernel that ignores
    the stride shows (as test_gpu_epipolar_edges._strided)."""
    n = t[0].numel()
    buf = torch.full((t.shape[0], n + extra), NAN, device=dev)
    v = buf[:, :n].view(t.shape)
    v.copy_(t)
    assert t.shape[0] == 1 or v.stride(0) == n + extra
    return buf, v


def _gout(which, dev):
    return torch.tensor(PC.GRAD_OUTS[which], dtype=torch.float32, device=dev)


def _run(flow, img1, img2, mask, eps, whichs=tuple(PC.GRAD_OUTS)):
    """(losses [3] as float64 NumPy, {which: grad_flow NumPy}, the bits of all of it) of one forward and len(whichs) backwards"""
    from opticalflow_amd import ops
    out = ops.proxy_loss(flow, img1, img2, mask, AP, AS, eps)
    g = {w: ops.proxy_loss_backward(flow, img1, img2, mask, _gout(w, flow.device), AP, AS, eps) for w in whichs}
    assert out.dtype == torch.float32 and tuple(out.shape) == (3,)
    assert all(t.dtype == torch.float32 and tuple(t.shape) == tuple(flow.shape) and t.is_contiguous() for t in g.values())
    bits = _bits(out) + b"".join(_bits(g[w]) for w in whichs)
    return out.double().cpu().numpy(), {w: t.cpu().numpy() for w, t in g.items()}, bits


def _against_oracle(tag, out, g, name, kind, eps, mask_kind=None):
    worst = {}
    for w in g:
        ref, gr = PC.oracle(name, kind, eps, w, mask_kind)
        try:
            worst["loss"] = PC.check_losses(out, ref)
            worst[w] = PC.check_grad(g[w], gr, w)
        except AssertionError as e:
            raise AssertionError("%s eps %g: %s" % (tag, eps, e)) from None
    for k, v in worst.items():
        _report("%s eps %g %s" % (tag, eps, k), v)
    return worst


def _inputs(name, kind, dev):
    img1, img2 = PC.images(name)
    return PC.flow(name, kind).to(dev), img1.to(dev), img2.to(dev)


# ---------------------------------------------------------------------------------------------------------------- loss, gradient
@pytest.mark.parametrize("name,kind", PC.CASE_KINDS, ids=["%s-%s" % nk for nk in PC.CASE_KINDS])
def test_loss_and_gradients_match_oracle(gpu_device, name, kind):
    flow, img1, img2 = _inputs(name, kind, gpu_device)
    for eps in PC.EPS:
        out, g, bits = _run(flow, img1, img2, None, eps)
        _against_oracle("%s-%s" % (name, kind), out, g, name, kind, eps)
        if kind == "oob":
            PC.check_axis_zero(g["photo"])            # every sample clipped on both axes: exact zeros, not small numbers
        if kind != "rough":
            assert not g["smooth"].any()              # a constant flow: |0| has gradient 0
        assert _run(flow, img1, img2, None, eps)[2] == bits


# ---------------------------------------------------------------------------------------------------------------- masks
@pytest.mark.parametrize("mask_kind", PC.MASK_KINDS)
@pytest.mark.parametrize("name", PC.MASK_CASES)
def test_masks(gpu_device, name, mask_kind):
    """every mask kind as bool / uint8 / float32 and [B,H,W] / [B,1,H,W]: one result, bit for bit, and it is the oracle's"""
    flow, img1, img2 = _inputs(name, "rough", gpu_device)
    first = None
    for tag, m in PC.mask_variants(mask_kind, name):
        out, g, bits = _run(flow, img1, img2, m.to(gpu_device), PC.EPS[1])
        if first is None:
            first = bits
            _against_oracle("%s mask %s" % (name, mask_kind), out, g, name, "rough", PC.EPS[1], mask_kind)
            out0, g0, _ = _run(flow, img1, img2, m.to(gpu_device), PC.EPS[0], ("photo",))
            _against_oracle("%s mask %s" % (name, mask_kind), out0, g0, name, "rough", PC.EPS[0], mask_kind)
        assert bits == first, (mask_kind, tag)
        if mask_kind == "off":
            assert out[1] == 0.0 and out[0] == np.float32(AS) * np.float32(out[2])
            PC.check_axis_zero(g["photo"])


# ---------------------------------------------------------------------------------------------------------------- strides
@pytest.mark.parametrize("name", PC.STRIDED_CASES)
def test_batch_strided_operands(gpu_device, name):
    """what the training scripts pass: the two halves of one [B,6,H,W] batch (batch stride 6 H W), a batch-strided flow with NaN
    between its samples, and one channel of a [B,2,H,W] float mask whose other channel is NaN"""
    from opticalflow_amd import ops
    c = PC.CASES[name]
    i1, i2 = PC.images(name)
    x = torch.cat((i1, i2), dim=1).to(gpu_device)
    img1, img2 = x[:, :3], x[:, 3:]
    fbuf, flow = _strided(PC.flow(name), gpu_device)
    mm = torch.full((c.B, 2, c.H, c.W), NAN, device=gpu_device)
    mm[:, 0] = torch.from_numpy(PC.mask_pattern("half", name)[1]).to(gpu_device)
    mask = mm[:, 0]
    for v, bs in ((img1, 6 * c.H * c.W), (img2, 6 * c.H * c.W), (flow, 2 * c.h * c.w + 37)):
        assert ops.densify(v) is v and v.stride(0) == bs and not v.is_contiguous()      # the kernel does receive the strides
    assert not mask.is_contiguous()
    dense = tuple(t.contiguous() for t in (flow, img1, img2, mask))
    for m_v, m_d, mk in ((None, None, None), (mask, dense[3], "half")):
        for eps in PC.EPS:
            out_v, g_v, bits_v = _run(flow, img1, img2, m_v, eps)
            out_d, g_d, bits_d = _run(dense[0], dense[1], dense[2], m_d, eps)
            assert bits_v == bits_d, (name, mk, eps)
            _against_oracle("%s strided mask %s" % (name, mk), out_v, g_v, name, "rough", eps, mk)
            _against_oracle("%s dense mask %s" % (name, mk), out_d, g_d, name, "rough", eps, mk)
    assert bool(torch.isnan(fbuf[:, flow[0].numel():]).all()) and bool(torch.isnan(mm[:, 1]).all())


# ---------------------------------------------------------------------------------------------------------------- module
@pytest.mark.parametrize("name", PC.MODULE_CASES)
def test_module_route(gpu_device, name):
    """ProxyLabelLoss(route="hip") does take the kernels at the smallest and the most extreme geometry, and autograd through it
    is ops.proxy_loss_backward bit for bit"""
    from opticalflow_amd import ops
    from opticalflow_amd.losses import ProxyLabelLoss
    flow, img1, img2 = _inputs(name, "rough", gpu_device)
    for variant, eps in zip(("pseudo", "fundamental"), PC.EPS):
        loss = ProxyLabelLoss(AP, AS, variant=variant, route="hip")
        f = flow.clone().requires_grad_(True)
        assert loss._hip_applies(f, img1, img2, None) and ops.proxy_loss_supported(f, img1, img2)
        total, photo, smooth = loss(f, img1, img2)
        total.backward()
        out, g, _ = _run(flow, img1, img2, None, eps, ("total",))
        assert _bits(torch.stack((total, photo, smooth))) == _bits(ops.proxy_loss(flow, img1, img2, None, AP, AS, eps))
        assert f.grad.cpu().numpy().tobytes() == g["total"].tobytes()
        _against_oracle("%s module %s" % (name, variant), out, {"total": f.grad.cpu().numpy()}, name, "rough", eps)


# ---------------------------------------------------------------------------------------------------------------- warp
WARP_CASES = [(n, None, "rough") for n in PC.CASES] + [("tail-1", 2, "rough"), ("tail-1", None, "oob"), ("same-3-tiles", None, "oob")]


@pytest.mark.parametrize("name,C,kind", WARP_CASES, ids=["%s%s-%s" % (n, "" if C is None else "-C%d" % C, k) for n, C, k in WARP_CASES])
def test_warp_image_edges(gpu_device, name, C, kind):
    from opticalflow_amd import ops
    from opticalflow_amd.losses import warp_image
    img = PC.images(name, C)[0]
    f = PC.flow(name, kind)
    B, C, H, W = img.shape
    amax = img.abs().max().item()
    img_d, f_d = img.to(gpu_device), f.to(gpu_device)
    out = warp_image(img_d, f_d)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, C, H, W)
    # against the float32 restatement of the kernel's arithmetic, and against fp64 at the kernel's sample points
    e32 = (out.cpu() - O.warp32(img, f)).abs().max().item() / (PC.WARP32_TOL * amax)
    e64 = (out.cpu().double() - O.warp_image64(img, f)).abs().max().item() / (PC.WARP64_TOL * amax)
    _report("%s-%s C=%d warp vs float32 restatement" % (name, kind, C), e32)
    _report("%s-%s C=%d warp vs fp64" % (name, kind, C), e64)
    assert e32 <= 1.0 and e64 <= 1.0, (e32, e64)
    # a caller's batch-strided output: the same bits, and the NaN between (and behind) the samples stays
    n = C * H * W
    buf = torch.full((B, n + 37), NAN, device=gpu_device)
    view = buf[:, :n].view(B, C, H, W)
    _, fv = _strided(f, gpu_device)
    got = ops.flow_warp_image(img_d, fv, out=view)
    assert got.data_ptr() == buf.data_ptr() and _bits(got) == _bits(out)
    assert bool(torch.isnan(buf[:, n:]).all())
