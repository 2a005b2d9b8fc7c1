"""GPU checks of the no-ground-truth validation path: the fused cycle + out-of-bounds kernel (csrc/pwc_fb_metrics.hip) against the
reference's own float64 results (g11 fixture) and the float64 oracle at the scripts' sizes; PWCDCNet.flow_pair (one pyramid pass
per image) against two ordinary forwards; validation.validate as the composition of those parts."""
import numpy as np
import pytest
import torch

from conftest import load_golden, seeded_rand
import validation_oracle as VO

pytestmark = pytest.mark.gpu

CASES = ("smooth", "rough", "odd", "same", "zero", "const_neg", "clamp", "oob_only")
SIZES = [(4, 384, 512), (2, 448, 1024), (3, 200, 328)]


def _flow(B, h, w, seed, rough):
    """Seeded sinusoids of 2-8 px amplitude at quarter resolution, plus noise for the rough kind (the inputs the knife-edge count
    was checked on: a few pixels in 1e5..1e6 lie within 1e-3 px of a border)."""
    gen = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
    ph = torch.rand(2, generator=gen) * 6.0
    f = torch.stack((4.0 * torch.sin(4 * xx + yy + ph[0]), 2.5 * torch.cos(3 * yy - xx + ph[1])))[None].repeat(B, 1, 1, 1)
    f = f * (0.5 + torch.rand(B, 1, 1, 1, generator=gen))
    if rough:
        f = f + 1.0 * torch.randn(B, 2, h, w, generator=gen)
    return f


def _pair(B, H, W, seed, rough):
    h, w = (H + 3) // 4, (W + 3) // 4
    f12 = _flow(B, h, w, seed, rough)
    f21 = -f12 + 0.3 * _flow(B, h, w, seed + 1, rough)          # roughly the inverse flow: a small, non-zero cycle
    return f12, f21


def _atol(f12):
    """Absolute floor used ONLY where the cycle is zero in exact arithmetic (the fixture's const_neg): a and wv each carry a
    handful of float32 roundings (interpolation weights, vector scale), about 8 ulp = 8 * 6e-8 of the upsampled magnitude in all.
    Every other input is compared with the pure relative bound."""
    return 5e-7 * 4.0 * float(np.abs(f12).max())


def _check(f12, f21, H, W, ref_cycle, ref_count, knife, dev, exact_zero=False):
    from opticalflow_amd import ops
    B = f12.shape[0]
    t21 = None if f21 is None else torch.as_tensor(f21).to(dev)
    out, csum, cnt = ops.fb_metrics(torch.as_tensor(f12).to(dev), t21, H, W, raw=True)
    out, csum, cnt = out.cpu(), csum.item(), int(cnt.item())
    print("B %d %dx%d: cycle hip %.9g ref %.9g (rel %.2e); oob count hip %d ref %d knife-edge %d"
          % (B, H, W, csum / (B * 2 * H * W), ref_cycle, abs(csum / (B * 2 * H * W) - ref_cycle) / max(abs(ref_cycle), 1e-30),
             cnt, ref_count, knife))
    if f21 is None:
        assert out[0].item() == 0.0 and csum == 0.0
    else:
        if exact_zero:
            assert abs(ref_cycle) < 1e-12 and abs(csum / (B * 2 * H * W)) <= _atol(np.asarray(f12))
        else:
            np.testing.assert_allclose(csum / (B * 2 * H * W), ref_cycle, rtol=1e-5, atol=0)
        assert out[0].item() == np.float32(csum / (B * 2 * H * W))          # the float32 result is that sum's mean, rounded once
    assert abs(cnt - ref_count) <= knife
    assert out[1].item() == np.float32(cnt / float(B * H * W))
    return out, csum, cnt


@pytest.mark.parametrize("name", CASES)
def test_kernel_matches_reference_g11(gpu_device, name):
    z = load_golden("g11_validation.npz")
    H, W = (int(v) for v in z[name + "/size"])
    f12 = z[name + "/flow12"]
    f21 = z[name + "/flow21"] if name + "/flow21" in z.files else None
    knife = VO.oob_count(f12, H, W)[1]
    # The knife-edge cap of the large inputs is not applied to the fixture: two of its cases are CONSTRUCTED on the edge.  zero:
    # every border pixel's sample point is the border itself, exactly, in any arithmetic (312 pixels) -- no allowance, the count
    # must be 0.  const_neg: the column X = 40 has px = 40 + 7 = W-1 up to the rounding of the interpolated constant (32 pixels),
    # which float32 and float64 may legitimately decide differently; those 32 are its allowance.
    if name == "zero":
        knife = 0
    _, csum, cnt = _check(f12, f21, H, W, float(z[name + "/cycle"][0]), int(z[name + "/oob_count"][0]), knife, gpu_device,
                          exact_zero=(name == "const_neg"))
    if name == "zero":
        assert csum == 0.0 and cnt == 0


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("rough", [False, True])
def test_kernel_matches_oracle_at_script_sizes(gpu_device, size, rough):
    B, H, W = size
    f12, f21 = _pair(B, H, W, 11 + int(rough), rough)
    m = VO.metrics(f12.numpy(), f21.numpy(), H, W)
    # a condition on the INPUTS: the out-of-bounds comparison means something only when few pixels sit on the knife edge
    assert m["knife_edge"] <= 1e-4 * B * H * W, m["knife_edge"]
    assert 0 < m["oob_count"] < B * H * W
    _check(f12, f21, H, W, m["cycle"], m["oob_count"], m["knife_edge"], gpu_device)
    # the stand-alone out-of-bounds call counts the same pixels
    from opticalflow_amd import ops
    _, csum, cnt = ops.fb_metrics(f12.to(gpu_device), None, H, W, raw=True)
    assert abs(int(cnt.item()) - m["oob_count"]) <= m["knife_edge"] and csum.item() == 0.0


def test_full_resolution_flows(gpu_device):
    B, H, W = 2, 96, 160
    f12 = _flow(B, H, W, 21, True) * 3
    f21 = -f12 + _flow(B, H, W, 22, True)
    m = VO.metrics(f12.numpy(), f21.numpy(), H, W)
    assert m["knife_edge"] <= 1e-4 * B * H * W
    _check(f12, f21, H, W, m["cycle"], m["oob_count"], m["knife_edge"], gpu_device)


def test_torch_route_vs_hip_route(gpu_device):
    from opticalflow_amd import ops, validation as V
    for (B, H, W), rough in zip(SIZES, (True, False, True)):
        f12, f21 = (t.to(gpu_device) for t in _pair(B, H, W, 31, rough))
        knife = VO.oob_count(f12.cpu().numpy(), H, W)[1]
        assert knife <= 1e-4 * B * H * W
        ch, oh = V.cycle_and_oob(f12, f21, H, W, route="hip")
        ct, ot = V.cycle_and_oob(f12, f21, H, W, route="torch")
        assert ch.dim() == 0 and oh.dim() == 0 and ch.dtype == torch.float32
        print("%dx%dx%d: cycle hip %.9g torch %.9g; oob hip %.9g torch %.9g (knife-edge %d)" % (B, H, W, ch.item(), ct.item(),
                                                                                             oh.item(), ot.item(), knife))
        np.testing.assert_allclose(ch.item(), ct.item(), rtol=1e-5)
        n = B * H * W
        cnt_h = int(ops.fb_metrics(f12, None, H, W, raw=True)[2].item())
        # the torch route's count from its boolean map (its float32 mean cannot resolve one pixel at these sizes)
        up = V.upsample_flow_to(f12, H, W)
        yy, xx = torch.meshgrid(torch.linspace(-1.0, 1.0, H, device=gpu_device), torch.linspace(-1.0, 1.0, W, device=gpu_device), indexing="ij")
        x, y = xx + 2.0 * up[:, 0] / (W - 1), yy + 2.0 * up[:, 1] / (H - 1)
        cnt_t = int(((x < -1) | (x > 1) | (y < -1) | (y > 1)).sum().item())
        assert abs(cnt_h - cnt_t) <= knife and abs(ot.item() - cnt_t / n) <= 1e-6
        assert torch.equal(V.oob_ratio(f12, H, W, device=gpu_device, dtype=torch.float32), oh)
        assert torch.equal(V.oob_ratio(f12, H, W, route="torch"), ot)


def test_deterministic(gpu_device):
    from opticalflow_amd import ops
    f12, f21 = (t.to(gpu_device) for t in _pair(4, 384, 512, 41, True))
    a = ops.fb_metrics(f12, f21, 384, 512, raw=True)
    b = ops.fb_metrics(f12, f21, 384, 512, raw=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # views of a larger batch (what flow_pair returns) give the values of their dense copies
    both = torch.cat((f12, f21), 0)
    c = ops.fb_metrics(both[:4], both[4:], 384, 512, raw=True)
    for x, y in zip(a, c):
        assert torch.equal(x, y)


def test_memory_peak(gpu_device):
    from opticalflow_amd import ops, validation as V
    B, H, W = 4, 384, 512
    f12, f21 = (t.to(gpu_device) for t in _pair(B, H, W, 51, True))
    peaks = {}
    for route in ("hip", "torch"):
        V.cycle_and_oob(f12, f21, H, W, route=route)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        res = V.cycle_and_oob(f12, f21, H, W, route=route)
        torch.cuda.synchronize()
        peaks[route] = torch.cuda.max_memory_allocated() - base
        del res
    ws = ops.fb_metrics_workspace_bytes(B, H, W)
    print("cycle + oob peak above the inputs: hip %d B (workspace %d B), torch %.1f MiB" % (peaks["hip"], ws, peaks["torch"] / 2 ** 20))
    # the workspace, the float32 [2] result, each rounded up to the allocator's 512-byte blocks: nothing image-sized
    assert peaks["hip"] <= ws + 2048
    assert peaks["hip"] < B * 2 * H * W * 4 and peaks["torch"] >= 4 * B * 2 * H * W * 4
    assert peaks["hip"] * 50 < peaks["torch"]


def test_decline_routes_match_torch(gpu_device):
    from opticalflow_amd import validation as V
    f12, f21 = (t.to(gpu_device) for t in _pair(2, 64, 96, 61, True))
    H, W = 64, 96
    cases = [(f12.double(), f21.double(), H, W),                              # float64
             (f12.half(), f21.half(), H, W),                                  # fp16 outside autocast
             (f12.bfloat16(), f21.bfloat16(), H, W),
             (f12, f21[:, :, :8, :12], H, W),                                 # flows of different sizes
             (f12, f21, 8, 96), (f12, f21, 64, 12),                           # H < h, W < w
             (f12[:, :, :1], f21[:, :, :1], H, W),                            # h < 2
             (f12.cpu(), f21.cpu(), H, W),                                    # off the device
             (f12.clone().requires_grad_(True), f21, H, W)]                   # requires grad with grad mode on
    for a, b, hh, ww in cases:
        assert not V._hip_applies("hip", a, b, hh, ww)
        with torch.no_grad():
            want = (V.cycle_torch(a, b, hh, ww), V.oob_torch(a, hh, ww))
        got = V.cycle_and_oob(a, b, hh, ww, route="hip")
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and (torch.equal(x, y) or (torch.isnan(x) and torch.isnan(y)))
    assert V._hip_applies("hip", f12, f21, H, W)
    with torch.no_grad():
        assert V._hip_applies("hip", f12.clone().requires_grad_(True), f21, H, W)
    # under autocast half-precision flows are cast to float32 and take the kernel
    with torch.autocast("cuda", dtype=torch.float16):
        assert V._hip_applies("hip", f12.half(), f21.half(), H, W)
        c16, o16 = V.cycle_and_oob(f12.half(), f21.half(), H, W)
    c32, o32 = V.cycle_and_oob(f12.half().float(), f21.half().float(), H, W)
    assert c16.dtype == torch.float32 and torch.equal(c16, c32) and torch.equal(o16, o32)


# ---------------------------------------------------------------- flow_pair
def _net(variant, dev, seed=3, **kw):
    from opticalflow_amd import PWCDCNet, PWCDCNet_old
    from opticalflow_amd.weights import synthetic_state_dict
    net = (PWCDCNet if variant == "dc" else PWCDCNet_old)(**kw)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=seed, gain=0.85, bias_std=0.02))
    return net.to(dev).eval()


def _images(B, H, W, seed, dev):
    img1 = seeded_rand((B, 3, H, W), seed, 0, 1)
    img2 = torch.roll(img1, shifts=(2, -3), dims=(2, 3)) * 0.9 + 0.1 * seeded_rand((B, 3, H, W), seed + 1, 0, 1)
    return img1.to(dev), img2.to(dev)


@pytest.mark.parametrize("variant", ["dc", "old"])
@pytest.mark.parametrize("B,H,W", [(1, 448, 1024), (4, 448, 1024), (4, 128, 192), (1, 128, 192)])
def test_flow_pair_matches_two_forwards(gpu_device, variant, B, H, W):
    net = _net(variant, gpu_device)
    img1, img2 = _images(B, H, W, 70 + B, gpu_device)
    f12, f21 = net.flow_pair(img1, img2)
    r12, r21 = net(torch.cat((img1, img2), 1)), net(torch.cat((img2, img1), 1))
    assert f12.shape == f21.shape == r12.shape == (B, 2, H // 4, W // 4)
    assert r12.abs().max().item() > 1e-2 and not torch.equal(r12, r21)
    d = max((f12 - r12).abs().max().item(), (f21 - r21).abs().max().item())
    print("%s %dx%dx%d: flow_pair vs two forwards max |diff| %.3e px (max |flow| %.3f)" % (variant, B, H, W, d, r12.abs().max().item()))
    assert d < 1e-4
    plan = net._plans[net._pair_key(img1)]
    assert not plan.c1_in_arena
    from opticalflow_amd.engine import PwcPlan
    seen, pyr = [], PwcPlan._pyramid
    PwcPlan._pyramid = lambda self, images, lo, hi: (seen.append(hi - lo), pyr(self, images, lo, hi))[1]
    try:
        net.flow_pair(img1, img2)
    finally:
        PwcPlan._pyramid = pyr
    assert seen == [2 * B]                                                  # every image through conv1a..conv6b exactly once
    assert net._key(torch.cat((img1, img2), 1)) in net._plans               # the forward's plan lives next to it under its own key


def test_flow_pair_options(gpu_device):
    """md, normalize_corr, align_corners and a trainable model (training mode, under no_grad) as PwcPlan covers them"""
    img1, img2 = _images(2, 128, 192, 80, gpu_device)
    for kw in (dict(normalize_corr=True), dict(align_corners=True), dict(md=3), dict(trainable=True)):
        net = _net("dc", gpu_device, **kw)
        if kw.get("trainable"):
            net.train()
        with torch.no_grad():
            f12, f21 = net.flow_pair(img1, img2)
        assert net.training == bool(kw.get("trainable"))
        net.eval()
        r12, r21 = net(torch.cat((img1, img2), 1)), net(torch.cat((img2, img1), 1))
        assert not f12.requires_grad
        assert max((f12 - r12).abs().max().item(), (f21 - r21).abs().max().item()) < 1e-4, kw


def test_flow_pair_follows_weight_updates(gpu_device):
    net = _net("dc", gpu_device, trainable=True)
    img1, img2 = _images(2, 128, 192, 90, gpu_device)
    before = net.flow_pair(img1, img2)
    plan = net._plans[net._pair_key(img1)]
    assert net.flow_pair(img1, img2)[0].data_ptr() != before[0].data_ptr() and net._plans[net._pair_key(img1)] is plan
    with torch.no_grad():                                                   # in-place, as optimizer.step() updates them
        for p in net.parameters():
            p.mul_(1.03)
    after = net.flow_pair(img1, img2)
    assert net._plans[net._pair_key(img1)] is not plan                      # the in-place update dropped the cached plan
    r12, r21 = net(torch.cat((img1, img2), 1)), net(torch.cat((img2, img1), 1))
    assert (after[0] - before[0]).abs().max().item() > 1e-4
    assert max((after[0] - r12).abs().max().item(), (after[1] - r21).abs().max().item()) < 1e-4


@pytest.mark.parametrize("precision", ["fp16", "fp16-strict"])
def test_flow_pair_half_precision_is_two_forwards(gpu_device, precision):
    net = _net("dc", gpu_device, precision=precision)
    img1, img2 = _images(2, 128, 192, 95, gpu_device)
    f12, f21 = net.flow_pair(img1, img2)
    assert torch.equal(f12, net(torch.cat((img1, img2), 1))) and torch.equal(f21, net(torch.cat((img2, img1), 1)))
    assert net._pair_key(img1) not in net._plans


# ---------------------------------------------------------------- validate
@pytest.mark.parametrize("variant", ["pseudo", "fundamental"])
def test_validate_is_the_composition_of_its_parts(gpu_device, variant):
    from opticalflow_amd import validation as V
    from opticalflow_amd.engine import PwcPlan
    from opticalflow_amd.losses import ProxyLabelLoss
    net = _net("dc", gpu_device)
    crit = ProxyLabelLoss(variant=variant, route="hip")
    B, H, W = 2, 128, 192
    loader = [tuple(t.cpu() for t in _images(B, H, W, 100 + 2 * i, gpu_device)) for i in range(3)]
    V.validate(net, loader[:1], crit, gpu_device)                          # builds the plan
    counts = {"images": 0, "forwards": 0}
    pyr, run = PwcPlan._pyramid, PwcPlan.run

    def counting_pyramid(self, images, lo, hi):
        counts["images"] += hi - lo
        return pyr(self, images, lo, hi)

    def counting_run(self, x):
        counts["forwards"] += 1
        return run(self, x)

    PwcPlan._pyramid, PwcPlan.run = counting_pyramid, counting_run
    try:
        got = V.validate(net, loader, crit, gpu_device, route="hip")
    finally:
        PwcPlan._pyramid, PwcPlan.run = pyr, run
    assert counts == {"images": 3 * 2 * B, "forwards": 0}                  # one pyramid pass per image, no ordinary forward
    sums = [0.0, 0.0, 0.0, 0.0]
    for img1, img2 in loader:
        img1, img2 = img1.to(gpu_device), img2.to(gpu_device)
        f12, f21 = net.flow_pair(img1, img2)
        _, photo, smooth = crit(f12, img1, img2)
        fb, oob = V.cycle_and_oob(f12, f21, H, W)
        for i, t in enumerate((photo, smooth, fb, oob)):
            sums[i] += float(t.item())
    want = dict(zip(("val_photo", "val_smooth", "val_fb", "val_oob"), (s / 3 for s in sums)))
    print(got)
    assert got == want and all(np.isfinite(v) for v in got.values()) and got["val_fb"] > 0
    # the scripts' names
    c = V.forward_backward_cycle(net, *(t.to(gpu_device) for t in loader[0]))
    f12, f21 = net.flow_pair(*(t.to(gpu_device) for t in loader[0]))
    assert c.dim() == 0 and torch.equal(c, V.cycle_and_oob(f12, f21, H, W)[0])
    assert torch.equal(c, V._forward_backward_consistency(net, *(t.to(gpu_device) for t in loader[0]), crit.warp))
    # the torch route runs the scripts' three forwards per batch (its values are compared with the scripts' arithmetic in
    # tests/test_validation_cpu.py; here they are printed beside the HIP route's)
    PwcPlan.run = counting_run
    try:
        ref = V.validate(net, loader, ProxyLabelLoss(variant=variant, route="torch"), gpu_device, route="torch")
    finally:
        PwcPlan.run = run
    assert counts["forwards"] == 9
    print(ref)
