"""F(4x4) Winograd on stacked tile groups (pwc_conv_wino4.hip, Geo4 with IH > 0): several short images per workgroup, each staged with
its own zero border.  The two launches the fp32 plan makes with them -- dc_conv4 (128 -> 96, its last 32 couts stacked two 14x32 images
per workgroup, stored as pixel lattices) and dc_conv5 (96 -> 64 on 7x16 images, four per workgroup) -- against float64 per element, an
image's result against its slot in the batch, and the whole forward against the 3-level lattice context (option "w4_stacked" = 0)."""
import random

import pytest
import torch

import launch_audit as LA
from oracle import pwc_oracle as O

pytestmark = pytest.mark.gpu

# (name, cin, cout, h, w, split2, images per network batch item at 448x1024)
LAYERS = {"dc_conv4": (128, 96, 14, 32, True, 64), "dc_conv5": (96, 64, 7, 16, False, 256)}


def _layer(name, n, seed, device):
    """n images with different content everywhere (borders included), filters, bias, packed bank, workspace"""
    cin, cout, h, w, split2, _ = LAYERS[name]
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, cin, h, w, generator=g) * 2 - 1).to(device)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(device)
    b = (torch.randn(cout, generator=g) * 0.05).to(device)
    return x, wt, b


def _run(x, wt, b, split2):
    from opticalflow_amd import ops
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    nbytes = ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, cout)
    ws = torch.empty((max(nbytes, 4) // 4,), dtype=torch.float32, device=x.device)
    out = ops.conv3x3_wino4(x, ops.pack_conv3x3_wino4(wt), b, cout, leaky_slope=LA.LEAKY, split2=split2, workspace=ws)
    torch.cuda.synchronize()
    return out


def _check(name, x, wt, b, out, imgs):
    split2 = LAYERS[name][4]
    got = torch.cat([out[4 * i:4 * i + 4] for i in imgs]).cpu() if split2 else out[imgs].cpu()
    ref, s = LA.conv_ref(x[imgs].cpu(), wt.cpu(), b.cpu())
    if split2:
        ref, s = LA.split2(ref), LA.split2(s)
    r, idx, chans = LA.worst(LA.bounded_ratio(got, ref, s, LA.REL_WINO4))
    assert r <= 1.0, "%s: %.2f x the bound at %s (channels %s)" % (name, r, idx, chans)
    return r


@pytest.mark.parametrize("name", sorted(LAYERS))
@pytest.mark.parametrize("B", [1, 2, 16, 32])
def test_stacked_launch_vs_fp64(gpu_device, name, B):
    """the launch of a batch-B forward at 448x1024 (64B / 256B lattice images), per element within REL_WINO4 x (sum |x||w| + |b|) on
    every position of a group of images, the first and last groups and seeded others"""
    from opticalflow_amd import ops
    cin, cout, h, w, split2, per_item = LAYERS[name]
    n = per_item * B
    x, wt, b = _layer(name, n, 100 + B, gpu_device)
    out = _run(x, wt, b, split2)
    rng = random.Random(B)
    imgs = sorted({0, 1, 2, 3, n - 4, n - 3, n - 2, n - 1, *rng.sample(range(n), 4)})
    r = _check(name, x, wt, b, out, imgs)
    print("%s B=%d (%d images): worst %.3f of the bound, workspace %d B" % (name, B, n, r, ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, cout)))
    if B >= 2:      # the rule takes the launch from batch 2 on (batch 1: the 32-cout launch would not cover the chip)
        assert ops.conv3x3_wino4_preferred(n, cin, h, w, cout)


@pytest.mark.parametrize("name", sorted(LAYERS))
@pytest.mark.parametrize("n", [1, 3, 5])
def test_stacked_launch_partial_group(gpu_device, name, n):
    """image counts that leave the last workgroup's group short: the missing images are neither read nor written"""
    split2 = LAYERS[name][4]
    x, wt, b = _layer(name, n, 7 + n, gpu_device)
    cout, h, w = LAYERS[name][1], LAYERS[name][2], LAYERS[name][3]
    from opticalflow_amd import ops
    shape = (4 * (n + 1), cout, h // 2, w // 2) if split2 else (n + 1, cout, h, w)
    buf = torch.full(shape, 1234.5, device=gpu_device)
    out = buf[:4 * n] if split2 else buf[:n]
    ops.conv3x3_wino4(x, ops.pack_conv3x3_wino4(wt), b, cout, leaky_slope=LA.LEAKY, split2=split2, out=out)
    torch.cuda.synchronize()
    _check(name, x, wt, b, out, list(range(n)))
    assert bool((buf[out.shape[0]:] == 1234.5).all()), "a store past the last image"


@pytest.mark.parametrize("name", sorted(LAYERS))
@pytest.mark.parametrize("B", [1, 16])
def test_stacked_batch_slot_invariance(gpu_device, name, B):
    """the same image in slot 0 and slot 15 (another place in its group, other neighbours) gives the same bits"""
    split2, per_item = LAYERS[name][4], LAYERS[name][5]
    n = per_item * B
    x, wt, b = _layer(name, n, 55, gpu_device)
    x[15] = x[0]
    out = _run(x, wt, b, split2)
    if split2:
        assert torch.equal(out[0:4], out[60:64])
    else:
        assert torch.equal(out[0], out[15])


def _forward(device, stacked, x, B):
    from opticalflow_amd import PWCDCNet, _lib
    from opticalflow_amd.weights import synthetic_state_dict
    saved = _lib.get_option("w4_stacked")
    try:
        _lib.set_option("w4_stacked", stacked)
        net = PWCDCNet()
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
        net = net.to(device).eval()
        out = net(x).clone()
        plan = net._plan_for(x)
        assert plan.ctx_lattice and plan.ctx_lattice4 == bool(stacked)
        return out
    finally:
        _lib.set_option("w4_stacked", saved)


@pytest.mark.parametrize("B", [2, 16])
def test_forward_stacked_context_matches_three_level_context(gpu_device, B):
    """dc_conv4 / dc_conv5 on the level-4 lattices (default) against the round-4 path (dc_conv4 as 64 F(4x4) + 32 F(2x2) couts, dc_conv5 as
    a dilation-2 direct convolution): the bound of test_forward_context_lattice_layout_matches_plain_layout; items of one batch with the
    same input give the same bits"""
    x = torch.rand(B, 6, 448, 1024, generator=torch.Generator().manual_seed(4321)).to(gpu_device)
    x[B - 1] = x[0]
    new = _forward(gpu_device, 1, x, B)
    old = _forward(gpu_device, 0, x, B)
    d = O.epe(new.cpu(), old.cpu())
    print("B=%d: stacked context vs 3-level context: EPE %.3e" % (B, d))
    assert d < 2e-5
    assert torch.equal(new[0], new[B - 1])
