"""One direct launch per form of the two Winograd launchers (pwc_conv_wino4.hip launch_wino4, pwc_conv_wino.hip launch_wino): which
kernel instantiation the library reports for it (pwc_last_conv_kernel: name<template arguments>, "/split" where the launch went through
the split workspace) and the result against float64.  The rule and scratch queries are pure and pinned on the CPU
(test_wino_rules_cpu.py); what only the launcher decides -- the form per launch, the fallback without a sufficient workspace, the
cout ladder of F(2x2) -- shows in the label alone, and test_kernel_coverage asks for the SET of labels, not the label per form.

The expected labels are literals recorded on an MI355X (256 compute units) from the library as it stood before the launchers read
their layer plans (wino4_layer, wino_plan); a device with another count plans other splits, so the file skips there.
conv3x3_wino4p_kernel<CB, TG, GW, Cin slices, 1, IH>, conv3x3_wino8r_kernel<MT, TG, 1, dilation, 1, 0>; a layer of two or three launches
reports the last."""
import pytest
import torch

import launch_audit as LA

pytestmark = pytest.mark.gpu

W4 = "conv3x3_wino4p_kernel"
W2 = "conv3x3_wino8r_kernel"

# id: (B, Cin, H, W, Cout, split2, workspace: "need" = what the query asks for, None, "short" = one byte less, label)
CASES4 = {
    "64cout-8x64": (3, 32, 8, 64, 64, False, "need", W4 + "<4, 2, 64, 1, 1, 0>"),
    "64cout-16x64": (3, 32, 16, 64, 64, False, "need", W4 + "<4, 2, 64, 1, 1, 0>"),
    "32cout-8x64": (3, 32, 8, 64, 32, False, "need", W4 + "<2, 4, 64, 1, 1, 0>"),           # half-filled 16-row workgroups: still launched
    "32cout-16x64": (3, 32, 16, 64, 32, False, "need", W4 + "<2, 4, 64, 1, 1, 0>"),
    "64cout-16x32": (3, 32, 16, 32, 64, False, "need", W4 + "<4, 2, 32, 1, 1, 0>"),
    "64cout-32x32": (3, 32, 32, 32, 64, False, "need", W4 + "<4, 2, 32, 1, 1, 0>"),
    "32cout-16x32": (3, 32, 16, 32, 32, False, "need", W4 + "<2, 4, 32, 1, 1, 16>"),        # 16 of a workgroup's 32 rows: two images stacked
    "32cout-32x32": (3, 32, 32, 32, 32, False, "need", W4 + "<2, 4, 32, 1, 1, 0>"),
    "stack-7x16-b5": (5, 32, 7, 16, 64, False, "need", W4 + "<4, 2, 16, 1, 1, 8>"),         # four images per workgroup, the second group short
    "stack-14x32-b3": (3, 32, 14, 32, 32, False, "need", W4 + "<2, 4, 32, 1, 1, 16>"),
    "96cout-two-launches": (3, 32, 16, 64, 96, False, "need", W4 + "<2, 4, 64, 1, 1, 0>"),
    "ragged-cout40-cin37": (3, 37, 8, 64, 40, False, "need", W4 + "<4, 2, 64, 1, 1, 0>"),
    "split2-8x64": (3, 32, 8, 64, 64, True, "need", W4 + "<4, 2, 64, 1, 1, 0>"),
    "whole-launch-cin-split": (1, 192, 8, 64, 64, False, "need", W4 + "<4, 2, 64, 6, 1, 0>/split"),
    "whole-launch-no-workspace": (1, 192, 8, 64, 64, False, None, W4 + "<4, 2, 64, 1, 1, 0>"),
    "tail-split": (64, 96, 40, 64, 64, False, "need", W4 + "<4, 2, 64, 2, 1, 0>/split"),     # 320 workgroups: one full round + 64
    "tail-split-short-workspace": (64, 96, 40, 64, 64, False, "short", W4 + "<4, 2, 64, 1, 1, 0>"),
}

# id: (B, Cin, H, W, Cout, dilation, label); the workspace is always what the query asks for
CASES2 = {
    "128cout": (2, 32, 16, 32, 128, 1, W2 + "<4, 1, 1, 1, 1, 0>"),
    "64cout": (2, 32, 16, 32, 64, 1, W2 + "<2, 2, 1, 1, 1, 0>"),
    "32cout": (2, 32, 16, 32, 32, 1, W2 + "<1, 4, 1, 1, 1, 0>"),
    "96cout-single-width": (2, 32, 16, 32, 96, 1, W2 + "<1, 4, 1, 1, 1, 0>"),                # 3 x 32 in one launch
    "192cout-single-width": (2, 32, 16, 32, 192, 1, W2 + "<2, 2, 1, 1, 1, 0>"),              # 3 x 64 in one launch
    "96cout-ladder": (128, 32, 32, 32, 96, 1, W2 + "<1, 4, 1, 1, 1, 0>"),                    # 64 + 32: the 32-cout launch has 256 workgroups
    "160cout-ladder": (128, 32, 32, 32, 160, 1, W2 + "<1, 4, 1, 1, 1, 0>"),                  # 128 + 32
    "dilation2-odd-w": (2, 32, 16, 31, 64, 2, W2 + "<2, 2, 1, 2, 1, 0>"),
    "split-k": (32, 256, 16, 32, 128, 1, W2 + "<4, 1, 1, 1, 1, 0>/split"),                   # 128 workgroups, 64 chunks
}


@pytest.fixture(scope="module")
def device(gpu_device):
    cus = torch.cuda.get_device_properties(gpu_device).multi_processor_count
    if cus != 256:
        pytest.skip("the expected labels were recorded with 256 compute units; this device reports %d and plans other splits" % cus)
    return gpu_device


def _layer(B, cin, h, w, cout, seed, device):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(B, cin, h, w, generator=g) * 2 - 1).to(device)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(device)
    b = (torch.randn(cout, generator=g) * 0.05).to(device)
    return x, wt, b


def _workspace(kind, need, device):
    if kind is None:
        return None
    nbytes = need - 1 if kind == "short" else max(need, 16)
    assert kind != "short" or need > 16
    return torch.empty((nbytes,), dtype=torch.uint8, device=device)


def _within_bound(name, out, x, wt, b, dilation, rel, split2=False):
    imgs = LA.pick_images(x.shape[0], len(name))
    got = torch.cat([out[4 * i:4 * i + 4] for i in imgs]).cpu() if split2 else out[imgs].cpu()
    ref, s = LA.conv_ref(x[imgs].cpu(), wt.cpu(), b.cpu(), 1, dilation)
    if split2:
        ref, s = LA.split2(ref), LA.split2(s)
    r, idx, chans = LA.worst(LA.bounded_ratio(got, ref, s, rel))
    assert r <= 1.0, "%s: %.2f x the bound at %s (channels %s)" % (name, r, idx, chans)


@pytest.mark.parametrize("name", list(CASES4))
def test_wino4_launch_form(device, name):
    from opticalflow_amd import ops
    B, cin, h, w, cout, split2, ws_kind, label = CASES4[name]
    x, wt, b = _layer(B, cin, h, w, cout, 11, device)
    A = dict(x=x, cout=cout, workspace=_workspace(ws_kind, ops.conv3x3_wino4_workspace_bytes(B, cin, h, w, cout), device))
    out = ops.conv3x3_wino4(x, ops.pack_conv3x3_wino4(wt), b, cout, leaky_slope=LA.LEAKY, split2=split2, workspace=A["workspace"])
    got = LA.last_kernel(LA.used_split("conv3x3_wino4", A))
    torch.cuda.synchronize()
    print("%s: %s" % (name, got))
    assert got == label
    _within_bound(name, out, x, wt, b, 1, LA.REL_WINO4, split2)


@pytest.mark.parametrize("name", list(CASES2))
def test_wino2_launch_form(device, name):
    from opticalflow_amd import ops
    B, cin, h, w, cout, dilation, label = CASES2[name]
    x, wt, b = _layer(B, cin, h, w, cout, 12, device)
    A = dict(x=x, cout=cout, dilation=dilation,
             workspace=_workspace("need", ops.conv3x3_wino_workspace_bytes(B, cin, h, w, cout, dilation), device))
    out = ops.conv3x3_wino(x, ops.pack_conv3x3_wino(wt), b, cout, leaky_slope=LA.LEAKY, dilation=dilation, workspace=A["workspace"])
    got = LA.last_kernel(LA.used_split("conv3x3_wino", A))
    torch.cuda.synchronize()
    print("%s: %s" % (name, got))
    assert got == label
    _within_bound(name, out, x, wt, b, dilation, LA.REL_WINO2)
