#!/usr/bin/env python3
"""Validation without ground truth (train_pseudo.py:289-341, train_fundamental.py:503-536) at 4x3x384x512 and 16x3x448x1024, fp32,
HIP events after warm-up, windows of at least 0.5 s.  The baseline of every line is the torch / parent route measured in the
same run:
  (a) the fused cycle + out-of-bounds kernel (ops.fb_metrics) against the torch chain on the same two flows, with the kernel's
      algorithmic bytes (both quarter-resolution flows read once, nothing written) as a share of the 8 TB/s HBM peak;
  (b) PWCDCNet.flow_pair (one pyramid pass per image, one decoder pass at batch 2B) against two ordinary forwards;
  (c) one whole validation batch, validation.validate on a one-batch loader, route "hip" against route "torch" (three forwards
      plus the torch metric chain: the only way before flow_pair existed), both with the HIP ProxyLabelLoss as criterion, which
      the library already had; the torch route with the torch criterion is printed beside it.
Each comparison is timed twice, alternating the two sides, and both readings are printed."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import PWCDCNet, ops, validation as V  # noqa: E402
from opticalflow_amd.losses import ProxyLabelLoss  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, min_s=0.5):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    n, ms = 1, 0.0
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_s * 1e3:
            return ms * 1e3 / n                     # microseconds per call
        n = max(n * 2, int(n * min_s * 1e3 / max(ms, 1e-3) * 1.1))


def ab(new, base):
    """two alternating readings of each side: ((new1, new2), (base1, base2)) in microseconds"""
    n1, b1 = timed(new), timed(base)
    n2, b2 = timed(new), timed(base)
    return (n1, n2), (b1, b2)


def line(tag, what, new, base, extra=""):
    print("%-22s %-30s hip %9.1f / %9.1f us  torch %9.1f / %9.1f us  speedup %5.2fx%s"
          % (tag, what, new[0], new[1], base[0], base[1], min(base) / min(new), extra))


def main():
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).eval()
    crit_hip, crit_torch = ProxyLabelLoss(route="hip"), ProxyLabelLoss(route="torch")
    for B, H, W in ((4, 384, 512), (16, 448, 1024)):
        tag = "%dx3x%dx%d" % (B, H, W)
        h, w = H // 4, W // 4
        g = torch.Generator(device=dev).manual_seed(0)
        img1 = torch.rand(B, 3, H, W, device=dev, generator=g)
        img2 = torch.roll(img1, shifts=(2, -3), dims=(2, 3)) * 0.9 + 0.1 * torch.rand(B, 3, H, W, device=dev, generator=g)
        with torch.no_grad():
            f12, f21 = net.flow_pair(img1, img2)
            # (a) on the model's own two flows
            new, base = ab(lambda: ops.fb_metrics(f12, f21, H, W), lambda: V.cycle_and_oob(f12, f21, H, W, route="torch"))
            alg = 2 * B * 2 * h * w * 4 + 8
            t = min(new) * 1e-6
            line(tag, "(a) cycle + oob on two flows", new, base,
                 "  %.2f MB algorithmic = %.3f%% of 8 TB/s" % (alg / 1e6, 100.0 * alg / t / 8e12))
            # (b)
            x12, x21 = torch.cat((img1, img2), 1), torch.cat((img2, img1), 1)
            new, base = ab(lambda: net.flow_pair(img1, img2), lambda: (net(x12), net(x21)))
            line(tag, "(b) flow_pair vs two forwards", new, base)
            one = timed(lambda: net(x12))
            print("%-22s %-30s one ordinary forward %9.1f us" % (tag, "", one))
            # (c)
            loader = [(img1, img2)]
            new, base = ab(lambda: V.validate(net, loader, crit_hip, dev, route="hip"),
                           lambda: V.validate(net, loader, crit_hip, dev, route="torch"))
            line(tag, "(c) one validation batch", new, base, "  (both sides with the HIP ProxyLabelLoss, which predates flow_pair)")
            allt = timed(lambda: V.validate(net, loader, crit_torch, dev, route="torch"))
            print("%-22s %-30s torch route with the torch ProxyLabelLoss as well %9.1f us" % (tag, "", allt))
            d = max((f12 - net(x12)).abs().max().item(), (f21 - net(x21)).abs().max().item())
            vh, vt = V.validate(net, loader, crit_hip, dev, route="hip"), V.validate(net, loader, crit_torch, dev, route="torch")
            print("%-22s results: flow_pair vs two forwards max |diff| %.2e px; validate hip %s torch %s" % (tag, d, vh, vt))


if __name__ == "__main__":
    main()
