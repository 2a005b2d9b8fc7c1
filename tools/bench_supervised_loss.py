#!/usr/bin/env python3
"""Supervised losses of train.py / train2.py, forward and forward+backward, fused HIP route (ops.FlowLossFunction /
ops.MultiscaleLossFunction) against the torch chain (route="torch"), HIP events; warm-up, then a window of at least 0.5 s per
measurement (the rules of tools/bench_proxy_loss.py).  Sizes: train.py's 4x320x896 with flow2 80x224 (MaskedCharbonnier on the
upsampled flow); train2.py's five levels at 4x384x768 (supervised_multiscale_loss, default weights, no regularisers); and
16x448x1024 with a 112x256 flow (both losses).  Prints the algorithmic bytes of the fused route and their fraction of 8 TB/s."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd.losses import MaskedCharbonnier, supervised_multiscale_loss  # noqa: E402

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


def report(label, res, fwd_bytes, fb_bytes):
    for i, what, nbytes in ((0, "forward", fwd_bytes), (1, "forward+backward", fb_bytes)):
        th, tt = res["hip"][i], res["torch"][i]
        print("%-34s %-17s hip %8.1f us  torch %8.1f us  speedup %5.2fx  %.1f MB algorithmic, %.2f%% of 8 TB/s"
              % (label, what, th, tt, tt / th, nbytes / 1e6, 100.0 * nbytes / (th * 1e-6) / 8e12))


def bench_flow(B, H, W, h, w):
    g = torch.Generator(device=dev).manual_seed(0)
    pred = (torch.randn(B, 2, h, w, device=dev, generator=g) * 3).requires_grad_(True)
    gt = torch.randn(B, 2, H, W, device=dev, generator=g) * 8
    valid = (torch.rand(B, 1, H, W, device=dev, generator=g) > 0.3).float()
    res = {}
    for route in ("hip", "torch"):
        loss = MaskedCharbonnier(route=route)

        def fwd():
            with torch.no_grad():
                loss(pred, gt, valid)

        def fwdbwd():
            pred.grad = None
            loss(pred, gt, valid).backward()

        res[route] = (timed(fwd), timed(fwdbwd))
    lo, full = B * 2 * h * w * 4, B * H * W * 4
    fwd_bytes = lo + 2 * full + full                               # pred, gt, mask read once
    bwd_bytes = fwd_bytes + 2 * B * 2 * H * w * 8 + lo             # + rows written and read back (fp64), grad written
    report("MaskedCharbonnier %dx%dx%d flow %dx%d" % (B, H, W, h, w), res, fwd_bytes, fwd_bytes + bwd_bytes)


def bench_multiscale(B, H, W):
    g = torch.Generator(device=dev).manual_seed(1)
    sizes = [(H // s, W // s) for s in (4, 8, 16, 32, 64)]
    preds = [(torch.randn(B, 2, h, w, device=dev, generator=g) * 2).requires_grad_(True) for h, w in sizes]
    gt = torch.randn(B, 2, H, W, device=dev, generator=g) * 8
    masks = (torch.rand(B, H, W, device=dev, generator=g) > 0.3).float()
    images = torch.rand(B, 6, H, W, device=dev, generator=g)
    res = {}
    for route in ("hip", "torch"):
        def fwd():
            with torch.no_grad():
                supervised_multiscale_loss(preds, images, gt, masks, route=route)

        def fwdbwd():
            for p in preds:
                p.grad = None
            supervised_multiscale_loss(preds, images, gt, masks, route=route).backward()

        res[route] = (timed(fwd), timed(fwdbwd))
    lo = sum(B * 2 * h * w * 4 for h, w in sizes)
    taps = sum(B * h * w * (2 * 4 + 1) * 4 for h, w in sizes)      # 4 GT taps per component + 1 mask tap per prediction pixel
    fwd_bytes = lo + taps
    report("multiscale 5 levels %dx%dx%d" % (B, H, W), res, fwd_bytes, 2 * fwd_bytes + lo)


def main():
    bench_flow(4, 320, 896, 80, 224)
    bench_multiscale(4, 384, 768)
    bench_flow(16, 448, 1024, 112, 256)
    bench_multiscale(16, 448, 1024)


if __name__ == "__main__":
    main()
