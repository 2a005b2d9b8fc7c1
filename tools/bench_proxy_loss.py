#!/usr/bin/env python3
"""Proxy-label loss (train_pseudo.py:65-164) forward and forward+backward, fused HIP route (ops.ProxyLossFunction) against the
torch composition (losses.proxy_loss_torch), HIP events, at train_pseudo's 4x3x384x512 and 16x3x448x1024 (flow at 1/4).
Warm-up, then a window of at least 0.5 s per measurement.  Prints the algorithmic bytes of the fused route (inputs read once,
grad_up written and read back, grad_flow written), its fraction of 8 TB/s and the speedup over the torch route."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd.losses import ProxyLabelLoss  # noqa: E402

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


def main():
    for B, C, H, W in ((4, 3, 384, 512), (16, 3, 448, 1024)):
        h, w = H // 4, W // 4
        g = torch.Generator(device=dev).manual_seed(0)
        img1 = torch.rand(B, C, H, W, device=dev, generator=g) * 4.7 - 2.1
        img2 = torch.rand(B, C, H, W, device=dev, generator=g) * 4.7 - 2.1
        flow = (torch.randn(B, 2, h, w, device=dev, generator=g) * 2).requires_grad_(True)
        res = {}
        for route in ("hip", "torch"):
            loss = ProxyLabelLoss(route=route)

            def fwd():
                with torch.no_grad():
                    loss(flow, img1, img2)

            def fwdbwd():
                flow.grad = None
                loss(flow, img1, img2)[0].backward()

            res[route] = (timed(fwd), timed(fwdbwd))
        fb_in = 2 * B * C * H * W * 4 + B * 2 * h * w * 4
        fwd_bytes = fb_in
        bwd_bytes = fb_in + 2 * B * 2 * H * W * 4 + 2 * B * 2 * h * w * 4
        for i, what, nbytes in ((0, "forward", fwd_bytes), (1, "forward+backward", fwd_bytes + bwd_bytes)):
            th, tt = res["hip"][i], res["torch"][i]
            print("%dx%dx%dx%d flow %dx%d %-17s hip %8.1f us  torch %8.1f us  speedup %5.2fx  %.1f MB algorithmic, %.1f%% of 8 TB/s"
                  % (B, C, H, W, h, w, what, th, tt, tt / th, nbytes / 1e6, 100.0 * nbytes / (th * 1e-6) / 8e12))


if __name__ == "__main__":
    main()
