#!/usr/bin/env python3
"""Training step (forward + backward + SGD step) of PWCDCNet(trainable=True) in pairs/s at train.py's shape (batch 4, 320x896),
HIP events: the fused cost-volume route (ops.WarpCorrelationFunction: fused forward, pwc_warp_corr81_bwd backward) against the
same eager composition with every cost volume done by the separate operators (warp -> correlation -> LeakyReLU, each with its
own backward: WarpFunction / pwc_corr_bwd / torch's LeakyReLU).  The convolutions are nn.Conv2d on PyTorch-ROCm in both.
Three warm-up steps, a 1 s pause, then PWC_BENCH_STEPS timed steps (see tools/train_step_share.py for a trace of those alone)."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import ops, pwcnet  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
B, H, W = [int(v) for v in os.environ.get("PWC_BENCH_TRAIN", "4,320,896").split(",")]
STEPS = int(os.environ.get("PWC_BENCH_STEPS", "10"))


class _CorrFunction(torch.autograd.Function):
    """correlation with pwc_corr_bwd as its backward (the separate operator of the old route)."""

    @staticmethod
    def forward(ctx, a, b, normalize):
        ctx.save_for_backward(a, b)
        ctx.normalize = normalize
        return ops.correlation(a, b, 4, 1, 4, 1, 1, 1.0, normalize)

    @staticmethod
    def backward(ctx, gy):
        a, b = ctx.saved_tensors
        g1, g2 = ops.correlation_backward(a, b, gy.contiguous(), normalize=ctx.normalize)
        return g1, g2, None


class _Separate:
    """stands in for ops.WarpCorrelationFunction: warp, correlation and LeakyReLU as three autograd nodes."""

    @staticmethod
    def apply(c1, c2, flo, scale, align, thr, mult, normalize, slope):
        w2 = ops.WarpFunction.apply(c2.contiguous(), flo.contiguous(), scale, align, thr) if flo is not None else c2.contiguous()
        return torch.nn.functional.leaky_relu(_CorrFunction.apply(c1.contiguous(), w2, normalize), slope)


def run(route):
    net = pwcnet.PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-6, momentum=0.9)
    x = torch.rand(B, 6, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    target = torch.zeros(B, 2, H // 4, W // 4, device=dev)
    saved = ops.WarpCorrelationFunction
    if route == "separate":
        pwcnet.ops.WarpCorrelationFunction = _Separate
    try:
        def step():
            opt.zero_grad(set_to_none=True)
            flows = net(x)
            loss = (flows[0] - target).abs().mean() + sum(0.1 * f.abs().mean() for f in flows[1:])
            loss.backward()
            opt.step()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        # idle gap between warm-up (MIOpen's solver search runs there) and the timed steps: tools/train_step_share.py cuts a
        # kernel trace at it; outside the timed region, so it does not change the figure below
        time.sleep(1.0)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(STEPS):
            step()
        e.record()
        e.synchronize()
        ms = s.elapsed_time(e) / STEPS
    finally:
        pwcnet.ops.WarpCorrelationFunction = saved
    return ms


if __name__ == "__main__":
    routes = sys.argv[1:] or ["fused", "separate"]
    for r in routes:
        ms = run(r)
        print("train step (%d,6,%d,%d) %-8s: %8.2f ms  %7.1f pairs/s" % (B, H, W, r, ms, B / ms * 1e3), flush=True)
