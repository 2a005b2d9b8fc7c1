#!/usr/bin/env python3
"""One train.py step (PWCDCNet(trainable=True) forward, MaskedCharbonnier on flow2 upsampled to the GT, backward, Adam step) in
pairs/s, with the fused HIP loss (route="hip") and the torch chain (route="torch").  Batch 4 at 320x896 by default
(PWC_BENCH_TRAIN=B,H,W); three warm-up steps, then PWC_BENCH_STEPS timed steps between HIP events."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import pwcnet  # noqa: E402
from opticalflow_amd.losses import MaskedCharbonnier  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
B, H, W = [int(v) for v in os.environ.get("PWC_BENCH_TRAIN", "4,320,896").split(",")]
STEPS = int(os.environ.get("PWC_BENCH_STEPS", "10"))


def run(route):
    net = pwcnet.PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).train()
    opt = torch.optim.Adam(net.parameters(), lr=1e-5)
    loss_fn = MaskedCharbonnier(route=route)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, 6, H, W, device=dev, generator=g) * 4.7 - 2.1
    flow_gt = torch.randn(B, 2, H, W, device=dev, generator=g) * 5
    valid = (torch.rand(B, 1, H, W, device=dev, generator=g) > 0.3).float()

    def step():
        opt.zero_grad(set_to_none=True)
        flow2, *_ = net(x)
        loss_fn(flow2, flow_gt, valid).backward()
        opt.step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        step()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / STEPS
    return ms, B / (ms * 1e-3)


if __name__ == "__main__":
    r = {route: run(route) for route in ("hip", "torch")}
    for route, (ms, ps) in r.items():
        print("train.py step %dx%dx%d loss route %-5s %7.2f ms/step  %6.1f pairs/s" % (B, H, W, route, ms, ps))
    print("speedup of the step: %.3fx" % (r["torch"][0] / r["hip"][0]))
