#!/usr/bin/env python3
"""One train_pseudo.py step (PWCDCNet(trainable=True) forward, ProxyLabelLoss on flow2, backward, SGD step) in pairs/s, with the
fused HIP loss (route="hip") and the torch composition (route="torch").  Batch 4 at 384x512 by default (PWC_BENCH_TRAIN=B,H,W);
three warm-up steps, then PWC_BENCH_STEPS timed steps between HIP events."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import pwcnet  # noqa: E402
from opticalflow_amd.losses import ProxyLabelLoss  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
B, H, W = [int(v) for v in os.environ.get("PWC_BENCH_TRAIN", "4,384,512").split(",")]
STEPS = int(os.environ.get("PWC_BENCH_STEPS", "10"))


def run(route):
    net = pwcnet.PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-5, momentum=0.9)
    loss = ProxyLabelLoss(route=route)
    x = torch.rand(B, 6, H, W, device=dev) * 4.7 - 2.1

    def step():
        opt.zero_grad(set_to_none=True)
        total, _, _ = loss(net(x)[0], x[:, :3], x[:, 3:])
        total.backward()
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
        print("train_pseudo step %dx%dx%d loss route %-5s %7.2f ms/step  %6.1f pairs/s" % (B, H, W, route, ms, ps))
    print("speedup of the step: %.3fx" % (r["torch"][0] / r["hip"][0]))
