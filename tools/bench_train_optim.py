#!/usr/bin/env python3
"""One train2.py-shaped step (PWCDCNet(trainable=True) forward, supervised multiscale loss, backward, gradient clip to norm 1, AdamW) in
one process with each optimizer:
  fused          opticalflow_amd.FusedAdamW(max_grad_norm=1.0)
  torch-foreach  clip_grad_norm_(1.0) + torch.optim.AdamW                (torch's default)
  torch-fused    clip_grad_norm_(1.0) + torch.optim.AdamW(fused=True)
Batch 4 at 384x768 by default (PWC_BENCH_TRAIN=B,H,W).  Every optimizer has its own network; after three warm-up steps each, the
three alternate for PWC_BENCH_ROUNDS rounds (default 5) of PWC_BENCH_STEPS steps (default 10) between HIP events.  The table gives the
median ms/step with the range over the rounds: a difference inside that range is run-to-run spread, not a result."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import FusedAdamW, pwcnet  # noqa: E402
from opticalflow_amd.losses import supervised_multiscale_loss  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
B, H, W = [int(v) for v in os.environ.get("PWC_BENCH_TRAIN", "4,384,768").split(",")]
ROUNDS = int(os.environ.get("PWC_BENCH_ROUNDS", "5"))
STEPS = int(os.environ.get("PWC_BENCH_STEPS", "10"))
HP = dict(lr=1e-4, weight_decay=1e-6)


def make(kind):
    net = pwcnet.PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).train()
    if kind == "fused":
        opt = FusedAdamW(net.parameters(), max_grad_norm=1.0, **HP)
    else:
        opt = torch.optim.AdamW(net.parameters(), fused=(kind == "torch-fused") or None, **HP)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.rand(B, 6, H, W, device=dev, generator=g) * 4.7 - 2.1
    flow_gt = torch.randn(B, 2, H, W, device=dev, generator=g) * 5
    valid = (torch.rand(B, 1, H, W, device=dev, generator=g) > 0.3).float()

    def step():
        opt.zero_grad(set_to_none=True)
        supervised_multiscale_loss(net(x), x, flow_gt, valid).backward()
        if kind != "fused":
            torch.nn.utils.clip_grad_norm_(net.parameters(), 1.0)
        opt.step()
    return step


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


if __name__ == "__main__":
    steps = {k: make(k) for k in ("fused", "torch-foreach", "torch-fused")}
    for fn in steps.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(ROUNDS):
        for k, fn in steps.items():
            ms[k].append(timed(fn, STEPS))
    print("train2.py-shaped step %dx%dx%d, %d rounds x %d steps, optimizers alternating" % (B, H, W, ROUNDS, STEPS))
    print("%-14s %10s %9s %9s %10s" % ("optimizer", "median ms", "min ms", "max ms", "pairs/s"))
    for k, v in ms.items():
        m = statistics.median(v)
        print("%-14s %10.2f %9.2f %9.2f %10.1f" % (k, m, min(v), max(v), B / (m * 1e-3)))
    spread = max((max(v) - min(v)) / statistics.median(v) for v in ms.values())
    d = statistics.median(ms["fused"]) / statistics.median(ms["torch-foreach"]) - 1.0
    print("fused vs torch-foreach: %+.2f %% ms/step; largest run-to-run range of one optimizer: %.2f %% of its median" % (100 * d, 100 * spread))
