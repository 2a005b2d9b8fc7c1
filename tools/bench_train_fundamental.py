#!/usr/bin/env python3
"""One train_fundamental.py step (:438-497): PWCDCNet(trainable=True) forward, upsample to full resolution, per-sample epipolar
mask, fundamental proxy-label loss with that mask, soft Sampson penalty from a fit on sample 0, backward, SGD step.  Timed with
the HIP epipolar path (opticalflow_amd.epipolar) and with the float64 NumPy oracle building the mask and the soft fit on the
host (tests/epipolar_oracle.py: the reference's algorithm; a few steps only).  Batch 4 at 384x512, epi_stride 6, epi_thresh 0.3
by default (PWC_BENCH_TRAIN=B,H,W, PWC_BENCH_STRIDE, PWC_BENCH_STEPS, PWC_BENCH_ORACLE_STEPS)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opticalflow_amd import epipolar, pwcnet  # noqa: E402
from opticalflow_amd.losses import ProxyLabelLoss, upsample_flow_to  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402
import epipolar_oracle as O  # noqa: E402

dev = torch.device("cuda:0")
B, H, W = [int(v) for v in os.environ.get("PWC_BENCH_TRAIN", "4,384,512").split(",")]
STRIDE = int(os.environ.get("PWC_BENCH_STRIDE", "6"))
STEPS = int(os.environ.get("PWC_BENCH_STEPS", "10"))
ORACLE_STEPS = int(os.environ.get("PWC_BENCH_ORACLE_STEPS", "2"))


def run(route, steps):
    net = pwcnet.PWCDCNet(trainable=True)
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=1e-5, momentum=0.9)
    crit = ProxyLabelLoss(variant="fundamental", route="hip")
    x = torch.rand(B, 6, H, W, device=dev) * 4.7 - 2.1

    def step():
        opt.zero_grad(set_to_none=True)
        flow_pred = net(x)[0]
        flow_full = upsample_flow_to(flow_pred, H, W)
        if route == "hip":
            keep = epipolar.build_epipolar_mask_from_flow(flow_full, tau=0.3, stride=STRIDE)
            Fs, ok = epipolar.ransac_fundamental(flow_full[0:1], STRIDE, 1.0, 1000, 0)
            F0, ok0 = Fs[0], ok[0]
        else:
            fl = flow_full.detach().cpu().numpy()
            keep = torch.from_numpy(np.stack([O.epipolar_mask(np.ascontiguousarray(fl[b].transpose(1, 2, 0)), 0.3, STRIDE)[0]
                                              for b in range(B)])[:, None]).to(dev)
            p1, p2 = O.flow_to_pairs(np.ascontiguousarray(fl[0].transpose(1, 2, 0)), STRIDE)
            fit = O.ransac(p1, p2, 1000, 1.0, 0)
            F0, ok0 = (fit["F"], True) if fit["ok"] else (np.zeros((3, 3)), False)
        total, _, _ = crit(flow_pred, x[:, :3], x[:, 3:], valid_mask=keep)
        total = total + epipolar.epipolar_sampson_loss(flow_full, F0, valid_mask=keep, weight=0.1, ok=ok0)
        total.backward()
        opt.step()

    for _ in range(2 if route == "hip" else 1):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / steps
    return ms, B / (ms * 1e-3)


if __name__ == "__main__":
    r = {"hip": run("hip", STEPS), "oracle-mask": run("oracle", ORACLE_STEPS)}
    for route, (ms, ps) in r.items():
        print("train_fundamental step %dx%dx%d stride %d mask route %-11s %9.2f ms/step  %7.2f pairs/s" % (B, H, W, STRIDE, route, ms, ps))
    print("speedup of the step: %.1fx" % (r["oracle-mask"][0] / r["hip"][0]))
