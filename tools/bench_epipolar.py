#!/usr/bin/env python3
"""Epipolar mask and soft Sampson penalty (train_fundamental.py:169-382, csrc/pwc_epipolar.hip): HIP-event time of each entry
and of the whole per-step work of train_fundamental.py:459-483 (mask fit + distance/mask for B samples, soft fit on sample 0,
soft loss forward + backward), at 4x384x512 stride 6 and 16x448x1024 stride 4, on seeded rigid-scene flows.  The float64
NumPy oracle (tests/epipolar_oracle.py, the reference's algorithm) is timed on one sample of each shape on the host."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from opticalflow_amd import epipolar, ops  # noqa: E402
import epipolar_oracle as O  # noqa: E402

dev = torch.device("cuda:0")


def timed(fn, min_s=0.3):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= min_s * 1e3 or n >= 256:
            return ms / n
        n *= 2


def bench(B, H, W, stride, oracle):
    flows = np.stack([O.rigid_flow(H, W, 100 + b) for b in range(B)])
    f = torch.from_numpy(flows).to(dev)
    pts, n = ops.epipolar_pairs(f, stride)
    N = [int(v) for v in n.cpu()]
    idx = torch.stack([epipolar._device_table(v, 0, 2000, dev) for v in N])
    F, ok, best, counts = ops.epipolar_ransac(pts, n, idx, 0.5)
    mask, thr = ops.epipolar_mask(f, F, ok)
    g = torch.ones((), device=dev)
    t = {}
    t["pairs"] = timed(lambda: ops.epipolar_pairs(f, stride))
    t["ransac 2000 it"] = timed(lambda: ops.epipolar_ransac(pts, n, idx, 0.5))
    t["distance+mask"] = timed(lambda: ops.epipolar_mask(f, F, ok))
    t["loss fwd"] = timed(lambda: ops.epipolar_loss(f, F[0].view(3, 3), ok[0], mask))
    t["loss bwd"] = timed(lambda: ops.epipolar_loss_backward(f, F[0].view(3, 3), ok[0], mask, g))

    def step():
        fr = f.detach().requires_grad_(True)
        m = epipolar.build_epipolar_mask_from_flow(fr, 0.3, stride)
        Fs, oks = epipolar.ransac_fundamental(fr[0:1], stride, 1.0, 1000, 0)
        loss = epipolar.epipolar_sampson_loss(fr, Fs[0], valid_mask=m, weight=0.1, ok=oks[0])
        loss.backward()

    t["step (mask + soft fit + loss fwd/bwd)"] = timed(step)
    for k, v in t.items():
        print("%dx%dx%d s%d N=%d  %-38s %9.1f us" % (B, H, W, stride, N[0], k, v * 1e3))
    if oracle:
        hw2 = np.ascontiguousarray(flows[0].transpose(1, 2, 0))
        t0 = time.perf_counter()
        O.epipolar_mask(hw2, 0.3, stride)
        t1 = time.perf_counter()
        p1, p2 = O.flow_to_pairs(hw2, stride)
        O.ransac(p1, p2, 1000, 1.0, 0)
        t2 = time.perf_counter()
        host = B * (t1 - t0) + (t2 - t1)
        print("%dx%dx%d s%d  oracle (NumPy, one host thread pool): mask %.3f s/sample, soft fit %.3f s -> %.2f s per step; "
              "HIP step %.3f ms = %.0fx" % (B, H, W, stride, t1 - t0, t2 - t1, host, t[list(t)[-1]], host * 1e3 / t[list(t)[-1]]))


if __name__ == "__main__":
    bench(4, 384, 512, 6, oracle=True)
    bench(16, 448, 1024, 4, oracle=os.environ.get("PWC_BENCH_ORACLE_LARGE", "0") == "1")
