#!/usr/bin/env python3
"""Micro-bench of the fp32 first pyramid level at the batch-16 geometry (32 images of 224x512 after conv1a), HIP events:
the five launches of the direct route (conv1a x2, conv1aa, conv1b, conv2a) one by one, and conv1aa / conv1b on the 16-channel
Winograd kernel (ops.pyr1_wino), and the two as one launch (ops.pyr1_wino_pair).  Every launch rotates over PWC_BENCH_SETS (default 3) operand sets, so that the 235 MB maps are not
served from the 256 MiB Infinity Cache.  PWC_BENCH_GEOM=B,H,W picks another geometry."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
B, H, W = [int(v) for v in os.environ.get("PWC_BENCH_GEOM", "16,448,1024").split(",")]
SETS = int(os.environ.get("PWC_BENCH_SETS", "3"))
g = torch.Generator().manual_seed(0)
ws = [((torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (ci * 9)) ** 0.5).to(dev), (torch.randn(co, generator=g) * 0.1).to(dev))
      for ci, co in ((3, 16), (16, 16), (16, 16), (16, 32))]
packed = [ops.pack_conv3x3(w) for w, _ in ws]
wino = [ops.pack_pyr1_wino(w) for w, _ in ws[1:3]]
h1, w1 = H // 2, W // 2
img = [torch.rand(B, 6, H, W, generator=g).to(dev) for _ in range(SETS)]
a = [torch.randn(2 * B, 16, h1, w1, generator=g).to(dev) for _ in range(SETS)]
bb = [torch.empty_like(a[0]) for _ in range(SETS)]
c2 = [torch.empty((2 * B, 32, h1 // 2, w1 // 2), device=dev) for _ in range(SETS)]


def conv1a(i, half):
    ops.conv3x3(img[i][:, 3 * half:3 * half + 3], packed[0], ws[0][1], 16, stride=2, leaky_slope=0.1, out=a[i][half * B:(half + 1) * B])


CASES = [
    ("conv1a image 1   (image_conv_s2)", lambda i: conv1a(i, 0)),
    ("conv1a image 2   (image_conv_s2)", lambda i: conv1a(i, 1)),
    ("conv1aa direct   (mfma16)", lambda i: ops.conv3x3(a[i], packed[1], ws[1][1], 16, leaky_slope=0.1, out=bb[i])),
    ("conv1b  direct   (mfma16)", lambda i: ops.conv3x3(bb[i], packed[2], ws[2][1], 16, leaky_slope=0.1, out=a[i])),
    ("conv2a  direct   (stride 2)", lambda i: ops.conv3x3(a[i], packed[3], ws[3][1], 32, stride=2, leaky_slope=0.1, out=c2[i])),
    ("conv1aa F(2x2)   (pyr1_wino2)", lambda i: ops.pyr1_wino(a[i], wino[0], ws[1][1], out=bb[i])),
    ("conv1b  F(2x2)   (pyr1_wino2)", lambda i: ops.pyr1_wino(bb[i], wino[1], ws[2][1], out=a[i])),
    ("conv1aa+conv1b   (pyr1_wino2_pair)", lambda i: ops.pyr1_wino_pair(a[i], wino[0], ws[1][1], wino[1], ws[2][1], out=bb[i])),
]


def t(fn, reps=10):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(SETS):
        fn(i)
    torch.cuda.synchronize()
    s.record()
    for r in range(reps * SETS):
        fn(r % SETS)
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / (reps * SETS) * 1e3


ref = ops.conv3x3(a[0], packed[1], ws[1][1], 16, leaky_slope=0.1)
got = ops.pyr1_wino(a[0], wino[0], ws[1][1])
two = ops.pyr1_wino(got, wino[1], ws[2][1])
pair = ops.pyr1_wino_pair(a[0], wino[0], ws[1][1], wino[1], ws[2][1])
print("pair vs two launches: max |diff| %.2e" % (two - pair).abs().max().item())
print("geometry %d x 16 x %d x %d, %d operand sets; pyr1_wino2 vs direct kernel: max |diff| %.2e" % (
    2 * B, h1, w1, SETS, (ref - got).abs().max().item()))
mb = 2 * B * 16 * h1 * w1 * 4 / 1e6
for rnd in range(3):
    for name, fn in CASES:
        us = t(fn)
        extra = "  %.2f TB/s in+out" % (2 * mb / us) if "conv1aa" in name or "conv1b" in name else ""
        print("round %d  %-34s %7.1f us%s" % (rnd, name, us, extra), flush=True)
