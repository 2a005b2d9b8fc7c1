#!/usr/bin/env python3
"""Fused warp + correlation + LeakyReLU backward (pwc_warp_corr81_bwd, all its launches: workspace clear, max prepass, main pass,
fixed-point -> float) against the composition it replaces (pwc_warp_fwd + LeakyReLU mask in torch + pwc_corr_bwd +
pwc_warp_bwd), level-2 geometry at batch 16 (C=32, 112x256, flow scale 5), HIP events, three operand sets in rotation.
Flows: smooth (low-resolution noise upsampled, as tools/bench_warpcorr.py) and rough (the smooth field plus independent
uniform +-3 px noise per 8x8-pixel cell, in pixels after the level's scale).
Algorithmic bytes of the fused backward: reads c1, c2, y, gy, flo and writes grad_c1, grad_c2, grad_flo = (4C + 2*81 + 4) * H*W*4
per image, y and gy counted once (the kernel re-reads them for every 16-channel chunk of a tile that a workgroup runs, and the int64
workspace is not counted)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import ops  # noqa: E402

dev = torch.device("cuda:0")
B, C, H, W = [int(v) for v in os.environ.get("PWC_BENCH_GEOM", "16,32,112,256").split(",")]
SCALE = 5.0
g = torch.Generator().manual_seed(0)


def t(fns, reps=20):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in fns:
        f()
    torch.cuda.synchronize()
    s.record()
    for i in range(reps):
        fns[i % len(fns)]()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def smooth():
    return torch.nn.functional.interpolate(torch.randn(B, 2, max(H // 8, 2), max(W // 8, 2), generator=g) * 0.6, size=(H, W),
                                           mode="bicubic", align_corners=False).contiguous()


def rough():
    cells = (torch.rand(B, 2, (H + 7) // 8, (W + 7) // 8, generator=g) * 6.0 - 3.0) / SCALE
    return (smooth() + cells.repeat_interleave(8, 2).repeat_interleave(8, 3)[:, :, :H, :W]).contiguous()


def composition(c1, c2, flo, y, gy):
    w2 = ops.warp(c2, flo, SCALE)
    gm = torch.where(y > 0, gy, gy * 0.1)
    g1, gw2 = ops.correlation_backward(c1, w2, gm)
    g2, gf = ops.warp_backward(c2, flo, gw2, SCALE)
    return g1, g2, gf


nbytes = (4 * C + 2 * 81 + 4) * H * W * 4 * B
for name, make in (("smooth", smooth), ("rough", rough)):
    sets = []
    for _ in range(3):
        c1 = torch.randn(B, C, H, W, generator=g).to(dev)
        c2 = torch.randn(B, C, H, W, generator=g).to(dev)
        flo = make().to(dev)
        y = ops.warp_correlation(c1, c2, flo, flow_scale=SCALE, leaky_slope=0.1)
        gy = torch.randn(B, 81, H, W, generator=g).to(dev)
        sets.append((c1, c2, flo, y, gy))
    fused = t([(lambda s=s: ops.warp_correlation_backward(*s, SCALE)) for s in sets])
    comp = t([(lambda s=s: composition(*s)) for s in sets])
    a = ops.warp_correlation_backward(*sets[0], SCALE)
    b = composition(*sets[0])
    rel = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(a, b))
    print("level 2 (%d,%d,%d,%d) %-6s flow: fused backward %7.1f us = %6.1f GB/s algorithmic (%.1f%% of 8 TB/s) | composition "
          "%7.1f us (%.1fx) | max rel. difference %.1e" % (B, C, H, W, name, fused, nbytes / fused / 1e3, nbytes / fused / 1e3 / 80.0,
                                                           comp, comp / fused, rel), flush=True)
