#!/usr/bin/env python3
"""KITTI evaluation (forward + EPE / Fl-all) at 375x1242 on 64 synthetic samples, the host loop against the device-scored stream,
both measured in the same run:
  (a) pairs/s of kitti.evaluate_pairs (per pair: eager forward at batch 1, full-resolution flow downloaded, NumPy metrics -- the
      loop as it stood before the score kernel) and of kitti.evaluate_stream at batch 1 and 16 (uint16 ground truth, ScoredInfer
      captured once and reused), for the fp16-strict and fp32 plans; wall clock around the whole call, best and worst of 3;
  (b) graph replay of ScoredInfer against GraphedInfer at batch 16 (HIP events, windows of at least 0.5 s, two alternating
      readings of each side);
  (c) the score kernel alone against flow_upsample alone at 16x375x1242 (HIP events), with the score kernel's algorithmic bytes
      (quarter-resolution flow + uint16 ground truth in, nothing image-sized out) as a share of the 8 TB/s HBM peak."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import PWCDCNet, kitti, ops  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
H, W, N = 375, 1242, 64


def timed(fn, min_s=0.5):
    for _ in range(3):
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
        if ms >= min_s * 1e3:
            return ms * 1e3 / n                     # microseconds per call
        n = max(n * 2, int(n * min_s * 1e3 / max(ms, 1e-3) * 1.1))


def wall(fn, reps=3):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return min(out), max(out), res


def make_samples(net):
    """images: seeded noise pairs; ground truth: the model's own flow plus an error vector of uniform length 0..6 px, as uint16"""
    g = torch.Generator().manual_seed(0)
    pairs = [(torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8))
             for _ in range(N)]
    pipe = kitti.GraphedInfer(net, H, W, dev, batch=16)
    full = torch.cat([pipe(u8).cpu() for u8 in kitti.BatchStream(pairs, dev, 16)], 0).numpy()
    rng = np.random.default_rng(1)
    gts = []
    for b in range(N):
        length, angle = rng.uniform(0, 6, (H, W)), rng.uniform(0, 2 * np.pi, (H, W))
        gt = full[b].transpose(1, 2, 0) + np.stack([length * np.cos(angle), length * np.sin(angle)], axis=-1)
        gts.append(kitti.encode_flow_rgb16(np.round(gt * 64.0) / 64.0, rng.uniform(0, 1, (H, W)) < 0.3))
    return pairs, gts


def main():
    for prec in ("fp16-strict", "fp32"):
        net = PWCDCNet(precision=prec) if prec != "fp32" else PWCDCNet()
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
        net = net.to(dev).eval()
        pairs, gts = make_samples(net)
        host_samples = [(a, b) + kitti.decode_flow_rgb16(g) for (a, b), g in zip(pairs, gts)]
        dev_samples = [(a, b, g) for (a, b), g in zip(pairs, gts)]
        # (a)
        kitti.evaluate_pairs(net, host_samples[:4], dev)                                     # warm-up: plans, first launches
        lo, hi, ref = wall(lambda: kitti.evaluate_pairs(net, host_samples, dev))
        print("%-11s (a) evaluate_pairs  (host loop, batch 1)   %8.1f .. %8.1f pairs/s   EPE %.6f Fl-all %.4f"
              % (prec, N / hi, N / lo, ref[0], ref[1]))
        base = N / lo
        for batch in (1, 16):
            pipe = kitti.ScoredInfer(net, H, W, dev, batch=batch, gt="png16", rows=N)
            kitti.evaluate_stream(net, dev_samples[:batch], dev, batch=batch, pipe=pipe)
            lo, hi, got = wall(lambda: kitti.evaluate_stream(net, dev_samples, dev, batch=batch, pipe=pipe))
            print("%-11s (a) evaluate_stream (device score, batch %2d) %6.1f .. %8.1f pairs/s   EPE %.6f Fl-all %.4f   %.1fx the host loop"
                  % (prec, batch, N / hi, N / lo, got[0], got[1], (N / lo) / base))
        # (b) pipe is the batch-16 ScoredInfer
        plain = kitti.GraphedInfer(net, H, W, dev, batch=16)
        plain.static_u8.copy_(pipe.static_u8)                                                # both graphs on the same 16 pairs
        s1, p1 = timed(pipe.graph.replay), timed(plain.graph.replay)
        s2, p2 = timed(pipe.graph.replay), timed(plain.graph.replay)
        print("%-11s (b) graph replay at batch 16: ScoredInfer %9.1f / %9.1f us   GraphedInfer %9.1f / %9.1f us   scored / plain %.4f"
              % (prec, s1, s2, p1, p2, min(s1, s2) / min(p1, p2)))
        del pipe, plain
    # (c)
    n, Hq, Wq, ch, cw = 16, 96, 320, 87, 282
    fq = torch.randn(n, 2, Hq, Wq, device=dev) * 5.0
    out = torch.empty(n, 2, H, W, device=dev)
    full = ops.flow_upsample(fq, ch, cw, H, W, out=out).cpu().numpy()
    rng = np.random.default_rng(2)
    gt16 = np.stack([kitti.encode_flow_rgb16(full[b].transpose(1, 2, 0) + rng.uniform(-4, 4, (H, W, 2)), rng.uniform(0, 1, (H, W)) < 0.3)
                     for b in range(n)])
    gt = torch.from_numpy(gt16).to(dev)
    res = torch.empty(n, 2, device=dev)
    k1, u1 = timed(lambda: ops.kitti_score(fq, ch, cw, H, W, gt, out=res)), timed(lambda: ops.flow_upsample(fq, ch, cw, H, W, out=out))
    k2, u2 = timed(lambda: ops.kitti_score(fq, ch, cw, H, W, gt, out=res)), timed(lambda: ops.flow_upsample(fq, ch, cw, H, W, out=out))
    kf = timed(lambda: ops.kitti_score(fq, ch, cw, H, W, gt, out=res, flow_out=out))
    alg = n * 2 * ch * cw * 4 + n * H * W * 6
    wr = n * 2 * H * W * 4
    t = min(k1, k2) * 1e-6
    print("16x375x1242 (c) kitti_score (tile + finish launches) %7.1f / %7.1f us   flow_upsample %7.1f / %7.1f us   kitti_score with flow_out %7.1f us"
          % (k1, k2, u1, u2, kf))
    print("16x375x1242 (c) kitti_score reads %.1f MB algorithmic (quarter flow + uint16 ground truth), writes 24 B per tile: %.1f%% of 8 TB/s;"
          " flow_upsample writes %.1f MB: %.1f%% of 8 TB/s" % (alg / 1e6, 100.0 * alg / t / 8e12, wr / 1e6, 100.0 * wr / (min(u1, u2) * 1e-6) / 8e12))


if __name__ == "__main__":
    main()
