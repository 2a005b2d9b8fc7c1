#!/usr/bin/env python3
"""The flow-comparison report on the device (FlowComparer.run: one tile launch + one finish launch) against the two ways callers
computed these numbers before there was an operator, at 1x96x128 (the reference's own 384x512 run), 16x112x256 (the bench's flow2)
and 16x375x1242 (full-resolution KITTI), with and without the EPE map.

  (a) device: FlowComparer.run on resident flows.  After a warm-up, REPEATS windows of CALLS back-to-back calls, each window between
      one HIP-event pair; per call = window / CALLS; median and range of the windows.  The same from a replayed graph of one call.
      Algorithmic bytes = 16 n H W (+ 4 n H W with the map) over the per-call time, as a share of the 8 TB/s HBM peak.  This is the
      time of the launch pair as a caller sees it, not a kernel time; the two smallest sizes are launch-latency-sized and their 0.2 /
      3.7 MB of input stay in the caches, so their "share" says nothing about memory.  Which unit limits the large size is NOT
      measured here: that needs a counter run of its own.
  (b) torch chain on the device: the same metrics for the batch row only (the operator also fills one row per sample) as the
      reference's expression chain in float32 torch ops, ending in one stacked device tensor; timed like (a).
  (c) host: download of both flows + the NumPy float64 oracle (tests/flow_compare_oracle.py) for the batch row, wall clock.
The device record is checked against (c) with the oracle's derived tolerances before anything is timed.

    python tools/bench_flow_compare.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from opticalflow_amd import compare  # noqa: E402
from opticalflow_amd._pipeline import capture_graph  # noqa: E402
import flow_compare_oracle as FO  # noqa: E402

HBM_PEAK = 8.0e12
SIZES = ((1, 96, 128), (16, 112, 256), (16, 375, 1242))
TAUS = (0.25, 0.5, 1.0, 2.0)


def fields(n, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    a = torch.stack([6.0 * (4.0 * xx * (1.0 - xx) - 0.5), 4.0 * (yy * yy - 0.7 * xx)], 0)[None].repeat(n, 1, 1, 1)
    a = a + 0.05 * torch.randn(n, 2, H, W, generator=g)
    e = (2.0 * torch.rand(n, 2, H, W, generator=g) - 1.0) * 1.9 * torch.rand(n, 1, H, W, generator=g)
    return a.to(dev).contiguous(), (a - e).to(dev).contiguous()


def windows(fn, calls, repeats=9, warmup=30):
    """microseconds per call: one event pair around `calls` back-to-back calls, `repeats` times"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(calls):
            fn()
        t1.record()
        torch.cuda.synchronize()
        out.append(t0.elapsed_time(t1) * 1e3 / calls)
    return sorted(out)


def spread(t):
    return "median %.2f us (range %.2f .. %.2f over %d windows)" % (statistics.median(t), t[0], t[-1], len(t))


def torch_chain(a, b):
    """the reference's chain for one (stacked) pair, float32 on the device; one stacked result, no host synchronisation"""
    d = a - b
    ad = d.abs()
    l2, mae, mx = torch.linalg.vector_norm(d), ad.mean(), ad.max()
    na, nb = torch.linalg.vector_norm(a), torch.linalg.vector_norm(b)
    af, bf = a.reshape(-1), b.reshape(-1)
    corr = torch.corrcoef(torch.stack([af, bf]))[0, 1]
    cos = torch.dot(af, bf) / (na * nb + 1e-8)
    e = torch.linalg.vector_norm(d, dim=1)
    out = [l2, mae, mx, l2 / (na + 1e-8), mae / (a.abs().mean() + 1e-8), corr, cos, e.mean(), e.max()]
    out += [(e <= t).float().mean() * 100.0 for t in TAUS]
    for f in (a, b):
        out += [f.min(), f.max(), f.mean(), f.std(unbiased=False)]
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(dev))
    for n, H, W in SIZES:
        tag = "%dx%dx%d" % (n, H, W)
        a, b = fields(n, H, W, 5, dev)
        calls = 400 if n * H * W < 1 << 20 else 100
        # (c) first: it is also the check of the device record
        t_host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ha, hb = a.cpu().numpy(), b.cpu().numpy()
            want = FO.report(ha, hb, TAUS)
            t_host.append(time.perf_counter() - t0)
        got = compare.compare_flows(a, b, TAUS).to_host()[1]
        used = FO.check_row(got, want, where=tag)
        say("%-14s device batch row within the derived tolerances of the float64 oracle (largest use of a bound: %.2g)"
            % (tag, max(used.values())))
        per, per_eager = {}, {}
        for with_map in (False, True):
            cmp = compare.FlowComparer(n, H, W, dev, TAUS, epe_map=with_map)
            nbytes = (16 + 4 * with_map) * n * H * W
            t = windows(lambda: cmp.run(a, b), calls)
            tg = windows(capture_graph(lambda: cmp.run(a, b), dev)[0].replay, calls)
            per[with_map], per_eager[with_map] = statistics.median(tg), statistics.median(t)
            for kind, tt in (("eager", t), ("graph replay", tg)):
                m = statistics.median(tt)
                say("%-14s (a) device, %s, %-12s %s; %.3f MB algorithmic -> %.1f GB/s = %.1f %% of 8 TB/s"
                    % (tag, "with map" if with_map else "no map  ", kind + ":", spread(tt), nbytes / 1e6, nbytes / m / 1e3,
                       100.0 * nbytes / (m * 1e-6) / HBM_PEAK))
        tc = windows(lambda: torch_chain(a, b), max(calls // 4, 25))
        try:
            tcg = windows(capture_graph(lambda: torch_chain(a, b), dev)[0].replay, max(calls // 4, 25))
            say("%-14s (b) torch chain on the device, batch row only: eager %s; graph replay %s" % (tag, spread(tc), spread(tcg)))
        except RuntimeError as e:                                  # a chain that cannot be captured is a finding, not a failure
            tcg = [float("nan")]
            say("%-14s (b) torch chain on the device, batch row only: eager %s; graph replay NOT measured (%s)"
                % (tag, spread(tc), str(e).splitlines()[0]))
        say("%-14s (c) host: download + NumPy float64 oracle, batch row only: median %.2f ms (range %.2f .. %.2f, %d runs)"
            % (tag, statistics.median(t_host) * 1e3, min(t_host) * 1e3, max(t_host) * 1e3, len(t_host)))
        ratio_g = "%.1fx" % (statistics.median(tcg) / per[False]) if tcg[0] == tcg[0] else "not measured"
        say("%-14s     no map: eager torch chain / eager operator %.1fx; replayed torch chain / replayed operator %s; host / eager "
            "operator %.0fx" % (tag, statistics.median(tc) / per_eager[False], ratio_g, statistics.median(t_host) * 1e6 / per_eager[False]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
