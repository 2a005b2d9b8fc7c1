#!/usr/bin/env python3
"""The cv2.warpPerspective-exact warp kernel (opticalflow_amd.cv_warp) at the top-view video's size, with the script's matrix
(cv_warp.topview_matrix(1920, 1080)), in one run:

  kernel : cv_warp.warp_frames on 1 x 1080x1920 and 16 x 1080x1920 uint8 BGR frames (one launch) against the yardstick, a device copy_
           of the same uint8 buffer into the same destination: the streaming floor for reading and writing 6.2 MB per frame.  One
           HIP-event pair around every call, the median of a window of calls; the two routes alternate, three windows each, and the
           range of the three medians is printed.  The sources rotate through more than 256 MiB so that no call finds its frame in
           the last-level cache.  Algorithmic bytes n * 2 * H * W * 3 over the median as a share of 8 TB/s.
  graph  : TopviewInfer (warp -> ingest -> net -> exit in one graph) at batch 1 and 1080x1920 against CvGraphedInfer(mode="topview")
           fed frames that are already warped; both calls copy the same 12.4 MB of uint8 pairs into their static buffer and replay.
           HIP events around each call, alternating windows; the difference is what the warp costs inside the graph.  The network
           has synthetic weights (the time does not depend on them).
  The limiting unit is not measured here (no counters).

    python tools/bench_cv_warp.py [--out FILE] [--label TEXT] [--skip-pipeline]"""
import argparse
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from opticalflow_amd import PWCDCNet, cv_resize, cv_warp  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

PEAK = 8e12                 # bytes / s
ROTATE_BYTES = 300 << 20    # more than the 256 MiB last-level cache
WINDOWS = 3
H, W = 1080, 1920


def window_median(fn, sets, calls, start):
    """Median HIP-event time in microseconds of `calls` calls fn(sets[i % len])."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(sets[(start + i) % len(sets)])
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev)


def alternate(routes, sets, calls, warmup=3):
    """routes: {name: fn}.  WINDOWS windows per route, the routes taking turns -> {name: [window medians]}."""
    for fn in routes.values():
        for i in range(warmup):
            fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for wdw in range(WINDOWS):
        for k, fn in routes.items():
            out[k].append(window_median(fn, sets, calls, wdw * calls))
    return out


def fmt(ws):
    return "median of window medians %.1f us (windows %s; range %.1f)" % (statistics.median(ws), ", ".join("%.1f" % w for w in ws),
                                                                          max(ws) - min(ws))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="unlabelled", help="what the figures were taken at (a commit), written into the report")
    ap.add_argument("--skip-pipeline", action="store_true", help="kernel only, no network")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("taken at: %s" % args.label)
    say("device: %s" % torch.cuda.get_device_name(dev))
    g = torch.Generator(device=dev).manual_seed(22)
    M = cv_warp.topview_matrix(W, H)
    cv_warp.prepare(M, dev)

    for n in (1, 16):
        nbytes = n * H * W * 3
        sets = [torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
                for _ in range(min(ROTATE_BYTES // nbytes + 2, 128))]
        dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
        calls = 40 if n == 1 else 10
        t = alternate({"warp": lambda s: cv_warp.warp_frames(s, M, out=dst), "copy": lambda s: dst.copy_(s)}, sets, calls)
        mw, mc = statistics.median(t["warp"]), statistics.median(t["copy"])
        say("%d x %dx%d, the script's matrix, %d rotating sources" % (n, H, W, len(sets)))
        say("    warp kernel: %s; algorithmic bytes %.2f MB read + %.2f MB written = %.1f GB/s = %.2f %% of 8 TB/s"
            % (fmt(t["warp"]), nbytes / 1e6, nbytes / 1e6, 2 * nbytes / mw / 1e3, 100 * 2 * nbytes / (mw * 1e-6) / PEAK))
        say("    copy_ of the same buffer (yardstick): %s = %.1f GB/s" % (fmt(t["copy"]), 2 * nbytes / mc / 1e3))
        say("    warp / copy = %.2f (ratios of the three window pairs: %s)"
            % (mw / mc, ", ".join("%.2f" % (a / b) for a, b in zip(t["warp"], t["copy"]))))
        del sets, dst

    if args.skip_pipeline:
        say("in-graph cost: NOT MEASURED (--skip-pipeline)")
    else:
        net = PWCDCNet()
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
        net = net.to(dev).eval()
        sets = [torch.randint(0, 256, (1, 2, H, W, 3), dtype=torch.uint8, device=dev, generator=g) for _ in range(26)]
        top = cv_warp.TopviewInfer(net, H, W, dev, M, batch=1)
        plain = cv_resize.CvGraphedInfer(net, H, W, dev, batch=1, mode="topview")
        t = alternate({"topview": top, "plain": plain}, sets, 20)
        mt, mp = statistics.median(t["topview"]), statistics.median(t["plain"])
        say("one pair of %dx%d per replay, fp32 net with synthetic weights, copy of the pair into the static buffer included" % (H, W))
        say("    TopviewInfer (warp + ingest + net + exit): %s" % fmt(t["topview"]))
        say("    CvGraphedInfer(mode='topview') on pre-warped frames: %s" % fmt(t["plain"]))
        spread = max(max(t["topview"]) - min(t["topview"]), max(t["plain"]) - min(t["plain"]))
        say("    in-graph cost of the warp (two frames): %.1f us = %.2f %% of the plain replay; largest spread of three windows %.1f us"
            % (mt - mp, 100 * (mt - mp) / mp, spread))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
