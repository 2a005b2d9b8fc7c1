#!/usr/bin/env python3
"""cv2.resize-exact ingest and flow exit (opticalflow_amd.cv_resize) against the torch-op chain of opticalflow_amd.harness, in one run,
at the sizes the two scripts are used on:

  (a)  1 x 436x1024  (Sintel, script_pwc.py)      -> 448x1024
  (b) 16 x 436x1024                                -> 448x1024
  (c)  1 x 1080x1920 (top-view video, topview.py)  -> 1088x1920

  ingest : cv_resize.ingest_pairs ([n,2,H,W,3] uint8 -> [n,6,H_,W_], one kernel) against harness.preprocess on the device (one call per
           pair: it takes no batch).  Algorithmic bytes n*2*H*W*3 + n*6*H_*W_*4.
  exit   : cv_resize.resize_flow (x 20, resize, rescale, [n,H,W,2], one kernel) against harness.postprocess (one call per item).
           Algorithmic bytes n*2*(H_/4)*(W_/4)*4 + n*2*H*W*4.
  timing : one HIP-event pair around every call (for the chain: around the n calls of one batch), the median of a window of calls;
           the two routes alternate, three windows each, and the range of the three medians is printed.  The ingest inputs rotate
           through more than 256 MiB so that no call finds its source in the last-level cache.  Bytes over the median window as a
           share of 8 TB/s.  The limiting unit is not measured here (no counters).
  pairs/s: CvGraphedInfer(mode="script") fed from pinned host memory, upload of the uint8 pairs and download of the flow included,
           against a loop of harness.estimate_flow (host images in, .cpu() out), wall clock over windows that end in a synchronise,
           alternating, three windows each.  The network has synthetic weights (the time does not depend on them).

    python tools/bench_cv_resize.py [--out FILE] [--skip-pipeline]"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from opticalflow_amd import PWCDCNet, cv_resize, harness  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

PEAK = 8e12                 # bytes / s
ROTATE_BYTES = 300 << 20    # more than the 256 MiB last-level cache
WINDOWS = 3
CASES = (("a", 1, 436, 1024), ("b", 16, 436, 1024), ("c", 1, 1080, 1920))


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


def verdict(hip, tor):
    gap = min(tor) - max(hip)
    spread = max(max(hip) - min(hip), max(tor) - min(tor))
    return "kernel faster than the chain by %.1f us (slowest kernel window to fastest chain window); largest spread of three windows %.1f us: %s" \
        % (gap, spread, "faster by more than the spread" if gap > spread else "NOT faster by more than the spread")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-pipeline", action="store_true", help="kernels only, no network")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(dev))
    g = torch.Generator(device=dev).manual_seed(21)
    net = None
    if not args.skip_pipeline:
        net = PWCDCNet()
        net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
        net = net.to(dev).eval()

    for tag, n, H, W in CASES:
        H_, W_ = harness.padded_size(H, W)
        hq, wq = H_ // 4, W_ // 4
        say("(%s) %d x %dx%d -> %dx%d" % (tag, n, H, W, H_, W_))

        # ---- ingest
        src_bytes, dst_bytes = n * 2 * H * W * 3, n * 6 * H_ * W_ * 4
        sets = [torch.randint(0, 256, (n, 2, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
                for _ in range(min(ROTATE_BYTES // src_bytes + 2, 128))]
        x = torch.empty((n, 6, H_, W_), device=dev)

        def chain_in(s):
            for b in range(n):
                harness.preprocess(s[b, 0], s[b, 1])
        calls = 20 if n == 1 else 6
        t = alternate({"hip": lambda s: cv_resize.ingest_pairs(s, out=x), "torch": chain_in}, sets, calls)
        med = statistics.median(t["hip"])
        say("    ingest kernel: %s; algorithmic bytes %.2f MB read + %.2f MB written = %.1f GB/s = %.2f %% of 8 TB/s"
            % (fmt(t["hip"]), src_bytes / 1e6, dst_bytes / 1e6, (src_bytes + dst_bytes) / med / 1e3,
               100 * (src_bytes + dst_bytes) / (med * 1e-6) / PEAK))
        say("    harness.preprocess on the device (%d call%s): %s" % (n, "" if n == 1 else "s", fmt(t["torch"])))
        say("    ingest: %s" % verdict(t["hip"], t["torch"]))
        del sets

        # ---- exit
        src_bytes, dst_bytes = n * 2 * hq * wq * 4, n * 2 * H * W * 4
        sets = [torch.randn((n, 2, hq, wq), device=dev, generator=g) for _ in range(8)]
        full = torch.empty((n, H, W, 2), device=dev)

        def chain_out(s):
            for b in range(n):
                harness.postprocess(s[b:b + 1], H, W)
        t = alternate({"hip": lambda s: cv_resize.resize_flow(s, (H, W), gain=20.0, layout="hwc", out=full), "torch": chain_out},
                      sets, calls)
        med = statistics.median(t["hip"])
        say("    exit kernel: %s; algorithmic bytes %.2f MB read + %.2f MB written = %.1f GB/s = %.2f %% of 8 TB/s"
            % (fmt(t["hip"]), src_bytes / 1e6, dst_bytes / 1e6, (src_bytes + dst_bytes) / med / 1e3,
               100 * (src_bytes + dst_bytes) / (med * 1e-6) / PEAK))
        say("    harness.postprocess on the device (%d call%s): %s" % (n, "" if n == 1 else "s", fmt(t["torch"])))
        say("    exit: %s" % verdict(t["hip"], t["torch"]))
        del sets, x, full

        # ---- whole pipeline from pinned host memory
        if net is None:
            continue
        host = torch.randint(0, 256, (n, 2, H, W, 3), dtype=torch.uint8).pin_memory()
        host_out = torch.empty((n, H, W, 2)).pin_memory()
        staged = torch.empty((n, 2, H, W, 3), dtype=torch.uint8, device=dev)
        pipe = cv_resize.CvGraphedInfer(net, H, W, dev, batch=n, mode="script")
        iters = 20 if n == 1 else 4

        def graphed():
            for _ in range(iters):
                staged.copy_(host, non_blocking=True)
                host_out.copy_(pipe(staged), non_blocking=True)
            torch.cuda.synchronize()

        def looped():
            for _ in range(iters):
                for b in range(n):
                    harness.estimate_flow(net, host[b, 0], host[b, 1]).cpu()
            torch.cuda.synchronize()
        rates = {"graphed": [], "loop": []}
        graphed()
        looped()
        for _ in range(WINDOWS):
            for k, fn in (("graphed", graphed), ("loop", looped)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                rates[k].append(iters * n / (time.perf_counter() - t0))
        for k, what in (("graphed", "CvGraphedInfer from pinned host memory, upload and download included"),
                        ("loop", "loop of harness.estimate_flow (torch chain), host images in, .cpu() out")):
            r = rates[k]
            say("    %s: %.1f pairs/s (windows %s; range %.1f)" % (what, statistics.median(r), ", ".join("%.1f" % v for v in r),
                                                                 max(r) - min(r)))
        del pipe, staged

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
