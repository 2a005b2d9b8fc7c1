#!/usr/bin/env python3
"""Front of the video pipeline: the host ingest (video.frame_to_tensor + kitti.pad_to_64, float32 upload) against the raw upload + the
HIP ingest kernel (video.ingest_frames, csrc/pwc_video.hip), and what it does to a video loop, at 384x512, 720x1280 and 1080x1920,
both routes from the same run:

  kernel : pwc_video_ingest_u8 on one frame, a HIP-event pair around every call, the median of a window of calls, three windows; the
           sources rotate through more than 256 MiB so that no call finds its frame in the last-level cache.  Algorithmic bytes
           (3*H*W read + 12*Hp*Wp written) over the median as a share of 8 TB/s.  The small sizes are launch latency.
  frame  : wall clock per frame, device synchronised after each, of (a) frame_to_tensor + pad_to_64 + .to(device) and (b) copy into a
           pinned staging buffer + upload of the bytes + kernel, the way RawFlowStream uploads.  Median of a window, three windows,
           the routes taking turns.
  loop   : frames / s of video.flow_video(net, frames, ingest=...) for ingest "host" and "hip", precision fp32 and fp16-strict: wall
           clock over a window of yielded flows (each is downloaded, so each is complete), three windows after a warm-up that holds
           the plan's construction and the graph capture; the median and the range.  Synthetic weights (the time does not depend on
           them); frames are random bytes, cycled from a pool of eight.
  The limiting unit is not measured here (no counters).

    python tools/bench_video_ingest.py [--out FILE] [--label TEXT] [--sizes 384x512,720x1280,1080x1920] [--skip-loop]"""
import argparse
import itertools
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from opticalflow_amd import PWCDCNet, video  # noqa: E402
from opticalflow_amd.kitti import pad_to_64  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

PEAK = 8e12                 # bytes / s
ROTATE_BYTES = 300 << 20    # more than the 256 MiB last-level cache
WINDOWS = 3


def med_range(ws, unit, scale=1.0):
    return "%.4g %s (windows %s; range %.3g)" % (statistics.median(ws) * scale, unit, ", ".join("%.4g" % (w * scale) for w in ws),
                                                (max(ws) - min(ws)) * scale)


def kernel_windows(sets, out, calls):
    for s in sets[:3]:
        video.ingest_frames(s, out=out)
    torch.cuda.synchronize()
    ws = []
    for w in range(WINDOWS):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for i, (a, b) in enumerate(ev):
            a.record()
            video.ingest_frames(sets[(w * calls + i) % len(sets)], out=out)
            b.record()
        torch.cuda.synchronize()
        ws.append(statistics.median(a.elapsed_time(b) * 1e-3 for a, b in ev))
    return ws                                                        # seconds


def wall_windows(routes, frames, calls):
    """routes {name: fn(frame)}; each call is followed by a device synchronise.  -> {name: [window medians in seconds]}"""
    for fn in routes.values():
        for f in frames[:2]:
            fn(f)
            torch.cuda.synchronize()
    out = {k: [] for k in routes}
    for w in range(WINDOWS):
        for k, fn in routes.items():
            ts = []
            for i in range(calls):
                f = frames[(w * calls + i) % len(frames)]
                t0 = time.perf_counter()
                fn(f)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            out[k].append(statistics.median(ts))
    return out


def loop_windows(net, frames, ingest, warmup, count):
    gen = video.flow_video(net, itertools.cycle(frames), ingest=ingest)
    for _ in range(warmup):
        next(gen)
    ws = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            next(gen)
        ws.append(count / (time.perf_counter() - t0))
    gen.close()
    return ws                                                        # frames / s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="unlabelled", help="what the figures were taken at (a commit), written into the report")
    ap.add_argument("--sizes", default="384x512,720x1280,1080x1920")
    ap.add_argument("--skip-loop", action="store_true", help="kernel and per-frame ingest only, no network")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("taken at: %s" % args.label)
    say("device: %s; host threads: %d" % (torch.cuda.get_device_name(dev), torch.get_num_threads()))
    rng = np.random.RandomState(23)
    nets = {}
    if not args.skip_loop:
        for precision in ("fp32", "fp16-strict"):
            net = PWCDCNet(precision=precision)
            net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
            nets[precision] = net.to(dev).eval()

    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        geo = video.raw_geometry(H, W)
        frames = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(8)]
        raw_b, flt_b = 3 * H * W, 12 * geo.height * geo.width
        say("%dx%d -> %dx%d: raw frame %.2f MB, float32 network input %.2f MB" % (H, W, geo.height, geo.width, raw_b / 1e6, flt_b / 1e6))

        g = torch.Generator(device=dev).manual_seed(24)
        sets = [torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
                for _ in range(min(ROTATE_BYTES // raw_b + 2, 128))]
        out = torch.empty((1, 3, geo.height, geo.width), device=dev)
        kw = kernel_windows(sets, out, 40)
        mk = statistics.median(kw)
        say("    kernel: %s; algorithmic bytes %.2f MB read + %.2f MB written = %.1f GB/s = %.2f %% of 8 TB/s (%d rotating sources)"
            % (med_range(kw, "us", 1e6), raw_b / 1e6, flt_b / 1e6, (raw_b + flt_b) / mk / 1e9, 100 * (raw_b + flt_b) / mk / PEAK, len(sets)))
        del sets

        stage = torch.empty((1, H, W, 3), dtype=torch.uint8).pin_memory()
        raw = torch.empty((1, H, W, 3), dtype=torch.uint8, device=dev)

        def host_route(f):
            return pad_to_64(video.frame_to_tensor(f).unsqueeze(0))[0].to(dev)

        def hip_route(f):
            stage.copy_(torch.from_numpy(f).unsqueeze(0))
            raw.copy_(stage, non_blocking=True)
            return video.ingest_frames(raw, out=out)

        t = wall_windows({"host": host_route, "hip": hip_route}, frames, 12)
        say("    per frame, host ingest + float32 upload: %s" % med_range(t["host"], "ms", 1e3))
        say("    per frame, raw upload + kernel:          %s" % med_range(t["hip"], "ms", 1e3))
        say("    host / hip = %.2f (ratios of the three window pairs: %s)"
            % (statistics.median(t["host"]) / statistics.median(t["hip"]), ", ".join("%.2f" % (a / b) for a, b in zip(t["host"], t["hip"]))))
        del stage, raw, out

        for precision, net in nets.items():
            res = {ingest: loop_windows(net, frames, ingest, warmup=4, count=12 if H >= 720 else 24) for ingest in ("host", "hip")}
            mh, mp = statistics.median(res["host"]), statistics.median(res["hip"])
            spread = max(max(r) - min(r) for r in res.values())
            say("    flow_video %-11s ingest=host: %s" % (precision, med_range(res["host"], "frames/s")))
            say("    flow_video %-11s ingest=hip:  %s" % (precision, med_range(res["hip"], "frames/s")))
            say("    flow_video %-11s hip - host = %+.1f frames/s (x %.2f); largest spread of three windows %.1f frames/s -> %s"
                % (precision, mp - mh, mp / mh, spread,
                   "hip faster by more than the spread" if mp - mh > spread else
                   "host faster by more than the spread" if mh - mp > spread else "within the spread"))
            torch.cuda.empty_cache()

    if args.skip_loop:
        say("video loop: NOT MEASURED (--skip-loop)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
