#!/usr/bin/env python3
"""Vanishing-point estimation on the device against the host, at 1x384x512 and 16x448x1024 frames, step 16 and the reference's
defaults (max_points 300: up to 44 850 pairs per frame, 64 x 64 bins), on a synthetic radial field with noise.

  (a) device: VanishingEstimator.run on a resident arrow grid, one HIP-event pair around every call after a warm-up; the median of
      the calls, and the same from a replayed graph of one call;
  (b) host, NumPy: the oracle of tests/vanishing_oracle.py with the pairs as array expressions, per frame, wall clock;
  (c) host, Python pair loop: the same oracle with the reference's double loop as it is written there, per frame, wall clock.
(b) and (c) get the cells the device selected (the same order table), so all three do the same work; the device result is checked
against (b) before anything is timed.  The download of the flow that the host paths need first is not counted.

    python tools/bench_vanishing.py [--out FILE]"""
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
from opticalflow_amd import vanishing  # noqa: E402
from opticalflow_amd._pipeline import capture_graph  # noqa: E402
import vanishing_oracle as VO  # noqa: E402

STEP = 16


def field(B, H, W, seed):
    gy, gx = -(-H // STEP), -(-W // STEP)
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(gy) * float(STEP), np.arange(gx) * float(STEP), indexing="ij")
    out = []
    for _ in range(B):
        fx, fy = g.uniform(0.3 * W, 0.7 * W), g.uniform(0.3 * H, 0.7 * H)
        out.append(0.03 * np.stack([xx - fx, yy - fy], axis=-1) + 0.2 * g.standard_normal((gy, gx, 2)))
    return np.ascontiguousarray(np.stack(out), dtype=np.float32)


def event_times(fn, warmup=20, calls=200):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)          # microseconds


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
    for B, H, W in ((1, 384, 512), (16, 448, 1024)):
        tag = "%dx%dx%d" % (B, H, W)
        vec_h = field(B, H, W, seed=17)
        gy, gx = vec_h.shape[1:3]
        vec = torch.from_numpy(vec_h).to(dev)
        est = vanishing.VanishingEstimator(B, (H, W), step=STEP, device=dev)
        got = est.run(vec)
        info, xy = got.info.cpu().numpy(), got.xy.cpu().numpy()
        order = vanishing.order_table(gy * gx, 0)
        idxs = []
        for b in range(B):
            mag = np.hypot(vec_h[b, ..., 0].astype(np.float64), vec_h[b, ..., 1].astype(np.float64)).ravel()
            keep = mag >= 1.0
            sel = VO.select_by_order(keep, order, 300)
            idxs.append(np.searchsorted(np.flatnonzero(keep), sel) if keep.sum() > 300 else None)
        r0 = VO.estimate(vec_h[0], (H, W), STEP, idx=idxs[0])
        agree = (int(info[0, 0]), int(info[0, 1]), int(info[0, 2])) == (r0["status"], r0["n_used"], r0["pairs_kept"]) and \
            (r0["xy"] is None or max(abs(xy[0, 0] - r0["xy"][0]), abs(xy[0, 1] - r0["xy"][1])) <= VO.xy_tolerance(r0))
        say("%-14s grid %dx%d, frame 0: status %d, N %d, pairs kept %d, device == oracle: %s"
            % (tag, gy, gx, info[0, 0], info[0, 1], info[0, 2], agree))
        t = event_times(lambda: est.run(vec))
        tg = event_times(capture_graph(lambda: est.run(vec), dev)[0].replay)
        say("%-14s (a) device, 3 launches (%d + %d + %d workgroups): median %.1f us per call (min %.1f, p90 %.1f; %d calls), "
            "%.1f us per frame; graph replay median %.1f us"
            % (tag, B, 16 * B, B, statistics.median(t), t[0], t[int(0.9 * len(t))], len(t), statistics.median(t) / B, statistics.median(tg)))
        t_np, t_py = [], []
        for b in range(min(B, 4)):
            for loop, dst in ((False, t_np), (True, t_py)):
                t0 = time.perf_counter()
                VO.estimate(vec_h[b], (H, W), STEP, idx=idxs[b], loop=loop)
                dst.append(time.perf_counter() - t0)
        m_np, m_py = statistics.median(t_np), statistics.median(t_py)
        say("%-14s (b) host NumPy oracle: median %.2f ms per frame, %.2f ms per batch   (c) host Python pair loop: median %.1f ms per "
            "frame, %.1f ms per batch (%d frames timed each)" % (tag, m_np * 1e3, m_np * B * 1e3, m_py * 1e3, m_py * B * 1e3, len(t_np)))
        dev_frame = statistics.median(t) / B * 1e-6
        say("%-14s     per frame: device %.1f us, NumPy %.0fx that, Python loop %.0fx that" % (tag, dev_frame * 1e6, m_np / dev_frame,
                                                                                              m_py / dev_frame))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
