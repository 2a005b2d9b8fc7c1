#!/usr/bin/env python3
"""inference.py's evaluation tail on the device (pil_resize.eval_flow, inference_eval.evaluate) against what it replaces, in one run.

Kernel level, inference.py's geometry 16 x 2 x 96x320 -> 375x1242 and the same at batch 1, every variant the same way: three windows
of per-call HIP-event pairs after a warm-up, the median of each window, and of those three the median (min .. max beside it as the
spread); the inputs rotate through more than 256 MiB so that no call finds its source in the last-level cache.
  fused     pil_resize.eval_flow: score only / encode only / both / both + the float flow
  planes    pil_resize.resize_flow alone (the yardstick: what the fused launch adds to or takes from it)
  torch     resize_flow + the same metric as torch calls on the device (float ground truth, no synchronisation)
  host      resize_flow + download + inference_eval.compute_epe / compute_fl on the host (wall clock, per batch)
End to end, wall clock: inference_eval.evaluate on --samples synthetic 375x1242 samples with uint16 ground truth, against the loop a
port had before it: infer_resized per batch + download of the flow + host scoring per sample.  Both include the pipeline's
construction-free steady state only: the pipeline is captured and both loops run once before they are timed.

    python tools/bench_inference_eval.py [--out FILE] [--samples 64] [--batch 16] [--skip-e2e]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from opticalflow_amd import inference_eval as IE  # noqa: E402
from opticalflow_amd import pil_resize  # noqa: E402

PEAK = 8e12                 # bytes / s
ROTATE_BYTES = 300 << 20    # more than the 256 MiB last-level cache


def windows(fn, sets, warmup=10, calls=40, nwin=3):
    """Median of the per-window medians (us) and the smallest / largest window median."""
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    meds = []
    for _ in range(nwin):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
        for i, (a, b) in enumerate(ev):
            a.record()
            fn(sets[i % len(sets)])
            b.record()
        torch.cuda.synchronize()
        meds.append(statistics.median(a.elapsed_time(b) * 1e3 for a, b in ev))
    return statistics.median(meds), min(meds), max(meds)


def wall(fn, reps):
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def torch_metric(pred, gt, valid):
    """compute_epe / compute_fl per sample as torch calls on the device -> [n,2]; nothing synchronises."""
    d = pred - gt
    epe = torch.sqrt((d * d).sum(1))
    mag = torch.sqrt((gt * gt).sum(1))
    bad = (epe > 3.0) & (epe > 0.05 * mag) & valid
    nv = valid.flatten(1).sum(1)
    return torch.stack([(epe * valid).flatten(1).sum(1) / nv, 100.0 * bad.flatten(1).sum(1) / nv], 1)


def kernel_level(say, dev, n):
    (h, w), (H, W) = (96, 320), (375, 1242)
    g = torch.Generator(device=dev).manual_seed(22 + n)
    npx = n * H * W
    src_b, gt_b, enc_b, flow_b = n * 2 * h * w * 4, npx * 6, npx * 6, npx * 8
    nsets = ROTATE_BYTES // (src_b + gt_b + enc_b + flow_b) + 2
    sets = []
    rng = np.random.RandomState(22 + n)
    for _ in range(nsets):
        x = torch.randn((n, 2, h, w), device=dev, generator=g) * 1.5 + 20.0
        gt16 = rng.randint(30000, 36000, (n, H, W, 3)).astype(np.uint16)          # {u, v, valid}: +-40 px around the prediction's scale
        gt16[..., 2] = rng.rand(n, H, W) < 0.7
        gtf = np.stack([(gt16[..., 0].astype(np.float32) - 32768.0) / 64.0, (gt16[..., 1].astype(np.float32) - 32768.0) / 64.0], 1)
        sets.append((x, torch.from_numpy(gt16).to(dev), torch.from_numpy(gtf).to(dev), torch.from_numpy(gt16[..., 2] != 0).to(dev)))
    enc = torch.empty((n, H, W, 3), dtype=torch.uint16, device=dev)
    flow = torch.empty((n, 2, H, W), dtype=torch.float32, device=dev)
    sc = torch.empty((n, 2), dtype=torch.float32, device=dev)
    say("kernel level, %d x 2 x %dx%d -> %dx%d (%d input sets in rotation)" % (n, h, w, H, W, nsets))

    def row(tag, fn, byts, calls=40):
        med, lo, hi = windows(fn, sets, calls=calls)
        say("  %-52s %8.1f us (windows %.1f .. %.1f); algorithmic bytes %.1f MB = %.0f GB/s = %.1f %% of 8 TB/s"
            % (tag, med, lo, hi, byts / 1e6, byts / med / 1e3, 100 * byts / (med * 1e-6) / PEAK))
        return med

    planes = row("planes: resize_flow alone", lambda s: pil_resize.resize_flow(s[0], (H, W)), src_b + flow_b)
    t = {}
    t["score"] = row("fused: score only (uint16 gt)", lambda s: pil_resize.eval_flow(s[0], (H, W), gt=s[1], scores_out=sc), src_b + gt_b)
    t["score_f"] = row("fused: score only (float gt + validity)",
                       lambda s: pil_resize.eval_flow(s[0], (H, W), gt=s[2], valid=s[3], scores_out=sc), src_b + npx * 9)
    t["enc"] = row("fused: encode only", lambda s: pil_resize.eval_flow(s[0], (H, W), encode="reference", encoded_out=enc), src_b + enc_b)
    t["both"] = row("fused: score + encode", lambda s: pil_resize.eval_flow(s[0], (H, W), gt=s[1], encode="reference", encoded_out=enc,
                                                                          scores_out=sc), src_b + gt_b + enc_b)
    t["all"] = row("fused: score + encode + float flow",
                   lambda s: pil_resize.eval_flow(s[0], (H, W), gt=s[1], encode="reference", keep_flow=True, encoded_out=enc, flow_out=flow,
                                                  scores_out=sc), src_b + gt_b + enc_b + flow_b)
    tt = row("torch: resize_flow + metric as torch calls", lambda s: torch_metric(pil_resize.resize_flow(s[0], (H, W)), s[2], s[3]),
             src_b + flow_b + npx * 9, calls=15)
    say("  score only / planes = %.2f; both / planes = %.2f; torch chain / fused score = %.1fx" % (t["score"] / planes, t["both"] / planes,
                                                                                                  tt / t["score"]))
    x, _, gtf, vd = sets[0]
    gt_h, v_h = gtf.permute(0, 2, 3, 1).cpu().numpy(), vd.cpu().numpy()

    def host():
        p = pil_resize.resize_flow(x, (H, W)).permute(0, 2, 3, 1).cpu().numpy()
        return [(IE.compute_epe(p[b], gt_h[b], v_h[b]), IE.compute_fl(p[b], gt_h[b], v_h[b])) for b in range(n)]
    host()
    say("  host: resize_flow + download (%.1f MB) + compute_epe / compute_fl on the host: %.0f us per batch (wall clock)"
        % (flow_b / 1e6, wall(host, 5)))
    del sets


def end_to_end(say, dev, nsamp, batch):
    from opticalflow_amd import PWCDCNet
    from opticalflow_amd.weights import synthetic_state_dict
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).eval()
    (H, W), size = (375, 1242), (384, 1280)
    rng = np.random.RandomState(22)
    base = [rng.randint(0, 256, (H, W, 3)).astype(np.uint8) for _ in range(4)]
    gt16 = rng.randint(30000, 36000, (H, W, 3)).astype(np.uint16)
    gt16[..., 0] = rng.rand(H, W) < 0.7                       # the reference's order: {valid, v, u}
    samples = [(base[i % 4], base[(i + 1) % 4], gt16, "%06d_10.png" % i) for i in range(nsamp)]
    gt_h = np.stack([(gt16[..., 2].astype(np.float32) - 32768.0) / 64.0, (gt16[..., 1].astype(np.float32) - 32768.0) / 64.0], -1)
    v_h = gt16[..., 0] != 0

    pipes = {}

    def make(model, in_hw, image_size, device, **kw):         # the capture is paid once per size, outside the timed loop
        key = (tuple(in_hw), kw["batch"], kw["gt"], kw["encode"])
        if key not in pipes:
            pipes[key] = IE.ResizedEval(model, in_hw, image_size, device, **kw)
        return pipes[key]

    def fused():
        return IE.evaluate(net, samples, image_size=size, batch=batch, order="reference", device=dev, make_pipeline=make)

    def parent_loop():
        rows = []
        for r0 in range(0, nsamp, batch):
            part = samples[r0:r0 + batch]
            f1 = torch.from_numpy(np.stack([s[0] for s in part])).to(dev)
            f2 = torch.from_numpy(np.stack([s[1] for s in part])).to(dev)
            flow = pil_resize.infer_resized(net, f1, f2, size).permute(0, 2, 3, 1).cpu().numpy()
            rows += [(IE.compute_epe(flow[b], gt_h, v_h), IE.compute_fl(flow[b], gt_h, v_h)) for b in range(len(part))]
        return {"EPE": float(np.mean([r[0] for r in rows])), "FL": float(np.mean([r[1] for r in rows])), "num_samples": len(rows)}

    a, b = fused(), parent_loop()
    say("end to end, %d samples of %dx%d through a %dx%d network input, batch %d (fp32 plan, synthetic weights)" % (nsamp, H, W, size[0], size[1], batch))
    say("  results agree: evaluate EPE %.6f FL %.4f; parent-style loop EPE %.6f FL %.4f" % (a["EPE"], a["FL"], b["EPE"], b["FL"]))
    ta, tb = [], []
    for _ in range(3):                                         # alternating, so that drift of the machine hits both alike
        ta.append(wall(fused, 1))
        tb.append(wall(parent_loop, 1))
    ma, mb = statistics.median(ta), statistics.median(tb)
    say("  inference_eval.evaluate (one graph replay per batch, 24 B per sample downloaded): %.1f ms = %.0f pairs/s (runs %s ms)"
        % (ma / 1e3, nsamp / (ma * 1e-6), ", ".join("%.1f" % (t / 1e3) for t in ta)))
    say("  infer_resized + download + host scoring (what a port had before): %.1f ms = %.0f pairs/s (runs %s ms); %.2fx"
        % (mb / 1e3, nsamp / (mb * 1e-6), ", ".join("%.1f" % (t / 1e3) for t in tb), mb / ma))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_inference_eval.py measures on a GPU; none is visible")
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(dev))
    with torch.no_grad():
        for n in (16, 1):
            kernel_level(say, dev, n)
        if not args.skip_e2e:
            end_to_end(say, dev, args.samples, args.batch)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
