#!/usr/bin/env python3
"""Pillow-exact device resize (opticalflow_amd.pil_resize) against the host chain it replaces and against the nearest torch
expression, in one run:

  frames (a)  8 x 1080x1920 -> 384x512  + ImageNet normalisation (one train_pseudo batch of 4 pairs)
         (b) 32 x 1080x1920 -> 384x512
         (c) 16 x 375x1242  -> 384x1280 (inference.py)
  flow   (d) 16 x 2 x 96x320 -> 375x1242 with the vectors rescaled (inference.py's resize_flow)

  kernel : one HIP-event pair around every call after a warm-up, median; the inputs rotate through more than 256 MiB so that no call
           finds its source in the last-level cache.  Algorithmic bytes (source read once + result written once) over that time as
           a share of 8 TB/s.
  torch  : F.interpolate(mode="bilinear", antialias=True) + normalise on the device, the same way.  NOT bit-equal to Pillow
           (float arithmetic, no 8-bit intermediate): timed only.
  host   : the reference's own chain per image (Pillow resize + torch CPU ToTensor / Normalize, or Pillow on float planes + NumPy
           scaling), wall clock, on a few images, given per batch.
  ingest : FrameIngest.pairs end to end from host memory (fill of the pinned slot + one upload of the raw uint8 frames + one resize
           call), wall clock per batch, beside the upload of the FINISHED float batch from pinned memory (what a host pipeline pays
           after its own resize).  The raw frames are the larger transfer whenever the source is larger than 4x the target.

    python tools/bench_resize.py [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from opticalflow_amd import pil_resize  # noqa: E402

MEAN, STD = pil_resize.IMAGENET_MEAN, pil_resize.IMAGENET_STD
PEAK = 8e12                 # bytes / s
ROTATE_BYTES = 300 << 20    # more than the 256 MiB last-level cache


def event_times(fn, sets, warmup=10, calls=60):
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(sets[i % len(sets)])
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) * 1e3 for a, b in ev)          # microseconds


def wall(fn, reps):
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    try:
        import PIL
        from PIL import Image
        say("device: %s; Pillow %s" % (torch.cuda.get_device_name(dev), PIL.__version__))
    except ImportError:
        Image = None
        say("device: %s; Pillow not importable: host chain not measured" % torch.cuda.get_device_name(dev))
    mean_d = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1)
    std_d = torch.tensor(STD, device=dev).view(1, 3, 1, 1)
    g = torch.Generator(device=dev).manual_seed(18)

    for tag, n, (H, W), (h, w) in (("a", 8, (1080, 1920), (384, 512)), ("b", 32, (1080, 1920), (384, 512)),
                                   ("c", 16, (375, 1242), (384, 1280))):
        src_bytes, dst_bytes = n * H * W * 3, n * 3 * h * w * 4
        sets = [torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device=dev, generator=g)
                for _ in range(ROTATE_BYTES // src_bytes + 2)]
        out = torch.empty((n, 3, h, w), device=dev)
        t = event_times(lambda s: pil_resize.resize_frames(s, (h, w), MEAN, STD, out=out), sets)
        med = statistics.median(t)
        say("(%s) frames %d x %dx%d -> %dx%d: kernel %.1f us median (min %.1f, max %.1f, %d calls); algorithmic bytes %.1f MB read + "
            "%.1f MB written = %.1f GB/s = %.1f %% of 8 TB/s" % (tag, n, H, W, h, w, med, t[0], t[-1], len(t), src_bytes / 1e6,
                                                                  dst_bytes / 1e6, (src_bytes + dst_bytes) / med / 1e3,
                                                                  100 * (src_bytes + dst_bytes) / (med * 1e-6) / PEAK))

        def torch_chain(s):
            x = s.permute(0, 3, 1, 2).float()
            x = F.interpolate(x, size=(h, w), mode="bilinear", antialias=True, align_corners=False)
            return (x / 255.0 - mean_d) / std_d
        tt = statistics.median(event_times(torch_chain, sets, warmup=3, calls=10))
        diff = (torch_chain(sets[0]) - pil_resize.resize_frames(sets[0], (h, w), MEAN, STD)).abs().max().item()
        say("    torch F.interpolate(antialias=True) + normalise on the device: %.1f us median (%.2fx the kernel's time; not bit-equal: "
            "max |difference| %.3g)" % (tt, tt / med, diff))

        host = [f.numpy() for f in sets[0][:min(n, 4)].cpu()]
        if Image is not None:
            m_h, s_h = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)

            def host_chain():
                for f in host:
                    r = np.array(Image.fromarray(f).resize((w, h), Image.BILINEAR))
                    torch.from_numpy(r).permute(2, 0, 1).contiguous().float().div(255).sub_(m_h).div_(s_h)
            host_chain()
            th = wall(host_chain, 3) / len(host) * n
            say("    host chain (Pillow + torch CPU, one thread of Python, %d images timed): %.0f us per batch of %d" % (len(host), th, n))

        if n % 2 == 0:
            B = n // 2
            ing = pil_resize.FrameIngest((h, w), MEAN, STD, device=dev, batch=B)
            raw = sets[0].cpu().numpy()
            x = torch.empty((B, 6, h, w), device=dev)
            for _ in range(3):
                ing.pairs(raw[:B], raw[B:], out=x)
            ti = wall(lambda: ing.pairs(raw[:B], raw[B:], out=x), 10)
            pinned_raw = torch.empty((n, H, W, 3), dtype=torch.uint8, pin_memory=True)
            dev_raw = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
            tr = wall(lambda: dev_raw.copy_(pinned_raw, non_blocking=True), 10)
            pinned_fin = torch.empty((B, 6, h, w), pin_memory=True)
            tf = wall(lambda: x.copy_(pinned_fin, non_blocking=True), 10)
            say("    FrameIngest.pairs from host arrays, %d pairs (slot fill + raw upload + resize): %.0f us per batch; the raw upload "
                "alone (%.1f MB, pinned) %.0f us; the upload of the finished float batch (%.1f MB, pinned) %.0f us"
                % (B, ti, src_bytes / 1e6, tr, dst_bytes / 1e6, tf))
        del sets

    n, c, (h, w), (H, W) = 16, 2, (96, 320), (375, 1242)
    src_bytes, dst_bytes = n * c * h * w * 4, n * c * H * W * 4
    sets = [torch.randn((n, c, h, w), device=dev, generator=g) * 30 for _ in range(ROTATE_BYTES // (src_bytes + dst_bytes) + 2)]
    t = event_times(lambda s: pil_resize.resize_flow(s, (H, W)), sets)
    med = statistics.median(t)
    say("(d) flow %d x 2 x %dx%d -> %dx%d, vectors rescaled: kernel %.1f us median (min %.1f, max %.1f, %d calls); algorithmic bytes "
        "%.1f MB read + %.1f MB written = %.1f GB/s = %.1f %% of 8 TB/s" % (n, h, w, H, W, med, t[0], t[-1], len(t), src_bytes / 1e6,
                                                                            dst_bytes / 1e6, (src_bytes + dst_bytes) / med / 1e3,
                                                                            100 * (src_bytes + dst_bytes) / (med * 1e-6) / PEAK))
    fac = torch.tensor([W / w, H / h], device=dev).view(1, 2, 1, 1)
    tt = statistics.median(event_times(lambda s: F.interpolate(s, size=(H, W), mode="bilinear", antialias=True) * fac, sets, 3, 10))
    say("    torch F.interpolate(antialias=True) * factors on the device: %.1f us median (%.2fx the kernel's time; not bit-equal)"
        % (tt, tt / med))
    if Image is not None:
        hf = sets[0][:2].cpu().numpy()

        def host_flow():
            for f in hf:
                u = np.array(Image.fromarray(f[0]).resize((W, H), Image.BILINEAR))
                v = np.array(Image.fromarray(f[1]).resize((W, H), Image.BILINEAR))
                r = np.stack([u, v], axis=-1)
                r[:, :, 0] *= (W / w)
                r[:, :, 1] *= (H / h)
        host_flow()
        say("    host chain (Pillow on float planes + NumPy, %d flows timed, download not counted): %.0f us per batch of %d"
            % (len(hf), wall(host_flow, 3) / len(hf) * n, n))

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
