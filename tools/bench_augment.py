#!/usr/bin/env python3
"""The KITTI training augmentation on the device against what a caller had before, at train.py's shape: 4 and 16 samples of 375x1242
cropped to 320x896, uint16 PNG ground truth (gt_kind 1) and float planes + valid bytes (gt_kind 0), all in one run.  Every second
sample is warped (rotation 2 degrees, scales 1.0815 / 0.9215: the extremes of the reduced augmentation), every third is flipped.

  (a) the launch alone (ops.kitti_augment on resident slots and records): HIP events around 30 back-to-back launches after a warm-up,
      ten such windows; mean and range of the window means.  With it the bytes the algorithm needs -- the crop window of both frames
      and of the ground truth read once, the nine float32 output planes written -- as a share of the 8 TB/s HBM peak.  The kernel is
      gather-bound by construction; the share says how far from the HBM roofline it runs, not which unit limits it (not measured).
  (b) the same operator chain written with torch on the device: the fixed-point coordinates in float64 / int64, reflect-101, four index
      gathers per source, the integer blend of the frames and the float32 blend of the flow and the mask, the linear part, the flip.
      Same timing; its outputs are compared with the kernel's and the number of differing elements is printed.
  (c) the NumPy oracle (tests/augment_oracle.py) on the host for ONE warped sample, wall clock.  cv2 itself is not installed and
      cannot be timed here; the oracle is a vectorised restatement of its arithmetic, not its speed.
  (d) end to end: DeviceAugmenter.__call__ (fill the pinned slots, upload 5.6 MB per sample, launch) against uploading the finished
      float32 tensors of the same batch from pinned memory (10.3 MB per sample; what DataLoader + .to(device) moves, its host-side warp,
      crop, flip and collation NOT included), wall clock around calls that end synchronised, two alternating readings each; the host
      fill alone (DeviceAugmenter.stage) is timed as well."""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
from opticalflow_amd import augment, ops  # noqa: E402
import augment_oracle as AO  # noqa: E402

dev = torch.device("cuda:0")
SIZE, CROP = (375, 1242), (320, 896)
WINDOWS, LAUNCHES = 10, 30


def timed(fn):
    """microseconds per call: (mean, min, max) of the means of WINDOWS windows of LAUNCHES back-to-back calls"""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(LAUNCHES):
            fn()
        b.record()
        b.synchronize()
        means.append(a.elapsed_time(b) * 1e3 / LAUNCHES)
    return float(np.mean(means)), min(means), max(means)


def wall(fn, min_s=1.0):
    """milliseconds per call of a function that ends synchronised"""
    for _ in range(2):
        fn()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < min_s:
        fn()
        n += 1
    return (time.perf_counter() - t0) * 1e3 / n


def records(n):
    recs = []
    for b in range(n):
        warp = (2.0 if b % 4 == 0 else -2.0, 1.0815, 0.9215) if b % 2 == 0 else None
        recs.append(AO.record(SIZE, y0=(7 * b) % (SIZE[0] - CROP[0] + 1), x0=(53 * b) % (SIZE[1] - CROP[1] + 1), warp=warp, flip=b % 3 == 0))
    p = augment.make_params(n)
    for i, r in enumerate(recs):
        for k in p.dtype.names:
            p[k][i] = r[k]
    return recs, p


def reflect(p, length):
    period = 2 * (length - 1)
    m = torch.remainder(p, period)
    return torch.where(m < length, m, period - m)


def torch_chain(frames, gt, valid, p, kind):
    """The operator as torch calls on the device, batched over samples of one size (frames [n,2,H,W,3], gt [n,H,W,3] uint16 or
    [n,2,H,W] float32 + valid [n,H,W] uint8)."""
    n, _, H, W, _ = frames.shape
    ch, cw = CROP
    m = torch.from_numpy(p["m"].copy()).to(dev)
    A = torch.from_numpy(p["a"].copy()).to(dev)
    i64 = dict(dtype=torch.int64, device=dev)
    y0, x0, warp, flip = (torch.from_numpy(p[k].astype(np.int64)).to(dev).view(n, 1, 1) for k in ("y0", "x0", "warp", "flip"))
    xs = torch.arange(cw, **i64).view(1, 1, cw)
    X = x0 + torch.where(flip != 0, cw - 1 - xs, xs)
    Y = (y0 + torch.arange(ch, **i64).view(1, ch, 1)).expand(n, ch, cw)
    Xd, Yd = X.double(), Y.double()
    mm = [m[:, k].view(n, 1, 1) for k in range(6)]
    ad = torch.round(mm[0] * Xd * 1024.0).long()                    # torch.round is half to even
    bd = torch.round(mm[3] * Xd * 1024.0).long()
    X0 = torch.round((mm[1] * Yd + mm[2]) * 1024.0).long() + 16
    Y0 = torch.round((mm[4] * Yd + mm[5]) * 1024.0).long() + 16
    Xq, Yq = (X0 + ad) >> 5, (Y0 + bd) >> 5
    w = warp != 0
    sx, sy = torch.where(w, Xq >> 5, X), torch.where(w, Yq >> 5, Y)
    fx, fy = torch.where(w, Xq & 31, torch.zeros_like(X)), torch.where(w, Yq & 31, torch.zeros_like(Y))
    xa, xb, ya, yb = reflect(sx, W), reflect(sx + 1, W), reflect(sy, H), reflect(sy + 1, H)
    bi = torch.arange(n, **i64).view(n, 1, 1).expand(n, ch, cw)
    taps = ((ya, xa), (ya, xb), (yb, xa), (yb, xb))
    iw = ((32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx)
    d255 = torch.full((1,), 255.0, device=dev)                      # a tensor: torch turns a division by a Python scalar into a
    imgs = []                                                       # multiplication by its reciprocal, which rounds differently
    for f in range(2):
        src = frames[:, f]
        acc = sum(src[bi, yy, xx].long() * wt.unsqueeze(-1) for (yy, xx), wt in zip(taps, iw))
        imgs.append(((acc + 512) >> 10).float() / d255)
    x = torch.cat(imgs, dim=-1).permute(0, 3, 1, 2).contiguous()
    if kind == 1:
        g = gt.view(torch.int16).to(torch.int32) & 0xFFFF
        u_src, v_src = (g[..., 0].float() - 32768.0) / 64.0, (g[..., 1].float() - 32768.0) / 64.0
        m_src = (g[..., 2] != 0).float()
    else:
        u_src, v_src, m_src = gt[:, 0], gt[:, 1], (valid != 0).float()
    gx, gy = fx.float() / 32.0, fy.float() / 32.0
    fw = ((1.0 - gy) * (1.0 - gx), (1.0 - gy) * gx, gy * (1.0 - gx), gy * gx)

    def blend(src):
        t = [src[bi, yy, xx] * wt for (yy, xx), wt in zip(taps, fw)]
        return ((t[0] + t[1]) + t[2]) + t[3]
    fu, fv, fm = blend(u_src), blend(v_src), blend(m_src)
    a = [torch.where(w, A[:, k].view(n, 1, 1), torch.full((n, 1, 1), 1.0 if k in (0, 3) else 0.0, device=dev)) for k in range(4)]
    u = torch.where(w, a[0] * fu + a[1] * fv, fu)
    v = torch.where(w, a[2] * fu + a[3] * fv, fv)
    u = torch.where(flip != 0, u * -1.0, u)
    return x, torch.stack([u, v], dim=1), (fm > 0.5).float().unsqueeze(1)


def main():
    ch, cw = CROP
    print("device: %s; frames %dx%d -> crop %dx%d; %d windows of %d launches after 5 warm-up calls" %
          (torch.cuda.get_device_name(0), SIZE[0], SIZE[1], ch, cw, WINDOWS, LAUNCHES))
    base = [AO.make_sample(SIZE, 1600 + i) for i in range(4)]
    for n in (4, 16):
        samples = [base[i % 4] for i in range(n)]
        recs, p = records(n)
        for kind in (1, 0):
            if kind == 1:
                host = samples
            else:
                host = [(a, b, np.stack(AO.decode_png(g)[:2], -1), g[..., 2] != 0) for a, b, g in samples]
            frames, gt, valid, _ = augment.pack_slots(host, SIZE, kind)
            frames, gt = torch.from_numpy(frames).to(dev), torch.from_numpy(gt).to(dev)
            valid = None if valid is None else torch.from_numpy(valid).to(dev)
            pd = torch.from_numpy(p.view(np.uint8).reshape(n, -1)).to(dev)
            out = ops.kitti_augment(frames, gt, pd, CROP, valid=valid)
            x, flow, vout, status = out
            assert not status.any()
            us = timed(lambda: ops.kitti_augment(frames, gt, pd, CROP, valid=valid, out=(x, flow, vout), status=status))
            src_bytes = n * ch * cw * (6 + (6 if kind == 1 else 9))
            out_bytes = n * ch * cw * 9 * 4
            share = (src_bytes + out_bytes) / (us[0] * 1e-6) / 8e12
            print("(a) kernel   n=%2d gt_kind %d: %7.1f us (window means %.1f - %.1f); algorithmic %.1f MB (%.1f read + %.1f written) = "
                  "%.1f %% of 8 TB/s" % (n, kind, us[0], us[1], us[2], (src_bytes + out_bytes) / 1e6, src_bytes / 1e6, out_bytes / 1e6,
                                        100 * share))
            tx, tf, tv = torch_chain(frames, gt, valid, p, kind)
            diff = [int((a != b).sum()) for a, b in ((tx, x), (tf, flow), (tv, vout))]
            ut = timed(lambda: torch_chain(frames, gt, valid, p, kind))
            print("(b) torch    n=%2d gt_kind %d: %7.1f us (window means %.1f - %.1f) = %.1fx the kernel; elements differing from the "
                  "kernel: x %d, flow %d, valid %d" % (n, kind, ut[0], ut[1], ut[2], ut[0] / us[0], diff[0], diff[1], diff[2]))
        # (d) end to end, gt_kind 1
        aug = augment.DeviceAugmenter(dev, n, SIZE, CROP, gt_kind=1)
        fx, ff, fv = (t.cpu().pin_memory() for t in ops.kitti_augment(frames, gt, pd, CROP, valid=valid)[:3])
        dx, df, dv = (torch.empty_like(t, device=dev) for t in (fx, ff, fv))

        def staged():
            aug(samples, p)
            torch.cuda.synchronize()

        def floats():
            dx.copy_(fx, non_blocking=True)
            df.copy_(ff, non_blocking=True)
            dv.copy_(fv, non_blocking=True)
            torch.cuda.synchronize()
        raw_mb = n * (2 * SIZE[0] * SIZE[1] * 3 + SIZE[0] * SIZE[1] * 6) / 1e6
        flt_mb = n * ch * cw * 9 * 4 / 1e6
        for rep in range(2):
            print("(d) end to end n=%2d reading %d: DeviceAugmenter (fill + upload %.1f MB + launch) %.2f ms, of which the fill of the "
                  "pinned slots on the host %.2f ms; upload of the finished float tensors (%.1f MB) %.2f ms"
                  % (n, rep, raw_mb, wall(staged), wall(lambda: aug.stage(samples, p)), flt_mb, wall(floats)))
    im1, im2, png = base[0]
    u, v, m = AO.decode_png(png)
    rec = AO.record(SIZE, y0=20, x0=100, warp=(2.0, 1.0815, 0.9215))
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < 1.0:
        AO.augment(im1, im2, u, v, m, rec, CROP)
        k += 1
    print("(c) NumPy oracle on the host, one warped sample, crop window only: %.1f ms (cv2 is not installed: not timed)" %
          ((time.perf_counter() - t0) * 1e3 / k))


if __name__ == "__main__":
    main()
