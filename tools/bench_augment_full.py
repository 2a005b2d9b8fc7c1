#!/usr/bin/env python3
"""train2.py's augmentation on the device against what a caller had before, at train2.py's shape: 4 and 16 samples of 375x1242 cropped
to 320x896, uint16 PNG ground truth, in three configurations -- "all" (flip on every third sample, rotation, translation, brightness /
contrast, 7-tap blur on every sample), "none" (crop only) and "rot+blur" -- all in one run.

  (a) the launch alone (ops.kitti_augment_full on resident slots and records): HIP events around 30 back-to-back launches after a
      warm-up, ten such windows; mean and range of the window means.  With it the bytes the algorithm needs -- the crop window of both
      frames and of the ground truth read once, the nine float32 output planes written -- as a share of the 8 TB/s HBM peak.  The share
      says how far from the HBM roofline the launch runs, not which unit limits it (the limiting unit is not measured).
  (b) the same chain written with torch on the device, stage after stage on whole windows as the reference does on the host: index
      gathers for crop / flip, the fixed-point coordinates in float64 / int64 and four gathers of nine planes for the rotation, the
      float64 flow rotation, a reflected gather for the shift, the float32 brightness map, the integer blur.  Its outputs are ASSERTED
      bit-equal to the kernel's before it is timed, and the fused launch is asserted not slower.
  (c) ops.kitti_augment (the reduced pipeline of train.py, every second sample warped) at the same shape, for scale.
  (d) end to end: DeviceFullAugmenter.__call__ (fill the pinned slots, upload 5.6 MB per sample, launch) against uploading the
      finished float32 tensors of the same batch from pinned memory (10.3 MB per sample; the host-side pipeline that made them NOT
      included), wall clock around calls that end synchronised, two alternating readings each.
  (e) the NumPy oracle (tests/augment_full_oracle.py) on the host for ONE sample with all stages on, wall clock.  cv2 itself is not
      installed and cannot be timed here; the oracle is a vectorised restatement of its arithmetic, not its speed."""
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from opticalflow_amd import augment, augment_full, ops  # noqa: E402
import augment_full_oracle as FO  # noqa: E402
import augment_oracle as AO  # noqa: E402
from bench_augment import timed, wall  # noqa: E402

SIZE, CROP = (375, 1242), (320, 896)
CONFIGS = {"all": dict(rot=True, trans=True, bright=True, blur=True, flip=True), "none": {}, "rot+blur": dict(rot=True, blur=True)}


def records(n, rot=False, trans=False, bright=False, blur=False, flip=False, size=SIZE, crop=CROP):
    recs = []
    for b in range(n):
        recs.append(FO.record(size, crop, y0=(7 * b) % (size[0] - crop[0] + 1), x0=(53 * b) % (size[1] - crop[1] + 1),
                              flip=flip and b % 3 == 0, rot=(17.0 if b % 2 == 0 else -9.0 - b) if rot else None,
                              trans=(10 - b % 21, b % 21 - 10) if trans else None, bright=(0.7 + 0.05 * (b % 14)) if bright else None,
                              blur=(1.5 if b % 2 == 0 else 1.3) if blur else None))
    return recs, to_params(recs)


def to_params(recs):
    p = augment_full.make_full_params(len(recs))
    for i, r in enumerate(recs):
        for k in p.dtype.names:
            p[k][i] = r[k]
    return p


def t_reflect(p, length):
    m = torch.remainder(p, 2 * length)
    return torch.where(m < length, m, 2 * length - 1 - m)


def t_reflect101(p, length):
    if length == 1:
        return torch.zeros_like(p)
    m = torch.remainder(p, 2 * (length - 1))
    return torch.where(m < length, m, 2 * (length - 1) - m)


def torch_chain(frames, gt, p, crop):
    """The operator as torch calls, batched over samples of ONE size whose stage flags agree except for the flip (frames [n,2,H,W,3]
    uint8, gt [n,H,W,3] uint16), in the reference's forward order.  -> (x, flow, mask)."""
    dev = frames.device
    n = frames.shape[0]
    ch, cw = crop
    i64 = dict(dtype=torch.int64, device=dev)
    col = lambda k, dt=np.int64: torch.from_numpy(p[k].astype(dt)).to(dev).view(n, 1, 1)  # noqa: E731
    rot, trans, bright, blur = (bool(p[k][0]) for k in ("rot", "trans", "bright", "blur"))
    assert all((p[k] != 0).all() == bool(p[k][0]) for k in ("rot", "trans", "bright", "blur")) and len(set(p["ksize"])) == 1
    bi = torch.arange(n, **i64).view(n, 1, 1).expand(n, ch, cw)
    ys, xs = torch.arange(ch, **i64).view(1, ch, 1), torch.arange(cw, **i64).view(1, 1, cw)
    flip = col("flip") != 0
    # crop + flip
    Y = (col("y0") + ys).expand(n, ch, cw)
    X = col("x0") + torch.where(flip, cw - 1 - xs, xs)
    g = gt.view(torch.int16).to(torch.int32) & 0xFFFF
    g = g[bi, Y, X]
    u = (g[..., 0].float() - 32768.0) / 64.0
    u = torch.where(flip, -u, u)
    planes = torch.cat([frames[bi, 0, Y, X].float(), frames[bi, 1, Y, X].float(), u.unsqueeze(-1),
                        ((g[..., 1].float() - 32768.0) / 64.0).unsqueeze(-1), (g[..., 2] != 0).float().unsqueeze(-1)], dim=-1)
    if rot:
        m = torch.from_numpy(p["m"].copy()).to(dev)
        mm = [m[:, k].view(n, 1, 1) for k in range(6)]
        Xd, Yd = xs.double(), ys.double()
        ad = torch.round(mm[0] * Xd * 1024.0).long()                # torch.round is half to even
        bd = torch.round(mm[3] * Xd * 1024.0).long()
        X0 = torch.round((mm[1] * Yd + mm[2]) * 1024.0).long() + 16
        Y0 = torch.round((mm[4] * Yd + mm[5]) * 1024.0).long() + 16
        Xq, Yq = (X0 + ad) >> 5, (Y0 + bd) >> 5
        sx, sy, fx, fy = Xq >> 5, Yq >> 5, Xq & 31, Yq & 31
        xa, xb, ya, yb = t_reflect(sx, cw), t_reflect(sx + 1, cw), t_reflect(sy, ch), t_reflect(sy + 1, ch)
        gx, gy = fx.float() / 32.0, fy.float() / 32.0
        fw = [((1.0 - gy) * (1.0 - gx)), ((1.0 - gy) * gx), (gy * (1.0 - gx)), (gy * gx)]
        t = [planes[bi, yy, xx] * w.unsqueeze(-1) for (yy, xx), w in zip(((ya, xa), (ya, xb), (yb, xa), (yb, xb)), fw)]
        planes = ((t[0] + t[1]) + t[2]) + t[3]
        cs = torch.from_numpy(p["cs"].copy()).to(dev)
        c, s = cs[:, 0].view(n, 1, 1), cs[:, 1].view(n, 1, 1)
        fu, fv = planes[..., 6].double(), planes[..., 7].double()
        ru = (fu * c - fv * s).float()
        rv = (ru.double() * s + fv * c).float()
        planes = torch.cat([planes[..., :6], ru.unsqueeze(-1), rv.unsqueeze(-1), planes[..., 8:]], dim=-1)
    if trans:
        planes = planes[bi, t_reflect(ys - col("ty"), ch).expand(n, ch, cw), t_reflect(xs - col("tx"), cw).expand(n, ch, cw)]
    imgs = planes[..., :6]
    if bright:
        gain = torch.from_numpy(p["gain"].copy()).to(dev).view(n, 1, 1, 1)
        imgs = torch.clamp(gain * (imgs - 127.5) + 127.5, 0.0, 255.0)
    if blur:
        k = int(p["ksize"][0])
        r = k // 2
        wk = torch.from_numpy(p["wk"][:, :k].astype(np.int64)).to(dev)
        s8 = imgs.to(torch.int64)                                    # truncation, as astype(np.uint8) of values in [0, 255]
        xi = t_reflect101(torch.arange(-r, cw + r, **i64), cw)
        yi = t_reflect101(torch.arange(-r, ch + r, **i64), ch)
        hp = sum(wk[:, i].view(n, 1, 1, 1) * s8[:, :, xi[i:i + cw]] for i in range(k))
        vp = sum(wk[:, j].view(n, 1, 1, 1) * hp[:, yi[j:j + ch]] for j in range(k))
        imgs = ((vp + 32768) >> 16).float()
    d255 = torch.full((1,), 255.0, device=dev)                      # a tensor: torch turns a division by a Python scalar into a
    x = (imgs / d255).permute(0, 3, 1, 2).contiguous()              # multiplication by its reciprocal, which rounds differently
    return x, planes[..., 6:8].permute(0, 3, 1, 2).contiguous(), planes[..., 8:].permute(0, 3, 1, 2).contiguous()


def main():
    dev = torch.device("cuda:0")
    ch, cw = CROP
    print("device: %s; frames %dx%d -> crop %dx%d; 10 windows of 30 launches after 5 warm-up calls" %
          (torch.cuda.get_device_name(0), SIZE[0], SIZE[1], ch, cw))
    base = [AO.make_sample(SIZE, 1600 + i) for i in range(4)]
    for n in (4, 16):
        samples = [base[i % 4] for i in range(n)]
        frames, gt, _, _ = augment.pack_slots(samples, SIZE, 1)
        frames, gt = torch.from_numpy(frames).to(dev), torch.from_numpy(gt).to(dev)
        src_bytes, out_bytes = n * ch * cw * 12, n * ch * cw * 9 * 4
        for name, kw in CONFIGS.items():
            recs, p = records(n, **kw)
            pd = torch.from_numpy(p.view(np.uint8).reshape(n, -1)).to(dev)
            x, flow, mask, status = ops.kitti_augment_full(frames, gt, pd, CROP)
            assert not status.any()
            tx, tf, tm = torch_chain(frames, gt, p, CROP)
            assert torch.equal(tx, x) and torch.equal(tf, flow) and torch.equal(tm, mask), "the torch chain and the kernel differ"
            us = timed(lambda: ops.kitti_augment_full(frames, gt, pd, CROP, out=(x, flow, mask), status=status))
            share = (src_bytes + out_bytes) / (us[0] * 1e-6) / 8e12
            print("(a) kernel   n=%2d %-8s: %7.1f us (window means %.1f - %.1f); algorithmic %.1f MB (%.1f read + %.1f written) = "
                  "%.1f %% of 8 TB/s" % (n, name, us[0], us[1], us[2], (src_bytes + out_bytes) / 1e6, src_bytes / 1e6, out_bytes / 1e6,
                                        100 * share))
            ut = timed(lambda: torch_chain(frames, gt, p, CROP))
            print("(b) torch    n=%2d %-8s: %7.1f us (window means %.1f - %.1f) = %.1fx the kernel; outputs bit-equal to the kernel's"
                  % (n, name, ut[0], ut[1], ut[2], ut[0] / us[0]))
            assert us[0] <= ut[0], "the fused launch is slower than the torch chain"
        # (c) the reduced pipeline at the same shape
        q = augment.make_params(n)
        for i, r in enumerate(AO.record(SIZE, y0=(7 * b) % 56, x0=(53 * b) % 347, warp=(2.0, 1.0815, 0.9215) if b % 2 == 0 else None,
                                        flip=b % 3 == 0) for b in range(n)):
            for k in q.dtype.names:
                q[k][i] = r[k]
        qd = torch.from_numpy(q.view(np.uint8).reshape(n, -1)).to(dev)
        rx, rf, rv, rs = ops.kitti_augment(frames, gt, qd, CROP)
        ur = timed(lambda: ops.kitti_augment(frames, gt, qd, CROP, out=(rx, rf, rv), status=rs))
        print("(c) reduced  n=%2d pwc_kitti_augment, every second sample warped: %7.1f us (window means %.1f - %.1f)" % (n, ur[0], ur[1], ur[2]))
        # (d) end to end, all stages on
        recs, p = records(n, **CONFIGS["all"])
        aug = augment_full.DeviceFullAugmenter(dev, n, SIZE, CROP, gt_kind=1)
        fx, ff, fm = (t.clone().cpu().pin_memory() for t in aug(samples, p))
        dx, df, dm = (torch.empty_like(t, device=dev) for t in (fx, ff, fm))

        def staged():
            aug(samples, p)
            torch.cuda.synchronize()

        def floats():
            dx.copy_(fx, non_blocking=True)
            df.copy_(ff, non_blocking=True)
            dm.copy_(fm, non_blocking=True)
            torch.cuda.synchronize()
        raw_mb = n * (2 * SIZE[0] * SIZE[1] * 3 + SIZE[0] * SIZE[1] * 6) / 1e6
        flt_mb = n * ch * cw * 9 * 4 / 1e6
        for rep in range(2):
            print("(d) end to end n=%2d reading %d: DeviceFullAugmenter (fill + upload %.1f MB + launch) %.2f ms, of which the fill of "
                  "the pinned slots on the host %.2f ms; upload of the finished float tensors (%.1f MB) %.2f ms"
                  % (n, rep, raw_mb, wall(staged), wall(lambda: aug.stage(samples, p)), flt_mb, wall(floats)))
    im1, im2, png = base[0]
    u, v, m = AO.decode_png(png)
    rec = records(1, **CONFIGS["all"])[0][0]
    t0, k = time.perf_counter(), 0
    while time.perf_counter() - t0 < 1.0:
        FO.augment_full((im1, im2, u, v, m), rec, CROP)
        k += 1
    print("(e) NumPy oracle on the host, one sample with all stages on: %.1f ms (cv2 is not installed: not timed)" %
          ((time.perf_counter() - t0) * 1e3 / k))


if __name__ == "__main__":
    main()
