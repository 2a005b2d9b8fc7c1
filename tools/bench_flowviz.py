#!/usr/bin/env python3
"""Flow pictures on the device against the host tail a caller had before, at 384x512 and 448x1024 frames, batch 1 and 16, fp32 net
with synthetic weights, all in one run.

Device path
  (a) the kernels alone on the stream's own flow, HIP events around back-to-back calls in windows of at least 0.5 s: ops.flow_stats
      (2 launches), ops.flow_color (1), ops.flow_quiver (1, step 16, style "video"), and the three together (4 launches).  With them
      the bytes the algorithm needs (flow read by stats, colour and the arrow taps; image, vectors, tips and flags written) as a share
      of the 8 TB/s HBM peak -- these kernels are latency-sized, the share says how far from a bandwidth problem they are, not what
      limits them (not measured);
  (b) one FlowStream graph replay without and with RenderSpec(color, quiver), HIP events, two alternating readings each;
  (c) frames/s end to end, wall clock around a loop that ends every push with its downloads: rendered stream + colour image + arrow
      grid to the host.
What a caller has today
  (d) FlowStream.push, flow.cpu(), then per sample on the host: a NumPy float32 statement of the colour wheel, harness.cv2_resize_linear
      of both planes to the frame size and the Python loop over the grid points (tips only, nothing drawn).  Wall clock, same loop.
(c) and (d) alternate twice; both readings are printed."""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import PWCDCNet, harness, ops, video  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict  # noqa: E402

dev = torch.device("cuda:0")
STEP = 16


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


def wall(fn, min_s=1.0):
    """calls per second of a function that ends synchronised"""
    for _ in range(2):
        fn()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < min_s:
        fn()
        n += 1
    return n / (time.perf_counter() - t0)


def _wheel():
    w = np.zeros((55, 3), np.float32)
    col = 0
    for n, full, ramp, up in ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False)):
        r = np.floor(255 * np.arange(n) / n)
        w[col:col + n, full] = 255
        w[col:col + n, ramp] = r if up else 255 - r
        col += n
    return w / np.float32(255)


WHEEL = _wheel()


def host_color(flow_hw2):
    """the colour wheel in NumPy float32 (what a caller writes on the host today)"""
    u, v = flow_hw2[..., 0], flow_hw2[..., 1]
    rad = np.sqrt(u * u + v * v)
    fk = (np.arctan2(-v, -u) / np.float32(np.pi) + 1) / 2 * 54 + 1
    k0 = np.floor(fk)
    f = (fk - k0)[..., None]
    k0 = (k0.astype(np.int64) - 1) % 55
    col = (1 - f) * WHEEL[k0] + f * WHEEL[(k0 + 1) % 55]
    rn = np.clip(rad / (rad.max() + np.float32(1e-5)), 0, 1)[..., None]
    return (np.clip(1 - rn * (1 - col), 0, 1) * 255).astype(np.uint8)


def host_arrows(flow_hw2, H, W):
    """resize both planes to the frame and walk the grid in Python, like create_quiver_frame without the drawing"""
    t = torch.from_numpy(flow_hw2)
    h, w = flow_hw2.shape[:2]
    u = (harness.cv2_resize_linear(t[..., 0].contiguous(), H, W) * (W / float(w))).numpy()
    v = (harness.cv2_resize_linear(t[..., 1].contiguous(), H, W) * (H / float(h))).numpy()
    out = []
    for y in range(0, H, STEP):
        for x in range(0, W, STEP):
            dx, dy = u[y, x], v[y, x]
            if (dx * dx + dy * dy) ** 0.5 < 0.5:
                continue
            out.append((x, y, int(round(x + dx)), int(round(y + dy))))
    return out


def main():
    net = PWCDCNet()
    net.load_state_dict(synthetic_state_dict(net.manifest(), seed=0, gain=0.85, bias_std=0.02))
    net = net.to(dev).eval()
    for H, W in ((384, 512), (448, 1024)):
        for B in (1, 16):
            tag = "%dx3x%dx%d" % (B, H, W)
            h, w = H // 4, W // 4
            gy, gx = -(-H // STEP), -(-W // STEP)
            spec = video.RenderSpec(color=True, quiver=dict(frame_hw=(H, W), step=STEP))
            plain = video.FlowStream(net, B, H, W, use_graph=True)
            rend = video.FlowStream(net, B, H, W, use_graph=True, render=spec)
            g = torch.Generator(device=dev).manual_seed(0)
            first = torch.rand(1, 3, H, W, device=dev, generator=g)
            frames = torch.roll(first, (2, -3), (2, 3)).expand(B, -1, -1, -1) * 0.9 + 0.1 * torch.rand(B, 3, H, W, device=dev, generator=g)
            plain.prime(first)
            rend.prime(first)
            flow = plain.push(frames).clone()
            # (a)
            r = rend.renderer
            t_stats = timed(lambda: ops.flow_stats(flow, out=r.stats, workspace=r.workspace))
            t_color = timed(lambda: ops.flow_color(flow, r.stats, out=r.color))
            t_quiv = timed(lambda: ops.flow_quiver(flow, H, W, STEP, (4.0, 4.0), 1.0, 0, 0.5, out=tuple(r.arrows)))
            t_all = timed(lambda: r.run(flow))
            fbytes = B * 2 * h * w * 4
            alg = 2 * fbytes + B * gy * gx * 8 * 4 + B * h * w * 3 + B * gy * gx * 17
            print("%-16s (a) kernels: stats %.1f us (2 launches)  colour %.1f us (1)  quiver %.1f us (1)  all three %.1f us (4 launches); "
                  "%.3f MB algorithmic = %.3f%% of 8 TB/s" % (tag, t_stats, t_color, t_quiv, t_all, alg / 1e6, 100.0 * alg / (t_all * 1e-6) / 8e12))
            # (b)
            p1, r1 = timed(lambda: plain.push(frames)), timed(lambda: rend.push(frames))
            p2, r2 = timed(lambda: plain.push(frames)), timed(lambda: rend.push(frames))
            print("%-16s (b) graph replay: plain %.1f / %.1f us  rendered %.1f / %.1f us  (+%.1f us, %.3fx)"
                  % (tag, p1, p2, r1, r2, min(r1, r2) - min(p1, p2), min(r1, r2) / min(p1, p2)))

            # (c) and (d)
            def device_path():
                rend.push(frames)
                rr = rend.rendered
                return rr.color.cpu(), [a.cpu() for a in rr.arrows]

            def host_path():
                f = plain.push(frames).cpu().numpy()
                return [(host_color(np.ascontiguousarray(f[b].transpose(1, 2, 0))),
                         host_arrows(np.ascontiguousarray(f[b].transpose(1, 2, 0)), H, W)) for b in range(B)]
            d1, h1 = wall(device_path), wall(host_path)
            d2, h2 = wall(device_path), wall(host_path)
            print("%-16s (c) rendered stream + downloads %.1f / %.1f frames/s   (d) push + .cpu() + host colour + resize + arrow loop "
                  "%.1f / %.1f frames/s   speedup %.2fx" % (tag, d1 * B, d2 * B, h1 * B, h2 * B, max(d1, d2) / max(h1, h2)))
            t0 = time.perf_counter()
            f = flow.cpu().numpy()
            t1 = time.perf_counter()
            host_color(np.ascontiguousarray(f[0].transpose(1, 2, 0)))
            t2 = time.perf_counter()
            host_arrows(np.ascontiguousarray(f[0].transpose(1, 2, 0)), H, W)
            t3 = time.perf_counter()
            print("%-16s     host tail, one reading: download %.2f ms, colour %.2f ms per sample, resize + arrow loop %.2f ms per sample"
                  % (tag, (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3))
            same = np.array_equal(host_color(np.ascontiguousarray(f[0].transpose(1, 2, 0))), r.run(flow).color[0].cpu().numpy())
            print("%-16s     device colour image == host float32 statement: %s" % (tag, same))
            del plain, rend


if __name__ == "__main__":
    main()
