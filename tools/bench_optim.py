#!/usr/bin/env python3
"""The optimizer step on PWCDCNet's own 128 parameter tensors (9.37 M floats), HIP events after warm-up, the alternatives interleaved:
  fused-adamw-clip   opticalflow_amd.FusedAdamW(max_grad_norm=1.0).step()                       (three HIP launches)
  torch-foreach-clip clip_grad_norm_(1.0) + torch.optim.AdamW.step()                            (torch's default foreach path)
  torch-fused-clip   clip_grad_norm_(1.0) + torch.optim.AdamW(fused=True).step()
  fused-adam         opticalflow_amd.FusedAdam(weight_decay=4e-4).step(), no clipping           (two launches)
  torch-foreach-adam torch.optim.Adam(weight_decay=4e-4).step()
Every alternative owns a copy of the parameters and fixed gradients.  PWC_BENCH_ROUNDS rounds (default 7), in each round every
alternative runs PWC_BENCH_STEPS steps (default 50) between two events; the table gives the median over the rounds and their range.
Then the three launches of the fused step one by one (the same launch repeated between two events), with the bytes the algorithm
needs -- 4 N for the square sum, 28 N for the update (p, g, m, v read, p, m, v written) -- as a share of 8 TB/s, and the number of
device kernels of one step of each alternative counted with torch.profiler."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from opticalflow_amd import FusedAdam, FusedAdamW, ops, pwcnet  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS = int(os.environ.get("PWC_BENCH_ROUNDS", "7"))
STEPS = int(os.environ.get("PWC_BENCH_STEPS", "50"))
PEAK = 8e12


def make_params(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    ps = []
    for p in pwcnet.PWCDCNet(trainable=True).parameters():
        q = torch.nn.Parameter((torch.rand(p.shape, device=dev, generator=g) - 0.5))
        q.grad = (torch.rand(p.shape, device=dev, generator=g) - 0.5) * 0.02
        ps.append(q)
    return ps


def alternatives():
    alts = {}
    ps = make_params(1)
    opt = FusedAdamW(ps, lr=1e-4, weight_decay=1e-6, max_grad_norm=1.0)
    alts["fused-adamw-clip"] = (opt.step, opt)
    for name, kw in (("torch-foreach-clip", {}), ("torch-fused-clip", {"fused": True})):
        ps = make_params(1)
        opt = torch.optim.AdamW(ps, lr=1e-4, weight_decay=1e-6, **kw)

        def step(ps=ps, opt=opt):
            torch.nn.utils.clip_grad_norm_(ps, 1.0)
            opt.step()
        alts[name] = (step, opt)
    ps = make_params(1)
    opt = FusedAdam(ps, lr=1e-4, weight_decay=4e-4)
    alts["fused-adam"] = (opt.step, opt)
    ps = make_params(1)
    opt = torch.optim.Adam(ps, lr=1e-4, weight_decay=4e-4)
    alts["torch-foreach-adam"] = (opt.step, opt)
    return alts


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n          # us per call


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return str(sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
                       and "Memset" not in e.name))
    except Exception as e:      # the count is a side figure: say that it is missing instead of failing the timings
        return "not measured (%s)" % type(e).__name__


def main():
    alts = alternatives()
    n = sum(p.numel() for p in alts["fused-adamw-clip"][1].param_groups[0]["params"])
    print("PWCDCNet: %d tensors, %d floats; %d rounds x %d steps, alternatives interleaved" % (
        len(alts["fused-adamw-clip"][1].param_groups[0]["params"]), n, ROUNDS, STEPS))
    for fn, _ in alts.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in alts}
    for _ in range(ROUNDS):
        for k, (fn, _) in alts.items():
            times[k].append(timed(fn, STEPS))
    med = {k: statistics.median(v) for k, v in times.items()}
    print("%-20s %10s %10s %10s" % ("step", "median us", "min us", "max us"))
    for k, v in times.items():
        print("%-20s %10.1f %10.1f %10.1f" % (k, med[k], min(v), max(v)))
    print("fused-adamw-clip vs torch-foreach-clip: %.2fx; vs torch-fused-clip: %.2fx; fused-adam vs torch-foreach-adam: %.2fx" % (
        med["torch-foreach-clip"] / med["fused-adamw-clip"], med["torch-fused-clip"] / med["fused-adamw-clip"],
        med["torch-foreach-adam"] / med["fused-adam"]))

    opt = alts["fused-adamw-clip"][1]
    t = opt._tables
    launches = {
        "square sum": (lambda: ops.optim_grad_sqsum(t.grads, t.tensors, t.chunks, t.nchunks, 1, t.workspace), 4 * n),
        "finish": (lambda: ops.optim_finish(t.workspace, t.nchunks, 1, 0, 1.0, None, None, 1e-4, 0.9, 0.999, opt._steprec, opt._norm),
                   8 * t.nchunks),
        "update": (lambda: ops.optim_adam_update(t.grads, t.tensors, t.chunks, t.nchunks, 0, t.nchunks, 1, 0, t.workspace, 1e-4, 0.9,
                                                 0.999, 1e-8, 1e-6, True), 28 * n),
    }
    print("%-12s %10s %12s %14s   (%d chunks; the same launch repeated %d times between two events, %d rounds)" % (
        "launch", "median us", "bytes", "of 8 TB/s", t.nchunks, STEPS, ROUNDS))
    for k, (fn, nbytes) in launches.items():
        for _ in range(5):
            fn()
        us = statistics.median(timed(fn, STEPS) for _ in range(ROUNDS))
        print("%-12s %10.1f %12d %13.1f%%" % (k, us, nbytes, 100.0 * nbytes / (us * 1e-6) / PEAK))
    print("device kernels of one step: " + ", ".join("%s %s" % (k, kernel_count(fn)) for k, (fn, _) in alts.items()))


if __name__ == "__main__":
    main()
