#!/usr/bin/env python3
"""Which convolution kernel instantiations does the fp32 plan launch?  One eager forward per geometry of the plan-census grid
(tests/plan_census.py), of the benchmark / README sizes and of the launch audit's configurations, all in THIS process, each under
launch_audit.KernelSpy (no reference, no synchronisation inside a forward: milliseconds each).  Writes
{"kernels": sorted union, "geometries": {"BxHxW[/id]": indices into "kernels"}, "grid_union": indices} to --out (default
profiles/kernel_census_fp32.json); launch_audit.KERNELS_REQUIRED is pinned from "grid_union" (grid + benchmark sizes).

The run stops at the first error (nothing is launched after a fault) and the process ends itself after --time-limit seconds
(SIGALRM's default action), so a hang cannot outlive it; what was collected until then is written every 50 geometries.
usage: kernel_census.py [--out FILE] [--time-limit SECONDS]"""
import argparse
import json
import os
import signal
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import launch_audit as LA                                    # noqa: E402
import plan_census as PC                                     # noqa: E402
from opticalflow_amd import PWCDCNet, PWCDCNet_old, _lib, engine  # noqa: E402
from opticalflow_amd.weights import synthetic_state_dict    # noqa: E402

BENCH = [(b, 448, 1024) for b in (1, 2, 4, 8, 16, 32)]      # bench.py's workload and the README's batch sweep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_census_fp32.json"))
    ap.add_argument("--time-limit", type=int, default=420)
    args = ap.parse_args()
    signal.alarm(args.time_limit)
    from test_gpu_launch_audit import CONFIGS
    dev = torch.device("cuda:0")
    params = {}
    for variant, cls in (("dc", PWCDCNet), ("old", PWCDCNet_old)):
        sd = synthetic_state_dict(cls().manifest(), seed=0, gain=0.85, bias_std=0.02)
        params[variant] = {k: v.to(dev) for k, v in sd.items()}
    jobs = [("%dx%dx%d" % g, "dc", g, None, "grid") for g in PC.grid()]
    jobs += [("%dx%dx%d" % g, "dc", g, None, "bench") for g in BENCH]
    jobs += [("%dx%dx%d/%s" % (b, h, w, cid), variant, (b, h, w), opts, "config") for cid, variant, b, h, w, opts, _ in CONFIGS]
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    seen, union, grid_union = {}, set(), set()

    def write():
        names = sorted(union)
        idx = {k: i for i, k in enumerate(names)}
        out = {"cus": cus, "kernels": names, "grid_union": sorted(idx[k] for k in grid_union),
               "geometries": {g: sorted(idx[k] for k in ks) for g, ks in seen.items()}}
        with open(args.out + ".tmp", "w") as f:
            json.dump(out, f, sort_keys=True, separators=(",", ":"))
            f.write("\n")
        os.replace(args.out + ".tmp", args.out)

    t0 = time.time()
    for i, (name, variant, (b, h, w), opts, kind) in enumerate(jobs):
        saved = {k: _lib.get_option(k) for k in (opts or {})}
        for k, v in (opts or {}).items():
            _lib.set_option(k, v)
        plan = engine.PwcPlan(params[variant], b, h, w, dev, variant=variant)
        x = torch.rand((b, 6, h, w), device=dev)
        with LA.KernelSpy() as spy, torch.no_grad():
            plan.run(x)
        torch.cuda.synchronize()                             # a fault of this forward surfaces here, before the next one starts
        for k, v in saved.items():
            _lib.set_option(k, v)
        del plan, x
        seen.setdefault(name, spy.kernels)
        union |= spy.kernels
        if kind != "config":
            grid_union |= spy.kernels
        if i % 50 == 49:
            write()
    write()
    print("%d forwards in %.1f s on %d CUs: %d kernel instantiations (%d on the grid and benchmark sizes) -> %s" % (
        len(jobs), time.time() - t0, cus, len(union), len(grid_union), args.out))


if __name__ == "__main__":
    main()
