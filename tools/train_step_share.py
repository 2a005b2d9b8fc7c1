#!/usr/bin/env python3
"""Kernel time of the TIMED steps of tools/bench_train.py, from a rocprofv3 kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o train -- python tools/bench_train.py fused
    python tools/train_step_share.py DIR/train_kernel_trace.csv [out.csv]
bench_train.py pauses 1 s between its warm-up steps (which include MIOpen's solver search: trial kernels of tens of ms) and its
timed steps; the trace is cut at its last idle gap of 0.5 s or more and only the dispatches after it are counted.  Steps are counted by the
level-6 cost-volume backward (warp_corr81_bwd_kernel<false>, one launch per step).  Prints the shares of kernel groups per step and
writes per-kernel rows (Name, Calls, TotalDurationNs, AverageNs, Percentage) of the timed steps to out.csv."""
import csv
import sys

GROUPS = (
    ("fused cost-volume backward (pwc_warp_corr81_bwd: prepass, main pass, grad_flo / grad_c2 passes)",
     ("warp_corr81_bwd_kernel", "absmax_bits_kernel", "flo_reduce_kernel", "fixed_to_float_kernel")),
    ("fused cost-volume forward (pwc_warp_corr81_fwd / pwc_corr_fwd / pwc_warp_fwd)",
     ("warp_corr81_pipe_kernel", "corr81_dma_kernel", "corr81_kernel", "corr_small", "corr81_small", "warp_kernel")),
    ("convolutions, forward and backward (MIOpen / composable_kernel)",
     ("naive_conv", "igemm_", "miopen", "Conv", "conv", "ck::", "_ZN2ck", "gemm", "Gemm", "transpose")),
)


def main():
    rows = []
    for r in csv.DictReader(open(sys.argv[1])):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    # the LAST idle gap of at least 0.5 s (warm-up may hold long gaps of its own while MIOpen compiles); no such gap: the largest
    big, cut_big, last, cut_last, last_end = -1, 0, -1, None, rows[0][1]
    for i in range(len(rows) - 1):                     # idle time before dispatch i+1: after every earlier dispatch has ended
        last_end = max(last_end, rows[i][1])
        g = rows[i + 1][0] - last_end
        if g > big:
            big, cut_big = g, i
        if g >= 500_000_000:
            last, cut_last = g, i
    gap, cut = (last, cut_last) if cut_last is not None else (big, cut_big)
    timed = rows[cut + 1:]
    steps = sum(1 for _, _, n in timed if "warp_corr81_bwd_kernel<false>" in n)
    per = {}
    for s, e, n in timed:
        t, c = per.get(n, (0, 0))
        per[n] = (t + (e - s), c + 1)
    tot = sum(t for t, _ in per.values())
    print("cut at an idle gap of %.0f ms; %d timed steps, %d dispatches, kernel time %.2f ms per step"
          % (gap / 1e6, steps, len(timed), tot / 1e6 / max(steps, 1)))
    rest = dict(per)
    for label, keys in GROUPS:
        t = 0
        for n in list(rest):
            if any(k in n for k in keys):
                t += rest.pop(n)[0]
        print("  %5.1f %%  %7.2f ms/step  %s" % (100 * t / tot, t / 1e6 / max(steps, 1), label))
    t = sum(v[0] for v in rest.values())
    print("  %5.1f %%  %7.2f ms/step  everything else (PyTorch elementwise / cat / reductions / SGD, runtime copies)"
          % (100 * t / tot, t / 1e6 / max(steps, 1)))
    for n, (t, c) in sorted(per.items(), key=lambda kv: -kv[1][0])[:12]:
        print("    %5.2f %%  %4d x %9.1f us  %s" % (100 * t / tot, c, t / c / 1e3, n[:100]))
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w", newline="") as f:
            w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
            w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage"])
            for n, (t, c) in sorted(per.items(), key=lambda kv: -kv[1][0]):
                w.writerow([n, c, t, t / c, 100.0 * t / tot])


if __name__ == "__main__":
    main()
