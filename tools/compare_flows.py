#!/usr/bin/env python3
"""The reference's flow-comparison report (onnx_pth_compare.py compare_flows / print_flow_stats), computed on the device.

Two .flo files (A is the reference side, "pth"):

    python tools/compare_flows.py A.flo B.flo

Two precisions of the network on the seeded bench input (uniform [0,1) pairs, seed 1234; the checkpoint's weights, or the seeded
synthetic ones of bench.py without --weights):

    python tools/compare_flows.py [--weights W] --precision-a fp32 --precision-b fp16 --size 448x1024 [--batch 1]

Both forwards and the comparison run on the device; only the (n + 1) x 44 record is downloaded.  The script's colour images,
overlay, report canvas and ONNX parts are out of scope (cv2- / onnx-defined)."""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from opticalflow_amd import PWCDCNet, compare, read_flo  # noqa: E402
from opticalflow_amd.weights import load_checkpoint, synthetic_state_dict  # noqa: E402

GAIN, BIAS_STD = 0.85, 0.02      # bench.py's synthetic-weight recipe


def report_lines(cmp, names=("pth", "onnx")):
    """the batch row as the reference prints it: compare_flows' lines, then print_flow_stats of both fields"""
    n, _, H, W = cmp.shape
    shape = (n * H, W, 2)
    _, batch = cmp.to_host()
    lines = compare.format_report(batch, shape, shape)
    for name, f in zip(names, ("a", "b")):
        lines += compare.format_stats(name, shape, batch["stats"][f])
    return lines


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("flo", nargs="*", help="A.flo B.flo")
    ap.add_argument("--weights", default=None)
    ap.add_argument("--precision-a", default="fp32", choices=("fp32", "fp16", "fp16-strict"))
    ap.add_argument("--precision-b", default="fp16", choices=("fp32", "fp16", "fp16-strict"))
    ap.add_argument("--size", default="448x1024", help="HxW of the seeded input (multiples of 64)")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if len(args.flo) not in (0, 2):
        ap.error("give two .flo files, or none to compare two precisions of the network")
    dev = torch.device(args.device)
    if args.flo:
        fa, fb = (torch.from_numpy(read_flo(p)).permute(2, 0, 1)[None].contiguous() for p in args.flo)
        if fa.shape != fb.shape:
            sys.exit("the two fields differ in shape: %s and %s" % (tuple(fa.shape[2:]), tuple(fb.shape[2:])))
        cmp = compare.compare_flows(fa.to(dev), fb.to(dev))
        names = tuple(os.path.basename(p) for p in args.flo)
    else:
        H, W = (int(v) for v in args.size.lower().split("x"))
        nets = []
        for precision in (args.precision_a, args.precision_b):
            net = PWCDCNet(precision=precision)
            net.load_state_dict(load_checkpoint(args.weights) if args.weights
                                else synthetic_state_dict(net.manifest(), seed=0, gain=GAIN, bias_std=BIAS_STD))
            nets.append(net.to(dev).eval())
        x = torch.rand(args.batch, 6, H, W, generator=torch.Generator().manual_seed(1234)).to(dev)
        cmp = compare.compare_models(nets[0], nets[1], x)
        names = (args.precision_a, args.precision_b)
    print("\n".join(report_lines(cmp, names)))


if __name__ == "__main__":
    main()
