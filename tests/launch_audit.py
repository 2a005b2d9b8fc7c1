"""Launch audit of the fp32 inference plan (tests/test_gpu_launch_audit.py): every ops.* launch of one eager forward is recorded,
re-computed from its own recorded inputs as ONE operator in float64 on the CPU, and compared per element.

Bounds (per output element, never a mean):
  * convolutions, deconvolutions, flow heads:  |got - ref| <= REL_<route> x (sum |x||w| + |b| (+ |residual|)), the form of
    test_gpu_parity._wino4_rel_errors / WINO4_REL_BAR;
  * correlation (plain and fused with the warp): |got - ref| <= REL_CORR x sum |c1||w2| (the absolute cost volume);
  * the warp: |got - ref| <= REL_WARP x sum of |tap weight| |x|;
  * permutations and copies (densify, lattice_unsplit, the up_feat phases of upsample_entry): bit-exact.
The warp's sample coordinates, tap cells, weights and mask come from the kernel's own float32 arithmetic (pwc_warp_taps.h,
built with -ffp-contract=off and IEEE division), restated here in float32 torch ops; everything after the taps is float64.  So
the mask decisions agree exactly; pixels whose float64 mask sum lies within 1e-6 of the threshold are still counted and left out.

Route labels come from the same public queries the plan uses (*_preferred, *_workspace_bytes, _lib.get_option, tile counts).
Every convolution record also keeps the kernel instantiation the library launched (pwc_last_conv_kernel, read right after the
launch: name and template arguments, "/split" where the launch went through the split workspace), as tests/launch_audit_f16.py does.
The 16 -> 16 Winograd launches of the first pyramid level are checked too: one layer like any F(2x2) launch; the two-layer launch
against the float64 composition under  REL_WINO2 x (sum |w2| S1 + S2),  S1 the first layer's sum of |terms| (its error, bounded by
REL_WINO2 x S1, passes LeakyReLU with slope <= 1 and is weighted by |w2|) and S2 the second layer's over the float64 intermediate.
This module is a helper, not a test module (tests/f16_error_budget.py is the precedent)."""
from __future__ import annotations

import inspect
import random
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

LEAKY = 0.1

# ---- bounds per route family: multiples of the sum of |terms| of each output element ------------------------------------------
REL_DIRECT = 1.0e-6        # direct MFMA / VALU kernels and their split-K form: fp32 accumulation
REL_WINO2 = 1.0e-6         # F(2x2,3x3): transforms with coefficients +-1 (test_conv3x3_winograd_vs_fp64)
REL_WINO4 = 2.0e-6         # F(4x4,3x3): WINO4_REL_BAR of tests/test_gpu_parity.py
REL_HEAD = 1.0e-6          # streaming predict_flowL + upfeatL (one pass or Cin slices, fixed-order reduction)
REL_DECONV = 1.0e-6        # ConvTranspose2d(4, 2, 1) kernels
REL_CORR = 1.0e-6          # correlation, fused or not, against sum |c1||w2|
REL_WARP = 1.0e-6          # bilinear blend of four taps
MASK_EPS = 1.0e-6          # float64 mask sums this close to the threshold are excluded ...
MASK_EXCLUDED_MAX = 1.0e-3  # ... and must stay under this share of a level's pixels

# ---- routes the suite must reach (test_route_coverage): adding or removing one is an edit of this list ----------------------------
ROUTES_REQUIRED = (
    "densify",
    "conv/direct/s2", "conv/direct", "conv/direct/dilated", "conv/direct/residual", "conv/direct/split-k",
    "conv/wino2", "conv/wino2/dilated", "conv/wino2/split-k",
    "conv/wino4", "conv/wino4/cin-split", "conv/wino4/split2",
    "conv/split96/wino4", "conv/split96/wino2",
    "head/head10", "head/upsample-entry", "head/upfeat", "head/upfeat-sliced", "head/conv", "deconv",
    "entry/fused-window", "entry/fused-r2", "entry/warp", "entry/corr-small", "entry/corr-level6",
    "ctx/lattice-unsplit",
    "pyr1/wino2",
)

# ---- kernel instantiations the suite must launch (test_kernel_coverage) ---------------------------------------------------------------
# Every label the fp32 plan produced on the census grid (plan_census.grid(), default options) and at 448x1024 with batch 1, 2, 4, 8, 16
# and 32, as tools/kernel_census.py collected them on an MI355X (profiles/kernel_census_fp32.json, "grid_union").  A label is what
# pwc_last_conv_kernel reports after the launch -- for a layer the library runs as two launches (F(4x4): a 64-cout and a 32-cout one)
# the LAST of them -- plus "/split" where the layer went through the split workspace.  conv3x3_mfma_kernel<MT, NT, stride, dilation,
# two per CU, 16 = folded tile>, conv3x3_wino4p_kernel<CB, TG, GW, Cin slices, 1, IH>, conv3x3_wino8r_kernel<MT, TG, 1, dilation, 1, 0>
KERNELS_REQUIRED = (
    "conv3x3_head_kernel<2, 0, 0, 0, 0, 0>",
    "conv3x3_mfma16_kernel<1, 4, 1, 1, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 1, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 1, 1, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 1, 1, 16>",
    "conv3x3_mfma_kernel<1, 1, 1, 16, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 16, 1, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 2, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 2, 1, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 4, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 4, 1, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 8, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 1, 8, 1, 0>",
    "conv3x3_mfma_kernel<1, 1, 2, 1, 0, 0>",
    "conv3x3_mfma_kernel<1, 1, 2, 1, 1, 0>",
    "conv3x3_mfma_kernel<1, 1, 2, 1, 1, 16>",
    "conv3x3_mfma_kernel<1, 2, 1, 4, 1, 0>",
    "conv3x3_mfma_kernel<1, 2, 1, 8, 1, 0>",
    "conv3x3_mfma_kernel<1, 2, 2, 1, 1, 0>",
    "conv3x3_mfma_kernel<2, 1, 1, 2, 1, 0>",
    "conv3x3_mfma_kernel<2, 1, 1, 4, 1, 0>",
    "conv3x3_mfma_kernel<2, 1, 2, 1, 1, 0>",
    "conv3x3_mfma_kernel<2, 2, 2, 1, 1, 0>",
    "conv3x3_mfma_kernel<3, 1, 1, 1, 1, 0>",
    "conv3x3_mfma_kernel<3, 1, 2, 1, 1, 0>",
    "conv3x3_mfma_kernel<3, 2, 2, 1, 1, 0>",
    "conv3x3_mfma_splitk_kernel<1, 1, 1, 1, 0, 0>/split",
    "conv3x3_mfma_splitk_kernel<1, 1, 1, 1, 0, 16>/split",
    "conv3x3_wino4p_kernel<2, 4, 32, 1, 1, 16>",
    "conv3x3_wino4p_kernel<2, 4, 32, 2, 1, 16>/split",
    "conv3x3_wino4p_kernel<2, 4, 32, 4, 1, 16>/split",
    "conv3x3_wino4p_kernel<2, 4, 32, 8, 1, 0>/split",
    "conv3x3_wino4p_kernel<2, 4, 64, 1, 1, 0>",
    "conv3x3_wino4p_kernel<2, 4, 64, 1, 1, 0>/split",
    "conv3x3_wino4p_kernel<2, 4, 64, 2, 1, 0>/split",
    "conv3x3_wino4p_kernel<2, 4, 64, 4, 1, 0>/split",
    "conv3x3_wino4p_kernel<2, 4, 64, 7, 1, 0>/split",
    "conv3x3_wino4p_kernel<2, 4, 64, 8, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 16, 1, 1, 8>",
    "conv3x3_wino4p_kernel<4, 2, 16, 2, 1, 8>/split",
    "conv3x3_wino4p_kernel<4, 2, 16, 4, 1, 8>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 2, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 3, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 4, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 5, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 6, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 7, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 32, 8, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 1, 1, 0>",
    "conv3x3_wino4p_kernel<4, 2, 64, 1, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 2, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 3, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 4, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 5, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 6, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 7, 1, 0>/split",
    "conv3x3_wino4p_kernel<4, 2, 64, 8, 1, 0>/split",
    "conv3x3_wino8r_kernel<1, 4, 1, 1, 1, 0>",
    "conv3x3_wino8r_kernel<1, 4, 1, 1, 1, 0>/split",
    "conv3x3_wino8r_kernel<2, 2, 1, 1, 1, 0>",
    "conv3x3_wino8r_kernel<2, 2, 1, 1, 1, 0>/split",
    "conv3x3_wino8r_kernel<4, 1, 1, 1, 1, 0>",
    "conv3x3_wino8r_kernel<4, 1, 1, 1, 1, 0>/split",
    "conv3x3_wino8r_kernel<4, 1, 1, 2, 1, 0>",
    "conv3x3_wino8r_kernel<4, 1, 1, 4, 1, 0>",
    "image_conv_s2_f32_kernel<1, 2, 2, 1, 0, 0>",
    "pyr1_wino2<8, 64, 0, 0, 0, 0>",
    "stream3x3_kernel<1, 4, 4, 0, 0, 0>",
    "stream3x3_kernel<1, 4, 4, 1, 0, 0>/split",
    "stream3x3_kernel<1, 8, 1, 0, 0, 0>",
    "stream3x3_kernel<3, 4, 4, 0, 0, 0>",
    "stream3x3_kernel<3, 4, 4, 1, 0, 0>",
)

# ---- tile instantiations of the direct kernel that no fp32 plan launches (test_gpu_parity.test_conv3x3_tile_instantiations_vs_fp64) ----
# Every entry of pwc_conv_mfma.h's tile tables that KERNELS_REQUIRED does not hold (tests/test_conv_tiles_cpu.py asserts that the two
# together are exactly the tables), each at a shape for which the cost model (choose_tile) picks it, the cheapest that
# tools/conv_tile_census.hip finds (profiles/conv_tile_census.txt): (B, Cin, Cout, H, W, stride, dilation, kernel).
# Cin is ragged against the 4- / 8-channel chunks, W against the 32-column tile, H against the 4 NT-row tile wherever the model allows.
# The two-per-CU variants (fifth argument 1) need more than 256 workgroups, the one-per-CU 96-cout ones a long K loop: hence B and Cin
TILE_CASES = [
    (1, 5, 196, 4, 20, 1, 1, "conv3x3_mfma_kernel<2, 1, 1, 1, 0, 0>"),
    (4, 197, 384, 30, 36, 1, 1, "conv3x3_mfma_kernel<3, 1, 1, 1, 0, 0>"),
    (4, 197, 288, 250, 36, 1, 1, "conv3x3_mfma_kernel<3, 2, 1, 1, 0, 0>"),
    (8, 101, 96, 250, 100, 1, 1, "conv3x3_mfma_kernel<3, 4, 1, 1, 0, 0>"),
    (32, 861, 356, 2, 228, 1, 1, "conv3x3_mfma_kernel<4, 1, 1, 1, 0, 0>"),
    (32, 541, 324, 5, 228, 1, 1, "conv3x3_mfma_kernel<4, 2, 1, 1, 0, 0>"),
    (32, 141, 100, 125, 36, 1, 1, "conv3x3_mfma_kernel<4, 4, 1, 1, 0, 0>"),
    (12, 13, 32, 100, 36, 1, 1, "conv3x3_mfma_kernel<1, 2, 1, 1, 1, 0>"),
    (32, 13, 160, 9, 72, 1, 1, "conv3x3_mfma_kernel<1, 4, 1, 1, 1, 0>"),
    (12, 13, 256, 9, 36, 1, 1, "conv3x3_mfma_kernel<2, 1, 1, 1, 1, 0>"),
    (7, 13, 48, 200, 36, 1, 1, "conv3x3_mfma_kernel<2, 2, 1, 1, 1, 0>"),
    (32, 13, 48, 100, 36, 1, 1, "conv3x3_mfma_kernel<2, 4, 1, 1, 1, 0>"),
    (20, 13, 160, 36, 36, 1, 1, "conv3x3_mfma_kernel<3, 2, 1, 1, 1, 0>"),
    (32, 13, 196, 9, 36, 1, 1, "conv3x3_mfma_kernel<4, 1, 1, 1, 1, 0>"),
    (32, 13, 100, 50, 36, 1, 1, "conv3x3_mfma_kernel<4, 2, 1, 1, 1, 0>"),
    (1, 5, 196, 4, 20, 1, 2, "conv3x3_mfma_kernel<2, 1, 1, 2, 0, 0>"),
    (4, 197, 384, 30, 36, 1, 2, "conv3x3_mfma_kernel<3, 1, 1, 2, 0, 0>"),
    (4, 197, 288, 250, 36, 1, 2, "conv3x3_mfma_kernel<3, 2, 1, 2, 0, 0>"),
    (8, 101, 96, 250, 100, 1, 2, "conv3x3_mfma_kernel<3, 4, 1, 2, 0, 0>"),
    (32, 861, 356, 3, 228, 1, 2, "conv3x3_mfma_kernel<4, 1, 1, 2, 0, 0>"),
    (32, 541, 324, 5, 228, 1, 2, "conv3x3_mfma_kernel<4, 2, 1, 2, 0, 0>"),
    (32, 141, 100, 125, 36, 1, 2, "conv3x3_mfma_kernel<4, 4, 1, 2, 0, 0>"),
    (5, 13, 32, 250, 36, 1, 2, "conv3x3_mfma_kernel<1, 2, 1, 2, 1, 0>"),
    (32, 13, 160, 9, 72, 1, 2, "conv3x3_mfma_kernel<1, 4, 1, 2, 1, 0>"),
    (7, 13, 48, 200, 36, 1, 2, "conv3x3_mfma_kernel<2, 2, 1, 2, 1, 0>"),
    (32, 13, 48, 100, 36, 1, 2, "conv3x3_mfma_kernel<2, 4, 1, 2, 1, 0>"),
    (32, 13, 160, 9, 36, 1, 2, "conv3x3_mfma_kernel<3, 1, 1, 2, 1, 0>"),
    (20, 13, 160, 36, 36, 1, 2, "conv3x3_mfma_kernel<3, 2, 1, 2, 1, 0>"),
    (32, 13, 196, 9, 36, 1, 2, "conv3x3_mfma_kernel<4, 1, 1, 2, 1, 0>"),
    (32, 13, 100, 50, 36, 1, 2, "conv3x3_mfma_kernel<4, 2, 1, 2, 1, 0>"),
    (1, 5, 196, 4, 20, 1, 4, "conv3x3_mfma_kernel<2, 1, 1, 4, 0, 0>"),
    (17, 629, 292, 141, 20, 1, 4, "conv3x3_mfma_kernel<2, 4, 1, 4, 0, 0>"),
    (1, 197, 384, 120, 36, 1, 4, "conv3x3_mfma_kernel<3, 1, 1, 4, 0, 0>"),
    (4, 197, 288, 250, 36, 1, 4, "conv3x3_mfma_kernel<3, 2, 1, 4, 0, 0>"),
    (8, 101, 288, 60, 136, 1, 4, "conv3x3_mfma_kernel<3, 4, 1, 4, 0, 0>"),
    (32, 485, 228, 21, 36, 1, 4, "conv3x3_mfma_kernel<4, 1, 1, 4, 0, 0>"),
    (32, 205, 324, 5, 228, 1, 4, "conv3x3_mfma_kernel<4, 2, 1, 4, 0, 0>"),
    (8, 101, 256, 250, 36, 1, 4, "conv3x3_mfma_kernel<4, 4, 1, 4, 0, 0>"),
    (32, 13, 160, 9, 72, 1, 4, "conv3x3_mfma_kernel<1, 4, 1, 4, 1, 0>"),
    (7, 13, 48, 200, 36, 1, 4, "conv3x3_mfma_kernel<2, 2, 1, 4, 1, 0>"),
    (32, 13, 48, 100, 36, 1, 4, "conv3x3_mfma_kernel<2, 4, 1, 4, 1, 0>"),
    (32, 13, 160, 9, 36, 1, 4, "conv3x3_mfma_kernel<3, 1, 1, 4, 1, 0>"),
    (32, 13, 160, 18, 36, 1, 4, "conv3x3_mfma_kernel<3, 2, 1, 4, 1, 0>"),
    (32, 13, 196, 9, 36, 1, 4, "conv3x3_mfma_kernel<4, 1, 1, 4, 1, 0>"),
    (5, 13, 196, 150, 36, 1, 4, "conv3x3_mfma_kernel<4, 2, 1, 4, 1, 0>"),
    (1, 5, 196, 4, 20, 1, 8, "conv3x3_mfma_kernel<2, 1, 1, 8, 0, 0>"),
    (4, 197, 384, 30, 36, 1, 8, "conv3x3_mfma_kernel<3, 1, 1, 8, 0, 0>"),
    (4, 197, 288, 250, 36, 1, 8, "conv3x3_mfma_kernel<3, 2, 1, 8, 0, 0>"),
    (17, 981, 356, 57, 20, 1, 8, "conv3x3_mfma_kernel<4, 1, 1, 8, 0, 0>"),
    (32, 541, 324, 29, 36, 1, 8, "conv3x3_mfma_kernel<4, 2, 1, 8, 0, 0>"),
    (12, 13, 256, 9, 36, 1, 8, "conv3x3_mfma_kernel<2, 1, 1, 8, 1, 0>"),
    (7, 13, 48, 200, 36, 1, 8, "conv3x3_mfma_kernel<2, 2, 1, 8, 1, 0>"),
    (32, 13, 160, 9, 36, 1, 8, "conv3x3_mfma_kernel<3, 1, 1, 8, 1, 0>"),
    (20, 13, 160, 36, 36, 1, 8, "conv3x3_mfma_kernel<3, 2, 1, 8, 1, 0>"),
    (32, 13, 196, 9, 36, 1, 8, "conv3x3_mfma_kernel<4, 1, 1, 8, 1, 0>"),
    (32, 13, 100, 50, 36, 1, 8, "conv3x3_mfma_kernel<4, 2, 1, 8, 1, 0>"),
    (1, 5, 196, 4, 20, 1, 16, "conv3x3_mfma_kernel<2, 1, 1, 16, 0, 0>"),
    (4, 197, 384, 30, 36, 1, 16, "conv3x3_mfma_kernel<3, 1, 1, 16, 0, 0>"),
    (4, 197, 288, 250, 36, 1, 16, "conv3x3_mfma_kernel<3, 2, 1, 16, 0, 0>"),
    (5, 13, 32, 250, 36, 1, 16, "conv3x3_mfma_kernel<1, 2, 1, 16, 1, 0>"),
    (12, 13, 256, 9, 36, 1, 16, "conv3x3_mfma_kernel<2, 1, 1, 16, 1, 0>"),
    (32, 13, 196, 9, 36, 1, 16, "conv3x3_mfma_kernel<2, 2, 1, 16, 1, 0>"),
    (32, 13, 160, 9, 36, 1, 16, "conv3x3_mfma_kernel<3, 1, 1, 16, 1, 0>"),
    (7, 13, 196, 75, 36, 1, 16, "conv3x3_mfma_kernel<3, 2, 1, 16, 1, 0>"),
    (1, 5, 196, 4, 20, 2, 1, "conv3x3_mfma_kernel<2, 1, 2, 1, 0, 0>"),
    (8, 197, 384, 10, 200, 2, 1, "conv3x3_mfma_kernel<3, 1, 2, 1, 0, 0>"),
    (8, 197, 288, 250, 72, 2, 1, "conv3x3_mfma_kernel<3, 2, 2, 1, 0, 0>"),
    (32, 861, 356, 3, 456, 2, 1, "conv3x3_mfma_kernel<4, 1, 2, 1, 0, 0>"),
    (32, 541, 324, 57, 72, 2, 1, "conv3x3_mfma_kernel<4, 2, 2, 1, 0, 0>"),
    (32, 13, 196, 9, 136, 2, 1, "conv3x3_mfma_kernel<4, 1, 2, 1, 1, 0>"),
    (20, 13, 196, 75, 72, 2, 1, "conv3x3_mfma_kernel<4, 2, 2, 1, 1, 0>"),
    (4, 16, 16, 224, 512, 1, 1, "conv3x3_mfma16_kernel<2, 4, 1, 1, 0, 0>"),       # the 16-cout kernel's 8-row ...
    (10, 16, 16, 224, 500, 1, 1, "conv3x3_mfma16_kernel<4, 4, 1, 1, 0, 0>"),      # ... and 16-row tiles
]

OPS = ("densify", "conv3x3", "conv3x3_wino", "conv3x3_wino4", "pyr1_wino", "pyr1_wino_pair", "warp_correlation", "warp", "correlation",
       "head_upfeat", "upsample_entry", "deconv4x4s2", "lattice_unsplit")


def last_kernel(split: bool = False) -> str:
    """the convolution kernel the library launched last on this thread: name<template arguments>[/split]"""
    from opticalflow_amd import _lib
    return _lib.load().pwc_last_conv_kernel().decode() + ("/split" if split else "")


CONV_OPS = ("conv3x3", "conv3x3_wino", "conv3x3_wino4", "pyr1_wino", "pyr1_wino_pair", "head_upfeat")


def split_need(op: str, A: Dict) -> int:
    """bytes of split workspace the launch `op`(**A) wants (0: it does not split; the pyramid kernels never do)"""
    from opticalflow_amd import ops
    if op not in ("conv3x3", "conv3x3_wino", "conv3x3_wino4"):
        return 0
    n, cin, h, w = A["x"].shape
    if op == "conv3x3":
        return ops.conv3x3_workspace_bytes(n, cin, h, w, A["cout"], A["stride"], A["dilation"])
    if op == "conv3x3_wino":
        return ops.conv3x3_wino_workspace_bytes(n, cin, h, w, A["cout"], A["dilation"])
    return ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, A["cout"])


def used_split(op: str, A: Dict) -> bool:
    """did the launch go through the split workspace?  (every C entry splits when the buffer it is given covers its demand)"""
    ws, need = A.get("workspace"), split_need(op, A)
    return bool(ws is not None and 0 < need <= ws.numel() * ws.element_size())


class KernelSpy:
    """Context manager: wraps the convolution operators of opticalflow_amd.ops, launches them unchanged and collects the kernel
    label of each (`kernels`), with no reference and no synchronisation -- tools/kernel_census.py runs hundreds of forwards under it."""

    def __init__(self):
        self.kernels = set()
        self._real = {}

    def __enter__(self):
        from opticalflow_amd import ops
        for n in CONV_OPS:
            self._real[n] = getattr(ops, n)
            setattr(ops, n, self._wrap(n, self._real[n]))
        return self

    def __exit__(self, *exc):
        from opticalflow_amd import ops
        for n, f in self._real.items():
            setattr(ops, n, f)
        return False

    def _wrap(self, name, real):
        sig = inspect.signature(real)

        def f(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            out = real(*a, **kw)
            self.kernels.add(last_kernel(used_split(name, ba.arguments)))
            return out
        return f


def pick_images(n: int, seed: int) -> List[int]:
    """every image of a launch of <= 4, else the first, the last and two seeded others (<= 8 took the suite over its time budget:
    batch 8 at 448x1024 alone 40 s)"""
    if n <= 4:
        return list(range(n))
    rng = random.Random(seed)
    return sorted({0, n - 1, *rng.sample(range(1, n - 1), 2)})


# ---- comparators (CPU tensors; used by the GPU audit and by tests/test_launch_audit_cpu.py) -----------------------------------
def bounded_ratio(got: torch.Tensor, ref: torch.Tensor, scale: torch.Tensor, rel: float,
                  keep: Optional[torch.Tensor] = None) -> torch.Tensor:
    """|got - ref| / (rel x scale) per element (> 1: out of bound); `keep` (broadcastable bool) masks excluded elements to 0.
    A zero scale with a non-zero error is infinitely out of bound (an exact operation must stay exact)."""
    err = (got.double() - ref.double()).abs()
    den = rel * scale.double()
    r = torch.where(den > 0, err / den.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    if keep is not None:
        r = torch.where(keep, r, torch.zeros_like(r))
    return r


def worst(ratio: torch.Tensor):
    """(max ratio, index of it as a tuple, channels (dim 1, or 0 for 3-D) whose max ratio exceeds 1)"""
    m = ratio.max()
    idx = tuple(int(i) for i in torch.nonzero(ratio == m)[0]) if ratio.numel() else ()
    cdim = 1 if ratio.dim() == 4 else 0
    per_c = ratio.transpose(0, cdim).reshape(ratio.shape[cdim], -1).max(1).values
    return float(m), idx, [int(c) for c in torch.nonzero(per_c > 1).flatten()]


def conv_ref(x, w, b, stride=1, dilation=1, act=True, residual=None):
    """float64 reference of one 3x3 convolution launch and the sum of |terms| of each output"""
    xd, wd = x.double(), w.double()
    y = F.conv2d(xd, wd, b.double(), stride=stride, padding=dilation, dilation=dilation)
    s = F.conv2d(x.float().abs(), w.float().abs(), b.float().abs(), stride=stride, padding=dilation, dilation=dilation).double()
    if act:
        y = F.leaky_relu(y, LEAKY)
    if residual is not None:
        y = y + residual.double()
        s = s + residual.double().abs()
    return y, s


def deconv_ref(x, w, b):
    y = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    s = F.conv_transpose2d(x.float().abs(), w.float().abs(), b.float().abs(), stride=2, padding=1).double()
    return y, s


def split2(t: torch.Tensor) -> torch.Tensor:
    """[n,C,H,W] -> its four pixel lattices [4n,C,H/2,W/2], image 4i + 2(y&1) + (x&1) (PWC_CONV_SPLIT2)"""
    n, c, h, w = t.shape
    return torch.stack([t[:, :, py::2, px::2] for py in range(2) for px in range(2)], 1).reshape(4 * n, c, h // 2, w // 2)


def unsplit(t: torch.Tensor, levels: int) -> torch.Tensor:
    """inverse of `levels` nested split2 (restated independently of the kernel)"""
    for _ in range(levels):
        n4, c, h, w = t.shape
        q = t.reshape(n4 // 4, 2, 2, c, h, w)
        out = t.new_empty((n4 // 4, c, 2 * h, 2 * w))
        for py in range(2):
            for px in range(2):
                out[:, :, py::2, px::2] = q[:, py, px]
        t = out
    return t


def corr_ref(c1, w2, normalize=False, act=True):
    """float64 cost volume of PWC-Net's correlation (pad 4, k 1, d 4) + LeakyReLU, and sum |c1||w2| per output"""
    from oracle import pwc_oracle as O
    y = O.correlation(c1.double(), w2.double(), 4, 1, 4, 1, 1, 1, normalize=normalize)
    s = O.correlation(c1.double().abs(), w2.double().abs(), 4, 1, 4, 1, 1, 1, normalize=normalize)
    if act:
        y = F.leaky_relu(y, LEAKY)
    return y, s


def warp_taps(flo: torch.Tensor, scale: float, align: bool, thr: float):
    """The kernel's taps (pwc_warp_taps.h make_taps) in float32: (x0, y0, [w00, w01, w10, w11] masked, fp64 mask sum, mask,
    (ax1, ay1, [in-bounds of the four taps])) -- the last item serves the derivative with respect to the sample coordinate."""
    B, _, H, W = flo.shape
    f32 = torch.float32
    u = flo[:, 0].float() * torch.tensor(scale, dtype=f32)
    v = flo[:, 1].float() * torch.tensor(scale, dtype=f32)
    px = torch.arange(W, dtype=f32).view(1, 1, W) + u
    py = torch.arange(H, dtype=f32).view(1, H, 1) + v
    gx = 2.0 * px / float(max(W - 1, 1)) - 1.0
    gy = 2.0 * py / float(max(H - 1, 1)) - 1.0
    if align:
        ix = (gx + 1.0) / 2.0 * float(W - 1)
        iy = (gy + 1.0) / 2.0 * float(H - 1)
    else:
        ix = ((gx + 1.0) * float(W) - 1.0) / 2.0
        iy = ((gy + 1.0) * float(H) - 1.0) / 2.0
    ix = ix.clamp(-16.0, W + 16.0)
    iy = iy.clamp(-16.0, H + 16.0)
    fx, fy = torch.floor(ix), torch.floor(iy)
    x0, y0 = fx.long(), fy.long()
    ax1, ay1 = ix - fx, iy - fy
    ax0, ay0 = 1.0 - ax1, 1.0 - ay1
    vx0, vx1 = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
    vy0, vy1 = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
    z = torch.zeros_like(ix)
    w = [torch.where(vx0 & vy0, ay0 * ax0, z), torch.where(vx1 & vy0, ay0 * ax1, z),
         torch.where(vx0 & vy1, ay1 * ax0, z), torch.where(vx1 & vy1, ay1 * ax1, z)]
    msum = ((w[0] + w[1]) + w[2]) + w[3]
    mask = msum >= thr
    w = [torch.where(mask, t, z) for t in w]
    m64 = sum(t.double() for t in (torch.where(vx0 & vy0, ay0 * ax0, z), torch.where(vx1 & vy0, ay0 * ax1, z),
                                    torch.where(vx0 & vy1, ay1 * ax0, z), torch.where(vx1 & vy1, ay1 * ax1, z)))
    return x0, y0, w, m64, mask, (ax1, ay1, [vx0 & vy0, vx1 & vy0, vx0 & vy1, vx1 & vy1])


def warp_apply(x: torch.Tensor, taps) -> torch.Tensor:
    """float64 blend of x's four taps with the given (float32) weights"""
    x0, y0, w = taps[:3]
    B, C, H, W = x.shape
    flat = x.double().reshape(B, C, H * W)
    out = torch.zeros((B, C, H, W), dtype=torch.float64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        idx = ((y0 + dy).clamp(0, H - 1) * W + (x0 + dx).clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
        out += torch.gather(flat, 2, idx).reshape(B, C, H, W) * w[k].double().unsqueeze(1)
    return out


def near_threshold(taps, thr: float) -> torch.Tensor:
    return (taps[3] - thr).abs() < MASK_EPS


# ---- the spies ---------------------------------------------------------------------------------------------------------------------
class LaunchAudit:
    """Install with `install(monkeypatch, plan)`, run plan.run(x) (eager), then read `records` / `routes`.  Every record:
    {op, route, kernel (convolutions; else ""), shape, images, ratio (max error / bound over the checked elements), excluded, pixels}."""

    def __init__(self, seed: int = 0):
        self.records: List[Dict] = []
        self.seed = seed
        self.in_split96 = False
        self.plan = None

    @property
    def routes(self):
        return {r["route"] for r in self.records}

    @property
    def kernels(self):
        return {r["kernel"] for r in self.records if r["kernel"]}

    def worst_by_family(self) -> Dict[str, float]:
        out: Dict[str, float] = {}
        for r in self.records:
            fam = family(r["route"])
            out[fam] = max(out.get(fam, 0.0), r["ratio"])
        return out

    def failures(self):
        return [r for r in self.records if not (r["ratio"] <= 1.0)]

    # raw filter bank of a packed buffer (the plan keeps both)
    def _raw_weight(self, packed: torch.Tensor) -> torch.Tensor:
        p = self.plan
        for d in (p.packed, p.wino_packed, p.wino4_packed, p.pyr1_packed):
            for k, t in d.items():
                if t.data_ptr() == packed.data_ptr() and t.numel() == packed.numel():
                    base, sl = (k.split("[", 1) + [""])[:2]
                    w = p.p[base + ".weight"]
                    if sl == ":64]":
                        w = w[:64]
                    elif sl == "64:]":
                        w = w[64:]
                    return w.detach().float().cpu()
        raise KeyError("packed weights not held by the plan")

    def _record(self, op, route, shape, images, ratio, excluded=0, pixels=0, kernel=""):
        self.records.append(dict(op=op, route=route, kernel=kernel, shape=tuple(shape), images=images, ratio=float(ratio),
                                 excluded=int(excluded), pixels=int(pixels)))

    def install(self, monkeypatch, plan) -> None:
        from opticalflow_amd import engine, ops
        self.plan = plan
        real = {n: getattr(ops, n) for n in OPS}
        for n in OPS:
            monkeypatch.setattr(ops, n, self._spy(n, real[n]))
        real96 = engine.PwcPlan._conv_split96

        def split96(plan_self, *a, **kw):
            self.in_split96 = True
            try:
                return real96(plan_self, *a, **kw)
            finally:
                self.in_split96 = False
        monkeypatch.setattr(engine.PwcPlan, "_conv_split96", split96)

    def _spy(self, name, real):
        sig = inspect.signature(real)
        check = getattr(self, "_check_" + name)

        def f(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            return check(real, ba.arguments)
        return f

    # ---- per operator --------------------------------------------------------------------------------------------------------------
    def _check_densify(self, real, A):
        t = A["t"]
        before = t.cpu()
        out = real(**A)
        torch.cuda.synchronize()
        self._record("densify", "densify", t.shape, t.shape[0], 0.0 if torch.equal(out.cpu(), before) else float("inf"))
        return out

    def _conv_common(self, op, real, A, route, rel, stride=1, dilation=1, split2_out=False):
        x, bias = A["x"], A["bias"]
        wp = A.get("wpacked", A.get("upacked"))
        n = x.shape[0]
        imgs = pick_images(n, self.seed + len(self.records))
        xs = x[imgs].cpu()
        res = A.get("residual")
        rs = res[imgs].cpu() if res is not None else None
        w = self._raw_weight(wp)
        b = bias.detach().float().cpu()
        out = real(**A)
        kernel = last_kernel(used_split(op, A))
        torch.cuda.synchronize()
        if split2_out:
            got = torch.cat([out[4 * i:4 * i + 4] for i in imgs]).cpu()
        else:
            got = out[imgs].cpu()
        ref, s = conv_ref(xs, w, b, stride, dilation, A["leaky_slope"] is not None, rs)
        if split2_out:
            ref, s = split2(ref), split2(s)
        self._record(op, route, x.shape, len(imgs), worst(bounded_ratio(got, ref, s, rel))[0], kernel=kernel)
        return out

    def _check_conv3x3(self, real, A):
        from opticalflow_amd import ops
        x, cout = A["x"], A["cout"]
        n, cin, h, w = x.shape
        s, d = A["stride"], A["dilation"]
        need = ops.conv3x3_workspace_bytes(n, cin, h, w, cout, s, d)
        if s == 2:
            route = "conv/direct/s2"
        elif A["residual"] is not None:
            route = "conv/direct/residual"
        elif cout == 10:
            route = "head/head10"
        elif cout == 2:
            route = "head/conv"
        elif d > 1:
            route = "conv/direct/dilated"
        elif A["workspace"] is not None and 0 < need:
            route = "conv/direct/split-k"
        else:
            route = "conv/direct"
        rel = REL_HEAD if route.startswith("head") else REL_DIRECT
        return self._conv_common("conv3x3", real, A, route, rel, s, d)

    def _check_conv3x3_wino(self, real, A):
        from opticalflow_amd import ops
        x, cout, d = A["x"], A["cout"], A["dilation"]
        n, cin, h, w = x.shape
        need = ops.conv3x3_wino_workspace_bytes(n, cin, h, w, cout, d)
        if self.in_split96:
            route = "conv/split96/wino2"
        elif d > 1:
            route = "conv/wino2/dilated"
        elif A["workspace"] is not None and 0 < need:
            route = "conv/wino2/split-k"
        else:
            route = "conv/wino2"
        return self._conv_common("conv3x3_wino", real, A, route, REL_WINO2, 1, d)

    def _check_conv3x3_wino4(self, real, A):
        from opticalflow_amd import ops
        x, cout = A["x"], A["cout"]
        n, cin, h, w = x.shape
        need = ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, cout)
        if self.in_split96:
            route = "conv/split96/wino4"
        elif A["split2"]:
            route = "conv/wino4/split2"
        elif A["workspace"] is not None and 0 < need:
            route = "conv/wino4/cin-split"
        else:
            route = "conv/wino4"
        return self._conv_common("conv3x3_wino4", real, A, route, REL_WINO4, 1, 1, split2_out=A["split2"])

    def _check_pyr1_wino(self, real, A):
        return self._conv_common("pyr1_wino", real, A, "pyr1/wino2", REL_WINO2)

    def _check_pyr1_wino_pair(self, real, A):
        x = A["x"]
        imgs = pick_images(x.shape[0], self.seed + len(self.records))
        xs = x[imgs].cpu()
        w1, w2 = self._raw_weight(A["upacked1"]), self._raw_weight(A["upacked2"])
        b1, b2 = A["bias1"].detach().float().cpu(), A["bias2"].detach().float().cpu()
        out = real(**A)
        kernel = last_kernel()
        torch.cuda.synchronize()
        y1, s1 = conv_ref(xs, w1, b1)
        ref = F.leaky_relu(F.conv2d(y1, w2.double(), b2.double(), padding=1), LEAKY)
        s2 = F.conv2d(y1.abs(), w2.double().abs(), b2.double().abs(), padding=1)
        s = F.conv2d(s1, w2.double().abs(), None, padding=1) + s2
        self._record("pyr1_wino_pair", "pyr1/pair", x.shape, len(imgs), worst(bounded_ratio(out[imgs].cpu(), ref, s, REL_WINO2))[0],
                     kernel=kernel)
        return out

    def _check_head_upfeat(self, real, A):
        from opticalflow_amd import ops
        x = A["x"]
        n, cin, h, w = x.shape
        tiles = n * ((w + 127) // 128) * ((h + 7) // 8)
        sliced = tiles < 64 and A["workspace"] is not None and ops.head_upfeat_workspace_bytes(n, cin, h, w) > 0
        route = "head/upfeat-sliced" if sliced else "head/upfeat"
        imgs = pick_images(n, self.seed + len(self.records))
        xs = x[imgs].cpu()
        wf = self._raw_weight(A["head_wpacked"])
        bf, uw, ub = (A[k].detach().float().cpu() for k in ("head_bias", "up_weight", "up_bias"))
        real(**A)
        kernel = last_kernel()
        torch.cuda.synchronize()
        gf, gu = A["flow_out"][imgs].cpu(), A["up_out"][imgs].cpu()
        rf, sf = conv_ref(xs, wf, bf, act=False)
        ru, su = deconv_ref(xs, uw, ub)
        r = max(worst(bounded_ratio(gf, rf, sf, REL_HEAD))[0], worst(bounded_ratio(gu, ru, su, REL_HEAD))[0])
        self._record("head_upfeat", route, x.shape, len(imgs), r, kernel=kernel)

    def _check_upsample_entry(self, real, A):
        head = A["head"]
        n, _, h, w = head.shape
        imgs = pick_images(n, self.seed + len(self.records))
        hs = head[imgs].cpu()
        dw, db = A["deconv_w"].float().cpu(), A["deconv_b"].float().cpu()
        out = real(**A)
        torch.cuda.synchronize()
        got = A["out"][imgs].cpu()
        rf, sf = deconv_ref(hs[:, 0:2], dw, db)
        r = worst(bounded_ratio(got[:, 0:2], rf, sf, REL_DECONV))[0]
        # up_feat: the phases co*4 + py*2 + px of the 10-channel convolution, re-ordered -- exact
        up = hs[:, 2:10].reshape(len(imgs), 2, 2, 2, h, w).permute(0, 1, 4, 2, 5, 3).reshape(len(imgs), 2, 2 * h, 2 * w)
        if not torch.equal(got[:, 2:4], up):
            r = float("inf")
        self._record("upsample_entry", "head/upsample-entry", head.shape, len(imgs), r)
        return out

    def _check_deconv4x4s2(self, real, A):
        x = A["x"]
        imgs = pick_images(x.shape[0], self.seed + len(self.records))
        xs = x[imgs].cpu()
        w, b = A["weight"].float().cpu(), A["bias"].float().cpu()
        out = real(**A)
        torch.cuda.synchronize()
        ref, s = deconv_ref(xs, w, b)
        self._record("deconv4x4s2", "deconv", x.shape, len(imgs), worst(bounded_ratio(out[imgs].cpu(), ref, s, REL_DECONV))[0])
        return out

    def _check_lattice_unsplit(self, real, A):
        x, batch, levels = A["x"], A["batch"], A["levels"]
        xs = x.cpu()
        out = real(**A)
        torch.cuda.synchronize()
        ok = torch.equal(out.cpu(), unsplit(xs, levels))
        self._record("lattice_unsplit", "ctx/lattice-unsplit", x.shape, batch, 0.0 if ok else float("inf"))
        return out

    def _corr_route(self, n, c, h, w):
        from opticalflow_amd import _lib
        tiles = n * ((w + 31) // 32) * ((h + 7) // 8)
        if tiles <= _lib.get_option("corr_small_tiles"):
            return "entry/corr-small"
        if _lib.get_option("corr_pipe") and (c + 3) // 4 in (8, 16) and tiles >= _lib.get_option("corr_pipe_min_tiles") and w % 4 == 0:
            return "entry/corr-pipe"
        return "entry/corr" if w % 4 == 0 else "entry/corr-generic"

    def _check_correlation(self, real, A):
        in1, in2 = A["in1"], A["in2"]
        n, c, h, w = in1.shape
        imgs = pick_images(n, self.seed + len(self.records))
        a, b = in1[imgs].cpu(), in2[imgs].cpu()
        out = real(**A)
        torch.cuda.synchronize()
        assert (A["pad_size"], A["kernel_size"], A["max_displacement"], A["stride1"], A["stride2"], A["corr_multiply"]) == (4, 1, 4, 1, 1, 1.0)
        ref, s = corr_ref(a, b, A["normalize"], A["leaky_slope"] is not None)
        # the plan correlates plain features only at level 6; below, the operand is the warp launch just recorded
        after_warp = bool(self.records) and self.records[-1]["op"] == "warp"
        route = self._corr_route(n, c, h, w) if after_warp else "entry/corr-level6"
        self._record("correlation", route, in1.shape, len(imgs), worst(bounded_ratio(out[imgs].cpu(), ref, s, REL_CORR))[0])
        return out

    def _check_warp(self, real, A):
        x, flo = A["x"], A["flo"]
        n, c, h, w = x.shape
        imgs = pick_images(n, self.seed + len(self.records))
        xs, fs = x[imgs].cpu(), flo[imgs].cpu()
        out = real(**A)
        torch.cuda.synchronize()
        taps = warp_taps(fs, A["flow_scale"], A["align_corners"], A["mask_threshold"])
        ref = warp_apply(xs, taps)
        s = warp_apply(xs.abs(), taps)
        near = near_threshold(taps, A["mask_threshold"])
        keep = (~near).unsqueeze(1)
        self._record("warp", "entry/warp", x.shape, len(imgs), worst(bounded_ratio(out[imgs].cpu(), ref, s, REL_WARP, keep))[0],
                     int(near.sum()), near.numel())
        return out

    def _check_warp_correlation(self, real, A):
        from opticalflow_amd import _lib
        in1, x2, flo = A["in1"], A["x2"], A["flo"]
        n, c, h, w = in1.shape
        imgs = pick_images(n, self.seed + len(self.records))
        a, b, fs = in1[imgs].cpu(), x2[imgs].cpu(), flo[imgs].cpu()
        out = real(**A)
        if out is None:
            return None
        torch.cuda.synchronize()
        mode = _lib.get_option("warpcorr_window")
        nch = (c + 3) // 4
        route = "entry/fused-window" if (mode > 0 and (nch == 8 or (nch == 16 and mode >= 2))) else "entry/fused-r2"
        taps = warp_taps(fs, A["flow_scale"], A["align_corners"], A["mask_threshold"])
        w2, w2a = warp_apply(b, taps), warp_apply(b.abs(), taps)
        ref, _ = corr_ref(a, w2, A["normalize"], A["leaky_slope"] is not None)
        _, s = corr_ref(a.abs(), w2a, A["normalize"], False)
        near = near_threshold(taps, A["mask_threshold"])
        # a pixel near the threshold enters the cost volume of its 81 neighbours through w2: drop those outputs too
        bad = F.max_pool2d(near.double().unsqueeze(1), 9, 1, 4)[:, 0] > 0
        keep = (~bad).unsqueeze(1)
        self._record("warp_correlation", route, in1.shape, len(imgs),
                     worst(bounded_ratio(out[imgs].cpu(), ref, s, REL_CORR, keep))[0], int(near.sum()), near.numel())
        return out


def family(route: str) -> str:
    parts = route.split("/")
    return "/".join(parts[:2]) if parts[0] == "conv" else parts[0]
