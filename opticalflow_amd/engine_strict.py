"""Strict half-precision plan of PWCDCNet.forward: ``PWCDCNet(precision="fp16-strict")``.

north_star asks for flow within 1e-3 mean EPE of the reference (models/PWCNet.py:180-273 on the CPU).  The fast half plan
(engine_f16.PwcPlanF16) sits at ~1.2e-3 of mean |flow| and cannot do better with 11-bit storage everywhere: its error is the sum
of ~25 rounded tensors per level, and -- worse -- every perturbation of the flows UPSTREAM of a warp can flip warp-mask decisions
at the 0.9999 threshold (PWCNet.py:174), which makes the error heavy-tailed (single events of 3e-3 in the CPU emulation,
tests/f16_error_budget.py ``policies``).  This plan removes both effects where they are cheap and keeps half precision where the
flops are:

  * feature pyramid, decoder levels 6..3 and the level-2 ENTRY (warp + cost volume) run on the fp32 plan (engine.PwcPlan with
    ``trunk2=False``: Winograd / direct MFMA fp32 kernels, 21 % of the network's multiplications).  Every warp therefore sees
    the same flow as the fp32 path: no discrete event is ever re-rolled, the remaining error is smooth;
  * the level-2 dense block, its flow head and the context network -- 79 % of the multiplications -- run in half precision on the
    c8 kernels, the layers with the largest share of the error budget with SPLIT FILTERS (hi + lo halves of every filter,
    ops_f16.pack_conv3x3_f16(split=True): ~22-bit filters, twice the MFMA passes, fp32 accumulation; PLAIN_FILTERS below names the
    layers that do without), fp32 flow head and fp32 ``flow2 = predict_flow2 + dc_conv7`` as in the fast plan.  What
    remains is the rounding of the activations those layers store (conv2_*, dc_conv*);
  * the level-2 BASE channels [corr 81 | c1 32 | up_flow 2 | up_feat 2] -- computed in fp32, read by all seven level-2 consumers
    -- are handed over with the rounding residual of corr and of the four flow channels stored as second channel sets
    (pwc_nchw_to_c8_f16_hilo) whose filters are copies of the first sets', so those 85 inputs carry ~22 bits (+96 input channels
    per consumer).  c1's residual is not carried: its rounding contributes 0.02e-4 of the EPE against 0.9e-4 (corr) and 1.2e-4
    (up_flow / up_feat) in the what-if emulation.

CPU emulation (tests/f16_error_budget.py): policy ``fffffss`` (pyr/dec6..3 fp32, dec2/ctx split) gives 0.35e-3 / 0.60e-3 /
0.85e-3 / 0.85e-3 on the 64x64, 128x192, 448x1024 and KITTI-sized random inputs (fast plan: 0.61 / 1.09 / 1.59 / 1.81); measured
on the GPU 0.33 / 0.57 / 0.83e-3 -- and 1.03e-3 on the smooth KITTI-like pair of the tests (mean |flow| 1.63), hence the hi + lo
base channels (``whatif``: 0.85 -> 0.65e-3 at 448x1024; the rest is conv2_* 0.52, dc_conv* 0.39, adding in quadrature).

No autograd; ``flows()`` gives the training-mode 5-tuple (flow3..flow6 straight from the fp32 plan).

``PwcVideoPlanStrict`` is the same mode for video.FlowStream: the fp32 part is engine.PwcVideoPlan (one pyramid pass per frame), the
half-precision level 2 is this plan's ``_level2``.
"""
from __future__ import annotations

import os
from typing import Dict

import torch

from . import ops
from . import ops_f16 as F16
from .engine import CONTEXT, DENSE_OUT, LEAKY, PYRAMID_CH, PwcPlan, PwcVideoPlan
from .engine_f16 import BASE_G, CORR_G, DENSE_G, _groups, context_filters, level_filters, prepare_params


# Layers of the level-2 block / context network that may run with PLAIN half filters (one MFMA pass instead of two).  Measured ladder
# (batch 16 x 448x1024; EPE on the 1x448x1024 golden / the smooth KITTI-sized pair of the tests, the worst input they hold):
#   every layer split                          (default)   1739 pairs/s   6.5e-4 / 8.0e-4
#   dc_conv4..6 plain                                      1783           6.8e-4 / 8.5e-4
#   dc_conv4..6, conv2_3, conv2_4 plain  ("fast" ladder)   1857           7.1e-4 / 8.7e-4
#   fast + conv2_2 / + conv2_1 / + conv2_0 / + dc_conv1    1915 / 1923 / 1901 / 1982     7.4-7.6e-4 / 9.1 / 9.1 / 9.5 / 9.3e-4
#   fast + dc_conv2, dc_conv3                              1897           8.0e-4 / 9.9e-4   (no margin left under 1e-3)
# in line with the CPU what-if emulation (tests/f16_error_budget.py kitti whatif shipped: +0.25e-4 for conv2_3/2_4, +0.37e-4 for
# dc_conv4..6, +1.1e-4 for dc_conv2..6).  The error of this mode is RELATIVE (0.5-0.6e-3 x mean |flow2|, tests/test_gpu_f16.py:
# test_forward_fp16_strict_larger_motion), so the absolute 1e-3 of north_star holds while mean |flow2| <~ 1.8 with every layer split and
# ~1.5 on the fast ladder.  Round 3 shipped the fast ladder with 13 % margin on the worst held input; since round 4 the DEFAULT keeps every
# layer split (20 % margin there) and the ladder is opt-in: PWC_STRICT_PLAIN=fast, or a comma-separated list of layer names.
SPLITTABLE = ("conv2_0", "conv2_1", "conv2_2", "conv2_3", "conv2_4", "dc_conv1", "dc_conv2", "dc_conv3", "dc_conv4", "dc_conv5", "dc_conv6")
FAST_LADDER = "dc_conv4,dc_conv5,dc_conv6,conv2_3,conv2_4"


def parse_plain_filters(spec: str) -> frozenset:
    """PWC_STRICT_PLAIN: "" / "none" = every layer split (default), "fast" = the measured ladder step above, else layer names."""
    spec = (spec or "").strip()
    if spec in ("", "none"):
        return frozenset()
    if spec == "fast":
        spec = FAST_LADDER
    names = [n.strip() for n in spec.split(",") if n.strip()]
    unknown = [n for n in names if n not in SPLITTABLE]
    if unknown:
        raise ValueError("PWC_STRICT_PLAIN: unknown layer name(s) %s (known: %s, or 'fast' / 'none')" % (unknown, ", ".join(SPLITTABLE)))
    return frozenset(names)


PLAIN_FILTERS = parse_plain_filters(os.environ.get("PWC_STRICT_PLAIN", ""))


class PwcPlanStrict:
    UPPER = PwcPlan                                                 # the fp32 upper part's plan class (PwcVideoPlanStrict: the stream's)

    def __init__(self, params: Dict[str, torch.Tensor], B: int, H: int, W: int, device: torch.device, md: int = 4,
                 normalize_corr: bool = False, align_corners: bool = False, variant: str = "dc"):
        if md != 4:
            raise NotImplementedError("the half-precision arena is laid out for md=4 (81 cost-volume channels)")
        # fp32 part: pyramid, levels 6..3, level-2 entry
        self.upper = self.UPPER(params, B, H, W, device, torch.float32, md, normalize_corr, align_corners, "hip", variant, trunk2=False)
        self.B, self.H, self.W, self.device = B, H, W, device
        self.nd = 81
        h2, w2 = H >> 2, W >> 2
        self.size2 = (h2, w2)
        g2 = _groups(PYRAMID_CH[2])
        self.f0 = BASE_G + CORR_G                                   # first group of c1 inside the c8 arena
        self.nbase = CORR_G + g2 + 1                                # groups of [corr | c1 | flow]
        # the residual (lo) set follows: [corr residual | flow residual].  c1 gets none: the what-if emulation (tests/f16_error_budget.py
        # kitti whatif, profiles/r03_f16_strict_budget.txt) attributes 0.9e-4 of the EPE to the rounding of corr, 1.2e-4 to the four
        # up_flow / up_feat channels and 0.02e-4 to the 32 channels of c1
        self.r_corr = BASE_G + self.nbase                           # first residual group of corr
        self.r_flow = self.r_corr + CORR_G                          # residual group of [up_flow | up_feat]
        hk = dict(device=device, dtype=torch.float16)
        self.arena = torch.zeros((B, self.r_flow + 1, h2, w2, 8), **hk)
        self.ctx = [torch.zeros((B, _groups(c), h2, w2, 8), **hk) for c, _ in CONTEXT]
        self.head = torch.zeros((B, 1, h2, w2, 8), device=device, dtype=torch.float32)
        self.dc7 = torch.zeros((B, 1, h2, w2, 8), device=device, dtype=torch.float32)
        self.flow_out = torch.empty((B, 2, h2, w2), device=device, dtype=torch.float32)

        self.split: Dict[str, bool] = {}
        self.w: Dict[str, torch.Tensor] = {}
        self.b: Dict[str, torch.Tensor] = {}
        self.cin: Dict[str, int] = {}
        self.cout: Dict[str, int] = {}
        p = prepare_params(params, variant, self.nd)
        nphys = int(self.arena.shape[1]) * 8
        corr0, flow0 = BASE_G * 8, (self.f0 + g2) * 8                 # physical channels of corr (88 with its pad) and of the flow group
        rc0, rf0 = self.r_corr * 8, self.r_flow * 8
        for name, w, bias, _ in list(level_filters(p, 2, nphys, self.nd)) + list(context_filters(p)):
            if not name.startswith("dc_conv") or name == "dc_conv1":
                # consumers of the level-2 arena: column j of w is physical channel (nphys - w.shape[1]) + j; the residual channel
                # sets get the filters of the sets they correct
                ps = nphys - w.shape[1]
                w = w.clone()
                w[:, rc0 - ps:rc0 + CORR_G * 8 - ps] = w[:, corr0 - ps:corr0 + CORR_G * 8 - ps]
                w[:, rf0 - ps:rf0 + 8 - ps] = w[:, flow0 - ps:flow0 + 8 - ps]
            # hi + lo filters, except on the layers PLAIN_FILTERS names (their what-if cost in EPE is recorded in the module docstring);
            # the two flow heads (Cout 2: the residuals ride in the idle half of the cout tile) always keep them
            self.split[name] = name in ("head2", "dc_conv7") or name not in PLAIN_FILTERS
            self.w[name] = F16.pack_conv3x3_f16(w.contiguous().float(), split=self.split[name])
            self.b[name] = bias.contiguous().float()
            self.cin[name], self.cout[name] = w.shape[1], w.shape[0]

    def _conv(self, name, x, out, dilation=1, act=True):
        F16.conv3x3_f16(x, self.w[name], self.b[name], self.cin[name], self.cout[name], dilation=dilation,
                        leaky_slope=LEAKY if act else None, out=out, out_f32=out.dtype == torch.float32, split_w=self.split[name])

    def run(self, x: torch.Tensor) -> torch.Tensor:
        up, B = self.upper, self.B
        if tuple(x.shape) != (B, 6, self.H, self.W) or x.dtype != torch.float32 or x.device != self.device:
            raise ValueError("plan built for float32 %s on %s, got %s %s on %s" % (
                (B, 6, self.H, self.W), self.device, x.dtype, tuple(x.shape), x.device))
        x = ops.densify(x)
        up.conv_macs = {"direct": 0, "executed": 0}
        up._pyramid([(x[:, :3], 0, B), (x[:, 3:], B, 2 * B)], 0, 2 * B)
        # levels 6..3 (level 3's heads write up_flow / up_feat into the fp32 level-2 base channels) and the level-2 entry:
        # c1 | fused warp + correlation + LeakyReLU, all fp32
        up._decode()
        return self._level2()

    def _level2(self) -> torch.Tensor:
        """The half-precision part, from the upper plan's level-2 base channels to flow2 (PwcVideoPlanStrict.push ends with it too)."""
        up = self.upper
        # hand-over: fp32 NCHW [corr 81 | c1 32 | up_flow 2 | up_feat 2] -> the c8 half arena's corr / c1 / flow groups + residuals
        base = up.arena[2]
        c = PYRAMID_CH[2]
        g2 = _groups(c)
        ar = self.arena
        F16.to_c8_hilo(base[:, 0:81], ar[:, BASE_G:BASE_G + CORR_G], ar[:, self.r_corr:self.r_corr + CORR_G])
        F16.to_c8(base[:, 81:81 + c], out=ar[:, self.f0:self.f0 + g2])
        F16.to_c8_hilo(base[:, 81 + c:81 + c + 4], ar[:, self.f0 + g2:self.f0 + g2 + 1], ar[:, self.r_flow:self.r_flow + 1])
        # level-2 dense block, flow head, context network: half activations, split filters, fp32 accumulation
        lo = BASE_G
        for i, og in enumerate(DENSE_G):
            self._conv("conv2_%d" % i, ar[:, lo:], ar[:, og:og + DENSE_OUT[i] // 8])
            lo = og
        self._conv("head2", ar, self.head, act=False)
        t = ar
        for i, (_, dil) in enumerate(CONTEXT):
            self._conv("dc_conv%d" % (i + 1), t, self.ctx[i], dilation=dil)
            t = self.ctx[i]
        self._conv("dc_conv7", t, self.dc7, act=False)
        torch.add(self.head[:, 0, :, :, 0:2].permute(0, 3, 1, 2), self.dc7[:, 0, :, :, 0:2].permute(0, 3, 1, 2), out=self.flow_out)
        return self.flow_out

    def flows(self):
        """(flow2, flow3, flow4, flow5, flow6) of the last run -- the training-mode return (PWCNet.py:270-271)."""
        f = self.upper.flow
        return (self.flow_out, f[3], f[4], f[5], f[6])


class PwcVideoPlanStrict(PwcPlanStrict):
    """The strict mode for consecutive frames (video.FlowStream with precision="fp16-strict"): the fp32 upper part is
    engine.PwcVideoPlan(trunk2=False) -- B + 1 pyramid slots, slot 0 carrying the previous push's last frame, one pyramid pass per frame,
    stopping after the level-2 entry -- and the half-precision level 2 is PwcPlanStrict's, the same statement.  Against the pairwise
    strict forward only the pyramid's batch size differs (B instead of 2B images), as between PwcVideoPlan and PwcPlan."""
    UPPER = PwcVideoPlan

    @property
    def primed(self) -> bool:
        return self.upper.primed

    @property
    def pyr_a(self):
        """the upper plan's pyramid buffers: pyr_a[l][0] is the carry slot a graph capture saves and restores"""
        return self.upper.pyr_a

    def prime(self, frame: torch.Tensor) -> None:
        self.upper.prime(frame)

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        # pyramid of the B new frames, levels 6..3, level-2 entry; then the half part, and only then the carry
        return self.upper.push(frames, tail=self._level2)

    def run(self, x):
        raise RuntimeError("PwcVideoPlanStrict is driven by prime()/push(), not run()")
