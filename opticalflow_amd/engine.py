"""Execution plan of PWCDCNet.forward on one MI355X: buffers, packed weights, launch order.

What the reference does per forward (models/PWCNet.py:180-273) and what the plan does instead:

  * ``torch.cat((conv(x), x), 1)`` five times per level (PWCNet.py:202-264, 747 MB of copies per
    1024x448 pair): the plan allocates ONE arena ``[B, Ctot, H, W]`` per level whose channel order
    is the final concatenation order
        [conv_4 | conv_3 | conv_2 | conv_1 | conv_0 | corr | c1 | up_flow | up_feat]
    and every producer (dense convs, correlation, the two deconvs) writes its channel slice in
    place (the first image's pyramid features are COPIED into their slot, 46 us per forward at
    batch 16: the pyramid runs both images as one 2B batch with one output stride); a consumer reads a channel *suffix* -- only the batch stride differs
    from a dense tensor, which the C ABI takes as an argument.
  * warp: one fused kernel instead of mesh + 2x grid_sample + mask ops (PWCNet.py:141-177), with the
    per-level flow scale (PWCNet.py:212,226,240,256) folded in.
  * correlation + LeakyReLU (PWCNet.py:198-199): one kernel writing straight into the arena.
  * both images go through the feature pyramid as one 2B batch (PWCNet.py:184-195 runs it twice).

All launches go to the current torch stream; nothing allocates after construction, so a plan can be
captured into a HIP graph (``PWCDCNet.forward(..., )`` does that when ``use_graph`` is set).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib, ops

PYRAMID_CH = (3, 16, 32, 64, 96, 128, 196)
PYRAMID_NAMES = (("conv1a", "conv1aa", "conv1b"), ("conv2a", "conv2aa", "conv2b"), ("conv3a", "conv3aa", "conv3b"),
                 ("conv4a", "conv4aa", "conv4b"), ("conv5a", "conv5aa", "conv5b"), ("conv6aa", "conv6a", "conv6b"))
PYRAMID_NAMES_OLD = (("conv1a", None, "conv1b"), ("conv2a", None, "conv2b"), ("conv3a", None, "conv3b"),
                     ("conv4a", None, "conv4b"), ("conv5a", None, "conv5b"), ("conv6a", None, "conv6b"))   # PWCNet.py:290-301
DENSE_OUT = (128, 128, 96, 64, 32)            # conv{L}_0 .. conv{L}_4 (PWCNet.py:78-82)
DENSE_TOTAL = sum(DENSE_OUT)                  # 448
# channel offset of conv{L}_i's output inside the arena; conv{L}_i reads everything after it
DENSE_OFF = (320, 192, 96, 32, 0)
CONTEXT = ((128, 1), (128, 2), (128, 4), (96, 8), (64, 16), (32, 1))   # dc_conv1..6 (PWCNet.py:126-131)
WARP_SCALE = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}                      # PWCNet.py:212,226,240,256
LEAKY = 0.1


def old_variant_perm(k: int, od: int) -> torch.Tensor:
    """Input-channel permutation for PWCDCNet_old (PWCNet.py:425-429): its dense block concatenates in the order
    [conv_1 | base | conv_0 | conv_2 | conv_3 | conv_4] while the arena is [conv_4 | conv_3 | conv_2 | conv_1 | conv_0 | base].
    Returns `perm` with arena_input_channel j == reference_input_channel perm[j] for the consumer that reads the
    outputs of conv_0..conv_{k-1} (k = 5: flow head / upfeat / dc_conv1).  A convolution over a concatenation does
    not care about the order as long as the filter's input channels follow it."""
    sizes = {"base": od}
    for i, c in enumerate(DENSE_OUT):
        sizes["c%d" % i] = c
    logical = [n for n in ("c1", "base", "c0", "c2", "c3", "c4") if n == "base" or int(n[1]) < k]
    physical = ["c%d" % i for i in range(k - 1, -1, -1)] + ["base"]
    start, pos = {}, 0
    for n in logical:
        start[n] = pos
        pos += sizes[n]
    return torch.cat([torch.arange(start[n], start[n] + sizes[n]) for n in physical])


def reorder_old_variant(p: Dict[str, torch.Tensor], nd: int = 81) -> None:
    """PWCDCNet_old's filters in `p`: input channels from the reference's concatenation order to the arena's (old_variant_perm)"""
    for l in range(2, 7):
        od = level_in_channels(l, nd)
        names = [("conv%d_%d.0.weight" % (l, k), k, 1) for k in range(1, 5)] + [("predict_flow%d.weight" % l, 5, 1)]
        names.append(("upfeat%d.weight" % l, 5, 0) if l > 2 else ("dc_conv1.0.weight", 5, 1))
        for key, k, dim in names:
            p[key] = p[key].index_select(dim, old_variant_perm(k, od).to(p[key].device)).contiguous()


# multiplications a route executes per multiplication of the direct form, as (numerator, denominator)
ROUTE_MACS = {"pyr1": (16, 36), "pyr1x2": (16, 36), "wino4": (36, 144), "wino2": (16, 36), "direct": (1, 1), "torch": (1, 1)}


def level_in_channels(level: int, nd: int = 81) -> int:
    """`od` of PWCNet.py:77,87,97,107,117."""
    return nd if level == 6 else nd + PYRAMID_CH[level] + 4


class PwcPlan:
    def __init__(self, params: Dict[str, torch.Tensor], B: int, H: int, W: int, device: torch.device,
                 dtype: torch.dtype = torch.float32, md: int = 4, normalize_corr: bool = False,
                 align_corners: bool = False, conv_backend: str = "hip", variant: str = "dc", trunk2: bool = True):
        """trunk2=False (engine_strict.PwcPlanStrict): this plan stops after the level-2 ENTRY (correlation, c1, up_flow, up_feat);
        the level-2 dense block, flow head and context network belong to the caller, so their buffers and packed filters are not
        allocated and the level-2 arena holds only its 117 base channels."""
        if variant not in ("dc", "old"):
            raise ValueError("variant must be 'dc' (PWCDCNet) or 'old' (PWCDCNet_old)")
        if H % 64 or W % 64 or H <= 0 or W <= 0:
            raise ValueError("PWCDCNet needs H and W to be positive multiples of 64 (got %dx%d); resize or pad the "
                             "pair first like script_pwc.py:47-54 / inference_kitti.py:53-63" % (H, W))
        self.trunk2 = trunk2
        if conv_backend not in ("hip", "torch"):
            raise ValueError("conv_backend must be 'hip' or 'torch'")
        if dtype != torch.float32:
            raise NotImplementedError("plan dtype %s: only float32 is wired up" % dtype)
        self.B, self.H, self.W = B, H, W
        self.device, self.dtype = device, dtype
        self.md = md
        self.nd = (2 * md + 1) ** 2
        self.normalize_corr = normalize_corr
        self.align_corners = align_corners
        self.conv_backend = conv_backend
        self.variant = variant
        self.fuse_warp = os.environ.get("PWC_FUSE_WARP_CORR", "1") != "0"     # 0: warp and correlation as two launches (A/B runs)
        self.pyramid_names = PYRAMID_NAMES if variant == "dc" else PYRAMID_NAMES_OLD
        self.mask_threshold = 0.9999 if variant == "dc" else 0.999        # PWCNet.py:174 / :400
        self.p = dict(params)
        if variant == "old":
            reorder_old_variant(self.p, self.nd)
        kw = dict(device=device, dtype=dtype)
        # The switches every convolution's route depends on, read ONCE: a plan fixes its routes when it is built (_route), as a
        # captured graph does.  conv_wino4 = 0 (environment, or pwc_set_option("conv_wino4", 0) before the plan is built): large
        # layers stay on F(2x2,3x3) (A/B runs, error budget); pyr1_wino = 0 keeps the 16 -> 16 layers on the direct MFMA kernel
        hip = conv_backend == "hip"
        self.wino = os.environ.get("PWC_CONV_WINO", "1") != "0"
        self.wino4 = os.environ.get("PWC_CONV_WINO4", "1") != "0" and (not hip or _lib.get_option("conv_wino4") != 0)
        self.pyr1_wino = bool(hip and self.wino and _lib.get_option("pyr1_wino") > 0)

        self.size = {l: (H >> l, W >> l) for l in range(1, 7)}
        # pyramid scratch: per level two ping-pong buffers for the 2B batch, plus c2 (second image)
        self.pyr_a, self.pyr_b, self.c1, self.c2 = {}, {}, {}, {}
        for l in range(1, 7):
            h, w = self.size[l]
            c = PYRAMID_CH[l]
            self.pyr_a[l] = torch.empty((self._level_slots(B, l), c, h, w), **kw)      # levels 2-5: replaced by a view of the arena below
            self.pyr_b[l] = torch.empty((self._level_slots(B, l), c, h, w), **kw)
        self.warped = {l: torch.empty((B, PYRAMID_CH[l], *self.size[l]), **kw) for l in range(2, 6)}
        self.arena = {}
        self.arena_base = {}                    # first channel after the dense-block outputs
        # Levels 2-5: the first image's level features are part of the dense block's input (PWCNet.py:215), i.e. they
        # have a slot in the level's arena.  Instead of copying them there, the level's pyramid buffer IS that slot: the arena is
        # allocated for 2B items, items [0,B) are the decoder's arena, items [B,2B) only ever hold the second image's features in the
        # same channel slot, and pyr_a[l] is the [2B, c, h, w] view of that slot at the arena's batch stride -- every kernel takes batch
        # strides, so the pyramid's last convolution writes c1 where the decoder reads it (four copies, 47 us at batch 16, gone; the
        # cost is address space: 2.1 GB instead of 1.0 GB at level 2 / batch 16).  Not for the video plan (its c1 / c2 overlap).
        self.c1_in_arena = bool(conv_backend == "hip" and self._slots(B) == 2 * B and _lib.get_option("c1_in_arena"))
        for l in range(2, 7):
            od = level_in_channels(l, self.nd)
            self.arena_base[l] = DENSE_TOTAL if (l > 2 or trunk2) else 0
            if self.c1_in_arena and l < 6:
                pair = torch.empty((2 * B, self.arena_base[l] + od, *self.size[l]), **kw)
                self.arena[l] = pair[:B]
                off = self.arena_base[l] + self.nd
                self.pyr_a[l] = pair[:, off:off + PYRAMID_CH[l]]
            else:
                self.arena[l] = torch.empty((B, self.arena_base[l] + od, *self.size[l]), **kw)
        for l in range(2, 7):
            self.c1[l], self.c2[l] = self._pair_views(self.pyr_a[l], B)
        self.flow = {l: torch.empty((B, 2, *self.size[l]), **kw) for l in range(2 if trunk2 else 3, 7)}
        # Levels too small for the streaming head + upfeat kernel (W < 64: levels 6-5; all of 6-3 for a single pair): predict_flowL and
        # upfeatL run as ONE 3x3 convolution with 10 output channels on the matrix cores (ConvTranspose2d(k4,s2,p1) = a 3x3 convolution
        # with four output phases per channel) and ops.upsample_entry finishes the level -- the VALU deconvolution kernel took 21-26 us
        # per launch there.  flow[l] is then channels 0,1 of that convolution's output.
        self.head10: Dict[int, torch.Tensor] = {}
        # predict_flowL + upfeatL as one streaming pass: where its one-pass kernel runs (64 tiles) and, on Cin slices through the plan's
        # workspace, down to "head_sliced_min_tiles" tiles (level 3 of 2..8 pairs: 20-36 us ahead of the 10-channel convolution).  Below
        # the one-pass kernel's 64 tiles the library's own slice plan decides (a workspace demand > 0 <=> it cuts the launch along Cin):
        # with a small "stream_slice_wgs" it may not, and pwc_head_upfeat_ws_fwd would then refuse the launch
        self.stream_head = {l: conv_backend == "hip" and (
            ops.head_upfeat_supported(B, *self.size[l]) or (
                ops.head_upfeat_supported(B, *self.size[l], min_tiles=_lib.get_option("head_sliced_min_tiles"))
                and ops.head_upfeat_workspace_bytes(B, level_in_channels(l, self.nd) + DENSE_TOTAL, *self.size[l]) > 0))
            for l in range(3, 7)}
        if conv_backend == "hip" and _lib.get_option("head10"):
            for l in range(3, 7):
                if not self.stream_head[l]:
                    self.head10[l] = torch.empty((B, 10, *self.size[l]), **kw)
                    self.flow[l] = self.head10[l][:, 0:2]
        h2, w2 = self.size[2]
        self.flow_out = torch.empty((B, 2, h2, w2), **kw) if trunk2 else None
        self.ctx = [torch.empty((B, c, h2, w2), **kw) for c, _ in CONTEXT] if trunk2 else []
        # Context network in LATTICE-MAJOR layout (round 3): dc_conv1..3 store their result as its four pixel lattices (PWC_CONV_SPLIT2),
        # so the next layer -- dilation 2, 4, 8 in the reference (PWCNet.py:126-131) -- is a dilation-1 convolution on 4x as many
        # images of half the size, with contiguous rows: F(4x4) / F(2x2) at their dilation-1 speed instead of strided lattice
        # addressing (dc_conv2 611 -> ~430 us, dc_conv3 679 -> ~470 us at batch 16).  dc_conv5 (dilation 16) is a dilation-2
        # convolution on the dilation-8 lattices; its 64-channel result is brought back to NCHW by pwc_lattice_unsplit_f32.
        # One level deeper (ctx_lattice4): dc_conv4 runs all 96 couts on F(4x4) and stores ITS result as lattices too, so dc_conv5 is a
        # dilation-1 F(4x4) layer on 256B images of h/16 x w/16 (7x16 at 448x1024) -- both on the stacked tile groups of
        # pwc_conv_wino4.hip (several short images per workgroup), where the rule takes them; option "w4_stacked" = 0 restores the 3-level form.
        self.ctx_lattice = bool(
            trunk2 and hip and self.wino and self.wino4 and os.environ.get("PWC_CTX_LATTICE", "1") != "0"
            and h2 % 8 == 0 and w2 % 32 == 0
            and ops.conv3x3_wino4_preferred(B, level_in_channels(2, self.nd) + DENSE_TOTAL, h2, w2, CONTEXT[0][0])
            and ops.conv3x3_wino4_preferred(4 * B, CONTEXT[0][0], h2 // 2, w2 // 2, CONTEXT[1][0])
            and ops.conv3x3_wino4_preferred(16 * B, CONTEXT[1][0], h2 // 4, w2 // 4, CONTEXT[2][0]))
        self.ctx_lattice4 = self.dc4_split = False
        self.ctx4_lat: Optional[torch.Tensor] = None
        if self.ctx_lattice:
            self.ctx[0] = torch.empty((4 * B, CONTEXT[0][0], h2 // 2, w2 // 2), **kw)
            self.ctx[1] = torch.empty((16 * B, CONTEXT[1][0], h2 // 4, w2 // 4), **kw)
            self.ctx[2] = torch.empty((64 * B, CONTEXT[2][0], h2 // 8, w2 // 8), **kw)
            w4 = self.p["dc_conv4.0.weight"]
            self.ctx_lattice4 = bool(
                h2 % 16 == 0 and w2 % 64 == 0
                and tuple(w4.shape[:2]) == (CONTEXT[3][0], CONTEXT[2][0])
                and tuple(self.p["dc_conv5.0.weight"].shape[:2]) == (CONTEXT[4][0], CONTEXT[3][0])
                and ops.conv3x3_wino4_preferred(64 * B, CONTEXT[2][0], h2 // 8, w2 // 8, CONTEXT[3][0])
                and ops.conv3x3_wino4_preferred(256 * B, CONTEXT[3][0], h2 // 16, w2 // 16, CONTEXT[4][0]))
            # dc_conv4 (128 -> 96 on 64B images of h/8 x w/8, e.g. 14x32): its first 64 couts fill F(4x4)'s 32-column tile
            # groups, a 32-cout F(4x4) launch (32-row workgroups) would be half empty -> those couts stay on F(2x2).  A decision of
            # its own, not _split96_wanted: it asks neither for F(4x4)'s no to all 96 couts nor for F(2x2)'s yes to the last 32
            self.dc4_split = bool(not self.ctx_lattice4 and w4.shape[0] == 96
                                  and ops.conv3x3_wino4_preferred(64 * B, w4.shape[1], h2 // 8, w2 // 8, 64))
            n4, s4 = (256 * B, 16) if self.ctx_lattice4 else (64 * B, 8)      # images / size divisor of dc_conv4's output and dc_conv5
            self.ctx[3] = torch.empty((n4, CONTEXT[3][0], h2 // s4, w2 // s4), **kw)
            self.ctx4_lat = torch.empty((n4, CONTEXT[4][0], h2 // s4, w2 // s4), **kw)
        for l in self.head10:
            w10 = torch.cat((self.p["predict_flow%d.weight" % l], ops.deconv_as_conv3x3(self.p["upfeat%d.weight" % l])), 0)
            self.p["head10_%d.weight" % l] = w10.contiguous()
            self.p["head10_%d.bias" % l] = torch.cat((self.p["predict_flow%d.bias" % l],
                                                       self.p["upfeat%d.bias" % l].repeat_interleave(4))).contiguous()

        # Filter banks in each kernel family's own order, packed by _route for the launches that take that family: direct MFMA,
        # G g Gt of F(2x2,3x3), of F(4x4,3x3) (4x the filter bytes), and of the 16-channel F(2x2) kernel (pwc_pyr1_wino.hip, 16 KB each)
        self.packed: Dict[str, torch.Tensor] = {}
        self.wino_packed: Dict[str, torch.Tensor] = {}
        self.wino4_packed: Dict[str, torch.Tensor] = {}
        self.pyr1_packed: Dict[str, torch.Tensor] = {}
        self.split96_bias: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}
        self.routes: Dict[tuple, str] = {}                     # (layer, geometry, ...) -> route, see _route
        self.conv_macs = {"direct": 0, "executed": 0}
        # ONE scratch shared by every convolution of the plan (they run back to back on one stream): split-K of the direct and
        # F(2x2) kernels, tail / whole-launch split of F(4x4), Cin slices of the streaming head.  pwc_conv3x3_wino*_preferred count
        # those splits, so the buffer has to cover EVERY launch the plan makes (a hand-written list of geometries had
        # missed the lattice layers and the pyramid; the C side then quietly ran unsplit).  Hence no list: the plan walks its own
        # forward once with `planning` set -- every launch site resolves its route, packs that route's bank, raises workspace_need
        # to that kernel's demand and returns without launching -- and allocates the scratch afterwards.
        self.workspace_need = 0
        self.workspace: Optional[torch.Tensor] = None
        self.planning = True
        self._plan_launches()
        self.planning = False
        if self.workspace_need:
            self.workspace = torch.empty((self.workspace_need // 4,), **kw)

    def _images(self, n: int) -> torch.Tensor:
        """shape-only stand-in for n input images (planning launches nothing)"""
        return torch.empty((n, 3, self.H, self.W), device="meta")

    def _plan_launches(self) -> None:
        """what run() launches"""
        B = self.B
        self._pyramid([(self._images(B), 0, B), (self._images(B), B, 2 * B)], 0, 2 * B)
        self._decode()

    @staticmethod
    def _slots(B: int) -> int:
        return 2 * B

    def _level_slots(self, B: int, level: int) -> int:
        """batch slots of level `level`'s two pyramid buffers (a plan may need fewer where no decoder level reads them)"""
        return self._slots(B)

    @staticmethod
    def _pair_views(buf: torch.Tensor, B: int):
        """first / second image's level features as dense views of the pyramid buffer"""
        return buf[:B], buf[B:]

    # ---- 96-cout layers as 64 couts on F(4x4) + 32 couts on F(2x2) -----------------------------------------------------
    # A 32-cout F(4x4) launch is four tile groups per workgroup: on a map that gives the 64-cout launch (two groups) enough workgroups it
    # leaves half the chip idle (conv3_2 at batch 16: 128 workgroups; dc_conv4 on its 14x32 lattice images), so the rule says no to the
    # whole layer.  Its first 64 couts still fill F(4x4); the last 32 go to F(2x2), whose 32-cout workgroups are smaller.
    @staticmethod
    def _split96_wanted(b: int, cin: int, h: int, w: int, cout: int) -> bool:
        return bool(cout == 96 and not ops.conv3x3_wino4_preferred(b, cin, h, w, 96) and ops.conv3x3_wino4_preferred(b, cin, h, w, 64)
                    and ops.conv3x3_wino_preferred(b, cin, h, w, 32, 1))

    def _pack_split96(self, key: str) -> None:
        w, b = self.p[key + ".weight"], self.p[key + ".bias"]
        self.wino4_packed[key + "[:64]"] = ops.pack_conv3x3_wino4(w[:64].contiguous())
        self.wino_packed[key + "[64:]"] = ops.pack_conv3x3_wino(w[64:].contiguous())
        self.split96_bias[key] = (b[:64].contiguous(), b[64:].contiguous())

    def _conv_split96(self, key: str, x: torch.Tensor, out: torch.Tensor, act: bool = True) -> None:
        self._route(key, *x.shape, 96, 1, 1, act, False, forced="split96")
        if self.planning:
            return
        macs = x.shape[0] * 96 * x.shape[1] * 9 * x.shape[2] * x.shape[3]
        self.conv_macs["direct"] += macs
        self.conv_macs["executed"] += macs * 2 // 3 * 36 // 144 + macs // 3 * 16 // 36
        b0, b1 = self.split96_bias[key]
        slope = LEAKY if act else None
        ops.conv3x3_wino4(x, self.wino4_packed[key + "[:64]"], b0, 64, leaky_slope=slope, out=out[:, :64], workspace=self.workspace)
        ops.conv3x3_wino(x, self.wino_packed[key + "[64:]"], b1, 32, leaky_slope=slope, out=out[:, 64:], workspace=self.workspace)

    # ---- which kernel runs a 3x3 layer: decided once per (layer, geometry) ------------------------
    def _rule(self, n: int, cin: int, h: int, w: int, cout: int, stride: int, dilation: int, act: bool, has_residual: bool) -> str:
        """Depends on the filter's shape, the geometry, the switches read when the plan was built and the library's measured rules;
        never on which banks are packed."""
        if self.conv_backend != "hip":
            return "torch"                                         # BASELINE config[1]: convolutions by PyTorch-ROCm (MIOpen)
        plain = stride == 1 and not has_residual
        wino = self.wino and cout >= 32 and cin >= 16 and plain    # the layers the Winograd kernels are built for
        if wino and self.wino4 and dilation == 1 and self._split96_wanted(n, cin, h, w, cout):
            return "split96"
        if self.pyr1_wino and (cout, cin) == (16, 16) and plain and dilation == 1 and act:
            # first pyramid level: Winograd F(2x2,3x3) with the whole filter bank in LDS (125 instead of 180 us per layer at batch 16)
            pyr1 = ops.pyr1_wino_preferred(n, h, w)
            if pyr1:
                return "pyr1x2" if pyr1 == 2 else "pyr1"           # x2: two consecutive such layers go as one launch (_conv16_pair)
        if wino and self.wino4 and dilation == 1 and ops.conv3x3_wino4_preferred(n, cin, h, w, cout):
            return "wino4"              # F(4x4,3x3): 4x fewer multiplications than the direct form, large well-filled layers
        if wino and ops.conv3x3_wino_preferred(n, cin, h, w, cout, dilation):
            return "wino2"              # F(2x2,3x3) on the matrix cores: 2.25x fewer MFMA passes for the same fp32 convolution
        return "direct"

    def _route(self, key: str, n: int, cin: int, h: int, w: int, cout: int, stride: int = 1, dilation: int = 1, act: bool = True,
               has_residual: bool = False, forced: Optional[str] = None) -> str:
        """"split96" | "pyr1" | "pyr1x2" | "wino4" | "wino2" | "direct" | "torch" for this launch, from the plan's table.  `forced`: the
        site states its route (the lattice-major context network) instead of asking _rule.  A launch seen for the first time packs
        the bank(s) its route reads; while the plan is built it also raises workspace_need to its kernel's demand.  After that the
        table only grows for callers that drive _conv with shapes the plan does not launch (bench probes): they may pack, the
        scratch stays -- every C entry compares the buffer with its own demand and runs unsplit when it is short."""
        geo = (key, n, cin, h, w, cout, stride, dilation, act, has_residual, forced)
        route = self.routes.get(geo)
        if route is not None:
            return route
        route = self.routes[geo] = forced or self._rule(*geo[1:-1])
        wt, need = self.p[key + ".weight"], 0
        if route == "split96":
            if key not in self.split96_bias:
                self._pack_split96(key)
            need = max(ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, 64), ops.conv3x3_wino_workspace_bytes(n, cin, h, w, 32, 1))
        elif route in ("pyr1", "pyr1x2"):
            if key not in self.pyr1_packed:
                self.pyr1_packed[key] = ops.pack_pyr1_wino(wt)
        elif route == "wino4":
            if key not in self.wino4_packed:
                self.wino4_packed[key] = ops.pack_conv3x3_wino4(wt)
            need = ops.conv3x3_wino4_workspace_bytes(n, cin, h, w, cout)
        elif route == "wino2":
            if key not in self.wino_packed:
                self.wino_packed[key] = ops.pack_conv3x3_wino(wt)
            need = ops.conv3x3_wino_workspace_bytes(n, cin, h, w, cout, dilation)
        elif route == "direct":
            if key not in self.packed:
                self.packed[key] = ops.pack_conv3x3(wt)
            need = ops.conv3x3_workspace_bytes(n, cin, h, w, cout, stride, dilation)
        if self.planning:
            self.workspace_need = max(self.workspace_need, need)
        return route

    # ---- layer primitives -----------------------------------------------------------------------
    def _conv(self, name: str, x: torch.Tensor, out: torch.Tensor, stride: int = 1, dilation: int = 1,
              act: bool = True, residual: Optional[torch.Tensor] = None, *, forced: Optional[str] = None, split2: bool = False) -> None:
        """forced / split2 (the lattice-major context network): the route stated, not asked; F(4x4) storing its result as four pixel lattices"""
        key = name + ".0" if (name + ".0.weight") in self.p else name
        w, b = self.p[key + ".weight"], self.p[key + ".bias"]
        cout = w.shape[0]
        route = self._route(key, *x.shape, cout, stride, dilation, act, residual is not None, forced)
        if route == "split96":
            self._conv_split96(key, x, out, act)
            return
        if self.planning:
            return
        macs = x.shape[0] * cout * w.shape[1] * 9 * ((x.shape[2] - 1) // stride + 1) * ((x.shape[3] - 1) // stride + 1)
        self.conv_macs["direct"] += macs                          # what the layer costs as a direct convolution
        num, den = ROUTE_MACS[route]
        self.conv_macs["executed"] += macs * num // den           # multiplications the matrix cores actually perform
        slope = LEAKY if act else None
        if route in ("pyr1", "pyr1x2"):
            ops.pyr1_wino(x, self.pyr1_packed[key], b, leaky_slope=LEAKY, out=out)
        elif route == "wino4":
            ops.conv3x3_wino4(x, self.wino4_packed[key], b, cout, leaky_slope=slope, out=out, split2=split2, workspace=self.workspace)
        elif route == "wino2":
            ops.conv3x3_wino(x, self.wino_packed[key], b, cout, leaky_slope=slope, out=out, dilation=dilation, workspace=self.workspace)
        elif route == "direct":
            ops.conv3x3(x, self.packed[key], b, cout, stride=stride, dilation=dilation, leaky_slope=slope, residual=residual, out=out,
                        workspace=self.workspace)
        else:
            y = F.conv2d(x, w, b, stride=stride, padding=dilation, dilation=dilation)
            if act:
                y = F.leaky_relu(y, LEAKY)
            if residual is not None:
                y = y + residual
            out.copy_(y)

    def _conv16_pair(self, name1: str, name2: str, x: torch.Tensor, out: torch.Tensor) -> bool:
        """Two consecutive 16 -> 16 layers (conv1aa, conv1b) as one launch where the rule says so; False: the caller runs them one by one"""
        k1, k2 = name1 + ".0", name2 + ".0"
        geo = (*x.shape, self.p[k1 + ".weight"].shape[0])
        if not (self._route(k1, *geo) == "pyr1x2" and self._route(k2, *geo) == "pyr1x2"):
            return False
        if self.planning:
            return True
        macs = 2 * x.shape[0] * 16 * 16 * 9 * x.shape[2] * x.shape[3]
        self.conv_macs["direct"] += macs
        self.conv_macs["executed"] += macs * 16 // 36              # the tiles' recomputed ring (1.22x on the first layer) is not counted
        ops.pyr1_wino_pair(x, self.pyr1_packed[k1], self.p[k1 + ".bias"], self.pyr1_packed[k2], self.p[k2 + ".bias"], leaky_slope=LEAKY, out=out)
        return True

    def _deconv(self, name: str, x: torch.Tensor, out: torch.Tensor) -> None:
        if self.planning:
            return
        w, b = self.p[name + ".weight"], self.p[name + ".bias"]
        if self.conv_backend == "hip":
            ops.deconv4x4s2(x, w, b, out=out)
        else:
            out.copy_(F.conv_transpose2d(x, w, b, stride=2, padding=1))

    # ---- the forward ----------------------------------------------------------------------------
    def run(self, x: torch.Tensor) -> torch.Tensor:
        B = self.B
        if tuple(x.shape) != (B, 6, self.H, self.W) or x.dtype != self.dtype or x.device != self.device:
            raise ValueError("plan built for %s %s on %s, got %s %s on %s" % (
                (B, 6, self.H, self.W), self.dtype, self.device, tuple(x.shape), x.dtype, x.device))
        x = ops.densify(x)
        self.conv_macs = {"direct": 0, "executed": 0}           # 3x3 layers of this run (bench.py: utilisation of the matrix cores)
        # -- feature pyramid, both images as one 2B batch (PWCNet.py:184-195) ----------------------
        self._pyramid([(x[:, :3], 0, B), (x[:, 3:], B, 2 * B)], 0, 2 * B)
        return self._decode()

    def _pyramid(self, images, lo: int, hi: int) -> None:
        """conv1a..conv6b over the batch slots [lo,hi) of the pyramid buffers; `images` lists
        (rgb [n,3,H,W], slot_lo, slot_hi) sources for the first conv."""
        prev = None
        for l in range(1, 7):
            na, naa, nb = self.pyramid_names[l - 1]
            a, bb = self.pyr_a[l][lo:hi], self.pyr_b[l][lo:hi]
            # three convs a -> bb -> a (PWCNet.py:184-195); two for PWCDCNet_old, bb -> a (PWCNet.py:411-422)
            first = self.pyr_a[l] if naa is not None else self.pyr_b[l]
            if l == 1:
                for img, s0, s1 in images:
                    self._conv(na, img, first[s0:s1], stride=2)
            else:
                self._conv(na, prev, first[lo:hi], stride=2)
            if naa is not None and self._conv16_pair(naa, nb, a, bb):
                prev = bb                                          # conv1aa + conv1b as one launch, a -> bb (tiles read their neighbours: not in place)
                continue
            if naa is not None:
                self._conv(naa, a, bb)
            self._conv(nb, bb, a)
            prev = a

    def _decode(self) -> Optional[torch.Tensor]:
        """Coarse-to-fine decoder + context network over self.c1[l] / self.c2[l] (PWCNet.py:198-268)."""
        for l in (6, 5, 4, 3, 2):
            self._level_entry(l)
            if l == 2 and not self.trunk2:
                return None                                        # the caller (engine_strict) takes over from the level-2 base channels
            self._dense(l)
            self._heads(l)
        return self._context()

    def _level_entry(self, l: int) -> None:
        """Cost volume of level l into its arena slot (PWCNet.py:198-199, 212-214 ...): plain correlation at level 6; below, c1
        into its slot and warp(c2, up_flow * scale) + correlation + LeakyReLU as one kernel."""
        if self.planning:
            return                                                 # no convolution, no scratch
        nd, base = self.nd, self.arena_base[l]
        ar = self.arena[l]
        c = PYRAMID_CH[l]
        corr_slot = ar[:, base:base + nd]
        if l == 6:
            ops.correlation(self.c1[6], self.c2[6], self.md, 1, self.md, 1, 1, 1.0,
                            normalize=self.normalize_corr, leaky_slope=LEAKY, out=corr_slot)
            return
        off = base + nd
        # first image's level features go into the level's arena slot (they are part of the
        # dense block's input, PWCNet.py:215); c2 is only ever read by the warp
        if not self.c1_in_arena:
            ar[:, off:off + c].copy_(self.c1[l])
        up_flow = ar[:, off + c:off + c + 2]
        # warp + correlation + LeakyReLU as one kernel (the warped features live in LDS only) where the geometry
        # allows it (md = 4, W % 4 == 0) and the map is more than a few tiles; otherwise the two operators
        fused = None
        if self.fuse_warp and self.md == 4 and ops.warp_correlation_preferred(ar.shape[0], c, *self.size[l]):
            fused = ops.warp_correlation(ar[:, off:off + c], self.c2[l], up_flow, flow_scale=WARP_SCALE[l],
                                         align_corners=self.align_corners, mask_threshold=self.mask_threshold,
                                         normalize=self.normalize_corr, leaky_slope=LEAKY, out=corr_slot)
        if fused is None:
            ops.warp(self.c2[l], up_flow, flow_scale=WARP_SCALE[l], align_corners=self.align_corners,
                     mask_threshold=self.mask_threshold, out=self.warped[l])
            ops.correlation(ar[:, off:off + c], self.warped[l], self.md, 1, self.md, 1, 1, 1.0,
                            normalize=self.normalize_corr, leaky_slope=LEAKY, out=corr_slot)

    def _dense(self, l: int) -> None:
        """DenseNet block convL_0..convL_4 (PWCNet.py:202-206 ...): each layer reads a channel suffix of the arena and writes
        its slice in front of it."""
        ar = self.arena[l]
        lo = self.arena_base[l]
        for i, (co, off_i) in enumerate(zip(DENSE_OUT, DENSE_OFF)):
            self._conv("conv%d_%d" % (l, i), ar[:, lo:], ar[:, off_i:off_i + co])
            lo = off_i

    def _heads(self, l: int) -> None:
        """predict_flowL, and for l > 2 deconvL / upfeatL into the next level's arena (PWCNet.py:207-209 ...)."""
        ar = self.arena[l]
        if l == 2:
            self._conv("predict_flow2", ar, self.flow[2], act=False)
            return
        nxt = self.arena[l - 1]
        cn = PYRAMID_CH[l - 1]
        o = self.arena_base[l - 1] + self.nd + cn
        h, w = self.size[l]
        if l in self.head10:
            self._conv("head10_%d" % l, ar, self.head10[l], act=False)
            if not self.planning:
                ops.upsample_entry(self.head10[l], self.p["deconv%d.weight" % l], self.p["deconv%d.bias" % l], nxt[:, o:o + 4])
            return
        if self.stream_head[l] and self.planning:
            # the one-pass kernel reads predict_flowL's direct bank and cuts a launch smaller than the chip along Cin through the scratch
            self.packed["predict_flow%d" % l] = ops.pack_conv3x3(self.p["predict_flow%d.weight" % l])
            self.workspace_need = max(self.workspace_need, ops.head_upfeat_workspace_bytes(*ar.shape))
        elif self.stream_head[l]:
            # predict_flowL and upfeatL read the same 3x3 windows of the same arena: one pass
            ops.head_upfeat(ar, self.packed["predict_flow%d" % l], self.p["predict_flow%d.bias" % l],
                            self.p["upfeat%d.weight" % l], self.p["upfeat%d.bias" % l],
                            self.flow[l], nxt[:, o + 2:o + 4], workspace=self.workspace)
        else:
            self._conv("predict_flow%d" % l, ar, self.flow[l], act=False)
            self._deconv("upfeat%d" % l, ar, nxt[:, o + 2:o + 4])
        self._deconv("deconv%d" % l, self.flow[l], nxt[:, o:o + 2])

    def _context(self) -> torch.Tensor:
        """Context network + residual (PWCNet.py:267-268)."""
        if self.ctx_lattice:
            return self._context_lattice()
        t = self.arena[2]
        for i, (_, dil) in enumerate(CONTEXT):
            self._conv("dc_conv%d" % (i + 1), t, self.ctx[i], dilation=dil)
            t = self.ctx[i]
        self._conv("dc_conv7", t, self.flow_out, act=False, residual=self.flow[2])
        return self.flow_out

    def _context_lattice(self) -> torch.Tensor:
        """The same seven layers with dc_conv1..5 in lattice-major layout (see __init__): every layer is the reference's layer on the
        same values, only the order in which pixels are stored between them differs."""
        w4 = dict(forced="wino4", split2=True)
        self._conv("dc_conv1", self.arena[2], self.ctx[0], **w4)  # [B,565,H,W]      -> 4B  x [128,H/2,W/2]   (lattices of dilation 2)
        self._conv("dc_conv2", self.ctx[0], self.ctx[1], **w4)    # dilation 2 = 1 on those -> 16B x [128,H/4,W/4]
        self._conv("dc_conv3", self.ctx[1], self.ctx[2], **w4)    # dilation 4 = 1          -> 64B x [128,H/8,W/8]
        if self.ctx_lattice4:
            self._conv("dc_conv4", self.ctx[2], self.ctx[3], **w4)                 # dilation 8 = 1 -> 256B x [96,H/16,W/16]
            self._conv("dc_conv5", self.ctx[3], self.ctx4_lat, forced="wino4")     # dilation 16 = 1 on those (stacked tile groups: 7x16 images)
        else:
            if self.dc4_split:                                     # dilation 8 = 1 on the dilation-8 lattices: 64 couts F(4x4) + 32 couts F(2x2)
                self._conv_split96("dc_conv4.0", self.ctx[2], self.ctx[3])
            else:
                self._conv("dc_conv4", self.ctx[2], self.ctx[3], dilation=1)
            self._conv("dc_conv5", self.ctx[3], self.ctx4_lat, dilation=2)         # dilation 16 = 2 on them
        if not self.planning:
            ops.lattice_unsplit(self.ctx4_lat, self.B, 4 if self.ctx_lattice4 else 3, out=self.ctx[4])
        self._conv("dc_conv6", self.ctx[4], self.ctx[5], dilation=1)
        self._conv("dc_conv7", self.ctx[5], self.flow_out, act=False, residual=self.flow[2])
        return self.flow_out

    def flows(self) -> Tuple[torch.Tensor, ...]:
        """(flow2, flow3, flow4, flow5, flow6) of the last run -- the training-mode return (PWCNet.py:270-271)."""
        return (self.flow_out, self.flow[3], self.flow[4], self.flow[5], self.flow[6])

    def bytes_allocated(self) -> int:
        tot = 0
        for group in (self.pyr_a, self.pyr_b, self.warped, self.arena, self.flow):
            tot += sum(t.numel() * t.element_size() for t in group.values())
        if self.c1_in_arena:                                    # pyr_a[2..5] are views of the arenas, which hold 2B items
            for l in range(2, 6):
                tot += (self.arena[l].numel() - self.pyr_a[l].numel()) * self.arena[l].element_size()
        tot += sum(t.numel() * t.element_size() for t in self.ctx + ([self.flow_out] if self.flow_out is not None else []))
        if self.ctx4_lat is not None:
            tot += self.ctx4_lat.numel() * self.ctx4_lat.element_size()
        tot += sum(t.numel() * t.element_size() for t in self.packed.values())
        tot += sum(t.numel() * t.element_size() for t in self.wino_packed.values())
        tot += sum(t.numel() * t.element_size() for t in self.wino4_packed.values())
        tot += sum(t.numel() * t.element_size() for t in self.pyr1_packed.values())
        if self.workspace is not None:
            tot += self.workspace.numel() * self.workspace.element_size()
        return tot


class VideoDriver:
    """prime() / push() of the video plans (PwcVideoPlan here, engine_f16.PwcVideoPlanF16): float32 frames in, B + 1 batch slots per
    pyramid buffer, slot 0 carrying the last frame of the previous step.  The plan class provides _pyramid, _decode, pyr_a, B, H, W."""
    primed = False

    def _check(self, frames: torch.Tensor, n: int) -> torch.Tensor:
        if tuple(frames.shape) != (n, 3, self.H, self.W) or frames.dtype != torch.float32 or frames.device != self.device:
            raise ValueError("expected float32 frames %s on %s, got %s %s on %s" % (
                (n, 3, self.H, self.W), self.device, frames.dtype, tuple(frames.shape), frames.device))
        return ops.densify(frames)

    def _carry(self) -> None:
        for l in range(2, 7):
            self.pyr_a[l][0].copy_(self.pyr_a[l][self.B])

    def prime(self, frame: torch.Tensor) -> None:
        """Pyramid of the very first frame [1,3,H,W] -> carry slot."""
        f = self._check(frame, 1)
        self._pyramid([(f, self.B, self.B + 1)], self.B, self.B + 1)
        self._carry()
        self.primed = True

    def push(self, frames: torch.Tensor, tail=None) -> torch.Tensor:
        """B new frames [B,3,H,W] -> flows of the pairs (previous, frames[0]), (frames[0], frames[1]), ...
        tail: a callable that finishes the decoder and returns the flow (engine_strict.PwcVideoPlanStrict: the half-precision level 2 of
        a trunk2=False plan).  It runs BEFORE the carry, which with c1_in_arena (batch 1) overwrites the c1 channels of the arenas."""
        if not self.primed:
            raise RuntimeError("%s.push before prime(first_frame)" % type(self).__name__)
        f = self._check(frames, self.B)
        self._pyramid([(f, 1, self.B + 1)], 1, self.B + 1)
        out = self._decode()
        if tail is not None:
            out = tail()
        self._carry()
        return out

    def run(self, x):
        raise RuntimeError("%s is driven by prime()/push(), not run()" % type(self).__name__)


class PwcVideoPlan(VideoDriver, PwcPlan):
    """Plan for consecutive frame pairs (f[t], f[t+1]) of one video, the loop of
    ``pwc_extract_flow_video.py:262-305`` (``frame1 = frame2`` each iteration).

    The reference runs the feature pyramid on both frames of every pair, i.e. twice per frame.  Here each
    level's pyramid buffer has B+1 batch slots: slot 0 carries the last frame of the previous step, slots
    1..B receive the pyramid of the B new frames, and the decoder's first/second-image features are the
    overlapping views [0:B] / [1:B+1] of the same buffer -- no copy, one pyramid pass per frame.
    """

    @staticmethod
    def _slots(B: int) -> int:
        return B + 1

    @staticmethod
    def _pair_views(buf: torch.Tensor, B: int):
        return buf[:B], buf[1:]

    def _plan_launches(self) -> None:
        """what prime() and push() launch"""
        B = self.B
        self._pyramid([(self._images(1), B, B + 1)], B, B + 1)
        self._pyramid([(self._images(B), 1, B + 1)], 1, B + 1)
        self._decode()


class PwcBidirPlan(PwcPlan):
    """Both flow directions of B pairs from ONE pyramid pass over their 2B images: ``run(img1, img2) -> (flow12, flow21)`` with
    flow12 = net(cat(img1, img2)) and flow21 = net(cat(img2, img1)) (the two forwards of the scripts' cycle-consistency check,
    train_pseudo.py:178-193 / train_fundamental.py:397-409, which run six pyramids over two distinct images).

    Layout: 3B pyramid slots [img1 | img2 | copy of img1's levels 2..6] and ONE decoder pass at batch 2B.  The decoder's
    first-image features are the view [0:2B] = (img1, img2), its second-image features the overlapping view [B:3B] =
    (img2, img1), as PwcVideoPlan overlaps [0:B] / [1:B+1]: items 0..B-1 decode the pairs (img1, img2), items B..2B-1 the pairs
    (img2, img1).  Every image passes conv1a..conv6b exactly once (slots [0,2B)); the third block is a device copy of B sets of
    level features.  With 3B slots for a 2B decoder c1_in_arena switches itself off, so the decoder copies c1 into its arena
    as for the video plan.  The base class is built for the DECODER batch 2B; its kernels, packed filters and workspace are
    PwcPlan's."""

    def __init__(self, params, B, H, W, device, dtype=torch.float32, md=4, normalize_corr=False,
                 align_corners=False, conv_backend="hip", variant="dc"):
        self.pairs = int(B)
        super().__init__(params, 2 * B, H, W, device, dtype, md, normalize_corr, align_corners, conv_backend, variant)

    @staticmethod
    def _slots(B2: int) -> int:
        return B2 + B2 // 2                     # B2 = 2B decoder items -> 3B pyramid slots

    def _level_slots(self, B2: int, level: int) -> int:
        # level 1 feeds only the pyramid (no decoder level reads it): the third block of slots would never be touched there
        return B2 if level == 1 else self._slots(B2)

    @staticmethod
    def _pair_views(buf: torch.Tensor, B2: int):
        return buf[:B2], buf[B2 // 2:]

    def _plan_launches(self) -> None:
        """what run() launches: the pyramid on the 2B images (not on all 3B slots), the decoder at batch 2B"""
        B = self.pairs
        self._pyramid([(self._images(B), 0, B), (self._images(B), B, 2 * B)], 0, 2 * B)
        self._decode()

    def run(self, img1: torch.Tensor, img2: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        B = self.pairs
        for name, t in (("img1", img1), ("img2", img2)):
            if t is None or tuple(t.shape) != (B, 3, self.H, self.W) or t.dtype != self.dtype or t.device != self.device:
                raise ValueError("plan built for two %s %s images on %s, got %s: %s" % (
                    (B, 3, self.H, self.W), self.dtype, self.device, name, None if t is None else (tuple(t.shape), t.dtype, t.device)))
        self.conv_macs = {"direct": 0, "executed": 0}
        self._pyramid([(ops.densify(img1), 0, B), (ops.densify(img2), B, 2 * B)], 0, 2 * B)
        for l in range(2, 7):
            self.pyr_a[l][2 * B:].copy_(self.pyr_a[l][:B])
        out = self._decode()
        return out[:B], out[B:]
