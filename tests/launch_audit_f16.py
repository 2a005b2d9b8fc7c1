"""Launch audit of the half-precision plans (tests/test_gpu_launch_audit_f16.py): every ops_f16.* launch of one eager forward of
engine_f16.PwcPlanF16 / PwcVideoPlanF16 / engine_strict.PwcPlanStrict is checked right after it runs, against a float64 CPU
restatement of that ONE operator computed from the launch's own inputs, with a per-element bound.  The fp32 part of the strict plan
(plan.upper) is audited by launch_audit.LaunchAudit in the same run.

Every half-precision kernel multiplies half operands (products exact in fp32), accumulates in fp32 and rounds to half ONCE, at the
store, to nearest (pwc::sat_half, saturating at +-65504).  So per output element, with S the sum of |terms| (launch_audit.conv_ref):
    half out:   |got - ref| <= u |ref| + t + (1 + u) REL_F16 S        u = 2^-11 (unit roundoff), t = 2^-25 (half the subnormal step)
    fp32 out:   |got - ref| <= REL_F16 S
and where |ref| lies past 65504 by more than the accumulation bound, got is +-65504 with ref's sign.  Filters are NEVER read back from
the packed banks: each bank is mapped (by the packed tensor's identity) to the fp32 filters the plan's own preparation produced
(prepare_params / level_filters / context_filters, and the strict plan's residual-column copies, restated here), and the reference
rounds them to half -- or to the split form hi + half((w - hi) 2^11) / 2^11 -- itself, so a wrong pack fails.

On every launch, whatever the operator: the pad lanes (channels past C in the last c8 group of every output) are exactly zero, and no
element of the outputs' storages outside the declared output views changed (the arena is snapshot before the launch).
This module is a helper, not a test module (like launch_audit.py)."""
from __future__ import annotations

import inspect
import os
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

import launch_audit as LA
from launch_audit import bounded_ratio, corr_ref, near_threshold, pick_images, warp_apply, warp_taps, worst

U16 = 2.0 ** -11           # unit roundoff of half (round to nearest)
T16 = 2.0 ** -25           # half the subnormal step of half: the absolute rounding error below 2^-14
HALF_MAX = 65504.0
# fp32 accumulation of products that are exact in fp32 (half x half, and the fp32 image x fp32 filter FMAs of image_conv_s2): the
# same summation structure as the fp32 direct kernels, so the same multiple of S as launch_audit.REL_DIRECT.  The conv kernels sum
# 16-channel MFMA steps (v_mfma_f32_32x32x16_f16: 16 exact products into the fp32 accumulator) in K-chunk order; the split form adds
# acc_lo / 2^11 once; the correlation chains v_dot2_f32_f16 over C/2 steps.  Observed worst ratios are in DESIGN.md section 7a.
REL_F16 = 1.0e-6
REL_WARP = LA.REL_WARP     # fp32 bilinear blend of four taps (four products, three adds), as in the fp32 warp
ENTRY_DOUBLE_ROUNDING_MAX = 4   # up_flow restated as fp64 a*b+c rounded to fp32: a tie of that double rounding may move one bit
SPLIT_REL, SPLIT_ABS = 2.0 ** -22, 2.0 ** -36   # |w_eff - w| of the split filters ("~22-bit filters")

# ---- routes the suite must reach (test_route_coverage_f16) -------------------------------------------------------------------
# conv16/<kernel and template arguments as pwc_last_conv_kernel names them>[/split][/f32]: conv3x3_f16_kernel<MT, NT, S, D, R, 0>,
# conv3x3_f16w8_kernel<MT, 2, 1, D, 2, 32>.  The plans reach no tall NT = 4 tile and no two-per-CU 2-slot ring at dilation 1: at the
# tile counts where those rules fire, the w8 kernel takes the layer first (dispatch16)
ROUTES_REQUIRED_F16 = (
    "conv16/conv3x3_f16_kernel<1, 2, 1, 1, 3, 0>",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 1, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 1, 3, 0>/split/f32",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 16, 2, 0>",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 16, 2, 0>/split",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 2, 3, 0>",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 4, 3, 0>",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 8, 3, 0>",
    "conv16/conv3x3_f16_kernel<1, 2, 1, 8, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<1, 2, 2, 1, 3, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 1, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 16, 2, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 2, 2, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 2, 2, 0>/split",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 2, 3, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 2, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 4, 2, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 4, 2, 0>/split",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 4, 3, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 4, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 8, 2, 0>",
    "conv16/conv3x3_f16_kernel<2, 2, 1, 8, 2, 0>/split",
    "conv16/conv3x3_f16_kernel<2, 2, 2, 1, 3, 0>",
    "conv16/conv3x3_f16_kernel<3, 2, 1, 1, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<3, 2, 1, 16, 2, 0>/split",
    "conv16/conv3x3_f16_kernel<3, 2, 1, 2, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<3, 2, 1, 4, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<3, 2, 1, 8, 2, 0>",
    "conv16/conv3x3_f16_kernel<3, 2, 2, 1, 2, 0>",
    "conv16/conv3x3_f16_kernel<4, 2, 1, 2, 3, 0>",
    "conv16/conv3x3_f16_kernel<4, 2, 1, 2, 3, 0>/split",
    "conv16/conv3x3_f16_kernel<4, 2, 1, 4, 2, 0>",
    "conv16/conv3x3_f16_kernel<4, 2, 1, 4, 2, 0>/split",
    "conv16/conv3x3_f16_kernel<4, 2, 1, 8, 2, 0>/split",
    "conv16/conv3x3_f16w8_kernel<1, 2, 1, 1, 2, 32>",
    "conv16/conv3x3_f16w8_kernel<2, 2, 1, 1, 2, 32>",
    "conv16/conv3x3_f16w8_kernel<2, 2, 1, 1, 2, 32>/split",
    "conv16/conv3x3_f16w8_kernel<3, 2, 1, 1, 2, 32>",
    "conv16/conv3x3_f16w8_kernel<3, 2, 1, 8, 2, 32>",
    "corr16/direct", "corr16/tiled",
    "entry/fused", "entry/two-launch",
    "pyr1/fused", "pyr1/image-s2",
    "handover/c8", "handover/hilo",
)

OPS_F16 = ("to_c8", "to_c8_hilo", "conv3x3_f16", "correlation_c8", "warp_c8", "level_entry", "level_entry_correlation",
           "image_conv_s2", "pyramid1_fused")


# ---- restatements (CPU; used by the GPU audit and by tests/test_launch_audit_f16_cpu.py) ----------------------------------------
def c8_to_nchw(t: torch.Tensor) -> torch.Tensor:
    """[n,G,H,W,8] -> [n,8G,H,W] (same dtype; pad lanes included)"""
    n, g, h, w, _ = t.shape
    return t.permute(0, 1, 4, 2, 3).reshape(n, g * 8, h, w)


def sat_half(x: torch.Tensor) -> torch.Tensor:
    """pwc::sat_half: float32 -> half, round to nearest, +-65504 past the range, NaN stays NaN"""
    return x.float().clamp(-HALF_MAX, HALF_MAX).half()


def split_filters(w: torch.Tensor) -> torch.Tensor:
    """float64 effective filters of pack3x3_f16_kernel(split=1): hi = sat_half(w), lo = half((w - hi) * 2^11) (fp32 ops, the
    difference is exact), w_eff = hi + lo / 2^11"""
    w = w.float()
    hi = sat_half(w)
    lo = ((w - hi.float()) * 2048.0).half()
    return hi.double() + lo.double() / 2048.0


def half_ratio(got, ref, s, rel=REL_F16, half_out=True, extra=None, keep=None) -> torch.Tensor:
    """error / bound per element for a launch that accumulates in fp32 and rounds once to half (half_out) or stores fp32.
    `extra` (float64, >= 0) is a propagated input error added to the accumulation bound."""
    acc = rel * s.double()
    if extra is not None:
        acc = acc + extra
    ref = ref.double()
    if not half_out:
        return bounded_ratio(got, ref, acc, 1.0, keep)
    refc = ref.clamp(-HALF_MAX, HALF_MAX)
    r = bounded_ratio(got, refc, U16 * refc.abs() + T16 + (1 + U16) * acc, 1.0, keep)
    sat = (ref.abs() - acc) > HALF_MAX
    bad = sat & (got.double() != torch.sign(ref) * HALF_MAX)
    if keep is not None:
        bad = bad & keep
    return torch.where(bad, torch.full_like(r, float("inf")), r)


def fma32(a, b, c):
    """fmaf restated: exact product, sum in float64, rounded to float32 (a tie of this double rounding may differ by one ulp)"""
    return (a.double() * b.double() + c.double()).float()


def entry_up_flow(flow: torch.Tensor, dw: torch.Tensor, db: torch.Tensor, swap_tap: bool = False) -> torch.Tensor:
    """deconvL (ConvTranspose2d(2,2,k4,s2,p1)) of flow [n,2,h,w] float32 in entry_up_flow's own order (csrc/pwc_f16_ops.hip):
    acc = bias; for the input rows a = 0,1 and columns c = 0,1 in range: fmaf over (ci 0, ci 1) per output channel.
    swap_tap (mutation tests only): kernel row taken from the other input row."""
    n, _, hh, wh = flow.shape
    H, W = 2 * hh, 2 * wh
    Y, X = torch.arange(H), torch.arange(W)
    py, px = Y & 1, X & 1
    dw, db = dw.float(), db.float()
    acc = [torch.full((n, H, W), float(db[0])), torch.full((n, H, W), float(db[1]))]
    for a in range(2):
        r = (Y >> 1) - 1 + py + a
        ky = 3 - py - 2 * ((1 - a) if swap_tap else a)
        vr = (r >= 0) & (r < hh)
        for c in range(2):
            cc = (X >> 1) - 1 + px + c
            kx = 3 - px - 2 * c
            vc = (cc >= 0) & (cc < wh)
            valid = (vr.view(H, 1) & vc.view(1, W)).unsqueeze(0)
            f = flow.float()[:, :, r.clamp(0, hh - 1)][:, :, :, cc.clamp(0, wh - 1)]       # [n,2,H,W]
            for co in range(2):
                for ci in range(2):
                    wk = dw[ci, co][ky.view(H, 1), kx.view(1, W)]
                    acc[co] = torch.where(valid, fma32(f[:, ci], wk, acc[co]), acc[co])
    return torch.stack(acc, 1)


def feat_shuffle(phases: torch.Tensor) -> torch.Tensor:
    """[n,1,h,w,8] float32 phases (channel co*4 + py*2 + px) -> up_feat [n,2,2h,2w]"""
    n, _, h, w, _ = phases.shape
    return phases[:, 0].reshape(n, h, w, 2, 2, 2).permute(0, 3, 1, 4, 2, 5).reshape(n, 2, 2 * h, 2 * w)


def _flip_allowance(v: torch.Tensor, window: torch.Tensor) -> torch.Tensor:
    """|half(v_kernel) - half(v)| for a kernel value within `window` of v: 0 unless a rounding midpoint of half lies within the
    window, else at most window + one ulp"""
    h = v.float().clamp(-HALF_MAX, HALF_MAX).half()
    up = torch.nextafter(h, torch.full_like(h, float("inf"))).double()
    dn = torch.nextafter(h, torch.full_like(h, float("-inf"))).double()
    hd = h.double()
    d = torch.minimum((v - (hd + up) / 2).abs(), (v - (hd + dn) / 2).abs())
    return torch.where(d <= window, window + torch.maximum(up - hd, hd - dn), torch.zeros_like(v))


def pyr1_chain(x: torch.Tensor, layers, slope: float = LA.LEAKY, pad_mode: str = "zeros"):
    """The chain conv1a (s2) -> conv1aa -> conv1b -> conv2a (s2) of pyramid1_fused restated in float64 with the kernel's roundings:
    the image read as halves, every stage rounded to half once (maps zero outside the image).  Returns (float64 reference of the
    output, allowance per element).  The kernel's fp32 value of a stage lies within window_k = REL_F16 S_k + conv(F_k-1, |w_k|) of the
    float64 one (F_k-1: the allowance of the stage before); it rounds to the same half unless a rounding midpoint lies inside that
    window, and then to within window + one ulp (F_k).  A few % of a stage's values lie that close to a midpoint, and the next
    stage's 3x3 windows spread their allowance, so by conv2a the allowance is a few % of the values: still ~50x tighter than the
    worst-case propagation E_k+1 = u|r| + t + (1+u)(REL S + conv(E_k, |w|)) of the unrounded chain, which
    grows by ||w||_1 ~ 17 per stage at these layers' fan-in, ends larger than the values themselves and would pass a wrong
    padding.  layers: [(w, b, stride)] with the filters as the kernel reads them (halves).  pad_mode "replicate": mutation tests."""
    r = x.float().half().double()
    f = torch.zeros_like(r)
    for w, b, stride in layers:
        wd = w.double()

        def conv(t, k, bb):
            if pad_mode == "zeros":
                return F.conv2d(t, k, bb, stride=stride, padding=1)
            return F.conv2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), k, bb, stride=stride)
        v = F.leaky_relu(conv(r, wd, b.double()), slope)
        window = REL_F16 * conv(r.abs(), wd.abs(), b.double().abs()) + conv(f, wd.abs(), None)
        f = _flip_allowance(v, window)
        r = sat_half(v).double()
    return r, f


def family_f16(route: str) -> str:
    """conv16 (half out) / conv16-f32 (fp32 out: the accumulation bound alone) / corr16 / entry / handover / pyr1/<kernel>"""
    parts = route.split("/")
    if parts[0] == "conv16":
        return "conv16-f32" if parts[-1] == "f32" else "conv16"
    return route if parts[0] == "pyr1" else parts[0]


class _Guard:
    """snapshot of the storages behind a launch's outputs; after the launch, count the elements outside the declared output views
    whose bits changed (stray stores).  Compared as 16-bit words on the device."""

    def __init__(self, outs):
        self.items = {}
        for t in outs:
            st = t.untyped_storage()
            key = st.data_ptr()
            if key not in self.items:
                flat = torch.empty(0, dtype=torch.int16, device=t.device).set_(st)
                self.items[key] = [flat, flat.clone(), torch.zeros(flat.shape, dtype=torch.bool, device=t.device)]
            k = t.element_size() // 2
            mask = self.items[key][2]
            mask.as_strided(tuple(t.shape) + (k,), tuple(s * k for s in t.stride()) + (1,), t.storage_offset() * k).fill_(True)

    def stray(self) -> int:
        n = 0
        for flat, snap, mask in self.items.values():
            n += int(((flat != snap) & ~mask).sum())
        self.items = {}
        return n


def _pad_lanes_zero(t: torch.Tensor, c: int) -> bool:
    """channels >= c of the last c8 group of t are exactly zero (whole tensor, on the device)"""
    if c % 8 == 0:
        return True
    return bool((t[:, -1, :, :, c % 8:] == 0).all())


# ---- the spies ---------------------------------------------------------------------------------------------------------------------
class LaunchAuditF16:
    """`LaunchAuditF16(params)` with the plan's fp32 state dict, then `install(monkeypatch, plan)`, run the plan eagerly, read
    `records` / `routes`.  Every record: {op, route, shape, images, ratio, excluded, pixels, stray, pad_ok}."""

    def __init__(self, params: Dict[str, torch.Tensor], seed: int = 0):
        self.params = params
        self.seed = seed
        self.records: List[Dict] = []
        self.filters: Dict[int, tuple] = {}
        self.pyr1: Dict[int, list] = {}
        self.split_checked = set()
        self.real = {}
        self.upper: Optional[LA.LaunchAudit] = None

    @property
    def routes(self):
        r = {x["route"] for x in self.records}
        return r | (self.upper.routes if self.upper is not None else set())

    def all_records(self):
        return self.records + (self.upper.records if self.upper is not None else [])

    def worst_by_family(self) -> Dict[str, float]:
        out: Dict[str, float] = {}
        for r in self.records:
            fam = family_f16(r["route"])
            out[fam] = max(out.get(fam, 0.0), r["ratio"])
        if self.upper is not None:
            for k, v in self.upper.worst_by_family().items():
                out["fp32:" + k] = v
        return out

    def failures(self):
        bad = [r for r in self.records if not (r["ratio"] <= 1.0) or r["stray"] or not r["pad_ok"]]
        return bad + (self.upper.failures() if self.upper is not None else [])

    def _record(self, op, route, shape, images, ratio, stray, pad_ok, excluded=0, pixels=0, **extra):
        self.records.append(dict(op=op, route=route, shape=tuple(shape), images=images, ratio=float(ratio), stray=int(stray),
                                 pad_ok=bool(pad_ok), excluded=int(excluded), pixels=int(pixels), **extra))

    # ---- raw filters through the plan's own preparation ------------------------------------------------------------------------
    def _map_filters(self, plan) -> None:
        from opticalflow_amd import engine_strict
        from opticalflow_amd.engine_f16 import _groups, _pad_cin, context_filters, level_filters, prepare_params
        strict = isinstance(plan, engine_strict.PwcPlanStrict)
        variant = plan.upper.variant if strict else plan.variant
        p = prepare_params(self.params, variant, plan.nd)
        raw = {}
        if strict:
            nphys = int(plan.arena.shape[1]) * 8
            g2 = _groups(engine_strict.PYRAMID_CH[2])
            corr0, flow0 = engine_strict.BASE_G * 8, (plan.f0 + g2) * 8
            rc0, rf0 = plan.r_corr * 8, plan.r_flow * 8
            cg8 = engine_strict.CORR_G * 8
            for name, w, b, _ in list(level_filters(p, 2, nphys, plan.nd)) + list(context_filters(p)):
                if not name.startswith("dc_conv") or name == "dc_conv1":
                    ps = nphys - w.shape[1]                       # the residual channel sets carry the filters of the sets they correct
                    w = w.clone()
                    w[:, rc0 - ps:rc0 + cg8 - ps] = w[:, corr0 - ps:corr0 + cg8 - ps]
                    w[:, rf0 - ps:rf0 + 8 - ps] = w[:, flow0 - ps:flow0 + 8 - ps]
                raw[name] = (w, b, plan.split[name])
        else:
            for l, names in enumerate(plan.pyramid_names, start=1):
                for i, n in enumerate(names):
                    if n is None or (l == 1 and i == 0):
                        continue
                    w = p[n + ".0.weight"]
                    raw[n] = (_pad_cin(w, _groups(w.shape[1]) * 8), p[n + ".0.bias"], n in plan.split)
            for l in range(2, 7):
                for name, w, b, _ in level_filters(p, l, int(plan.arena[l].shape[1]) * 8, plan.nd):
                    raw[name] = (w, b, name in plan.split)
            for name, w, b, _ in context_filters(p):
                raw[name] = (w, b, name in plan.split)
            if plan.pyr1 is not None:
                self.pyr1[id(plan.pyr1[0])] = [(p[k + ".0.weight"], p[k + ".0.bias"], s)
                                               for k, s in (("conv1a", 2), ("conv1aa", 1), ("conv1b", 1), ("conv2a", 2))]
        assert set(raw) == set(plan.w), sorted(set(raw) ^ set(plan.w))
        for name, (w, b, split) in raw.items():
            self.filters[id(plan.w[name])] = (name, w.detach().float().cpu(), b.detach().float().cpu(), split)
        self.conv1a = (p["conv1a.0.weight"].detach().float().cpu(), p["conv1a.0.bias"].detach().float().cpu())

    def install(self, monkeypatch, plan) -> None:
        from opticalflow_amd import engine_strict, ops_f16
        self._map_filters(plan)
        if isinstance(plan, engine_strict.PwcPlanStrict):
            self.upper = LA.LaunchAudit(seed=self.seed)
            self.upper.install(monkeypatch, plan.upper)
        self.real = {n: getattr(ops_f16, n) for n in OPS_F16}
        for n in OPS_F16:
            monkeypatch.setattr(ops_f16, n, self._spy(n, self.real[n]))

    def _spy(self, name, real):
        sig = inspect.signature(real)
        check = getattr(self, "_check_" + name)

        def f(*a, **kw):
            ba = sig.bind(*a, **kw)
            ba.apply_defaults()
            return check(real, ba.arguments)
        return f

    def _imgs(self, n):
        return pick_images(n, self.seed + len(self.records))

    # ---- layout conversions --------------------------------------------------------------------------------------------------------
    def _check_to_c8(self, real, A):
        x, out = A["x"], A["out"]
        c = x.shape[1]
        xs = x.cpu()
        guard = _Guard([out]) if out is not None else None
        out = real(**A)
        torch.cuda.synchronize()
        got = c8_to_nchw(out.cpu())
        ok = torch.equal(got[:, :c].view(torch.int16), sat_half(xs).view(torch.int16)) and bool((got[:, c:] == 0).all())
        self._record("to_c8", "handover/c8", x.shape, x.shape[0], 0.0 if ok else float("inf"),
                     guard.stray() if guard else 0, _pad_lanes_zero(out, c))
        return out

    def _check_to_c8_hilo(self, real, A):
        x, hi, lo = A["x"], A["out_hi"], A["out_lo"]
        c = x.shape[1]
        xs = x.cpu()
        guard = _Guard([hi, lo])
        real(**A)
        torch.cuda.synchronize()
        gh, gl = c8_to_nchw(hi.cpu()), c8_to_nchw(lo.cpu())
        rh = sat_half(xs)
        res = xs - rh.float()                                  # exact in fp32
        rl = torch.where(torch.isnan(res), torch.zeros_like(res), res)
        ok = (torch.equal(gh[:, :c].view(torch.int16), rh.view(torch.int16))
              and torch.equal(gl[:, :c].view(torch.int16), sat_half(rl).view(torch.int16))
              and bool((gh[:, c:] == 0).all()) and bool((gl[:, c:] == 0).all()))
        self._record("to_c8_hilo", "handover/hilo", x.shape, x.shape[0], 0.0 if ok else float("inf"), guard.stray(),
                     _pad_lanes_zero(hi, c) and _pad_lanes_zero(lo, c))

    # ---- convolutions ----------------------------------------------------------------------------------------------------------------
    def _check_conv3x3_f16(self, real, A):
        from opticalflow_amd import _lib
        x, out = A["x"], A["out"]
        cin, cout, stride, dil = A["cin"], A["cout"], A["stride"], A["dilation"]
        name, w, b, split_plan = self.filters[id(A["wpacked"])]
        split, out_f32 = A["split_w"], A["out_f32"]
        assert split == split_plan and w.shape[:2] == (cout, cin) and torch.equal(A["bias"].cpu(), b), name
        n = x.shape[0]
        imgs = self._imgs(n)
        xs = c8_to_nchw(x[imgs].cpu()).float()
        guard = _Guard([out])
        out = real(**A)
        torch.cuda.synchronize()
        route = "conv16/" + _lib.load().pwc_last_conv_kernel().decode() + ("/split" if split else "") + ("/f32" if out_f32 else "")
        stray = guard.stray()
        pad_ok = _pad_lanes_zero(out, cout)
        got = c8_to_nchw(out[imgs].cpu())
        if split:
            weff = split_filters(w)
            if id(A["wpacked"]) not in self.split_checked:
                self.split_checked.add(id(A["wpacked"]))
                assert bool(((weff - w.double()).abs() <= SPLIT_REL * w.double().abs() + SPLIT_ABS).all()), name
        else:
            weff = sat_half(w).double()
        # the kernel reads every lane of the input groups: pad channels meet zero filters (0 * NaN would show)
        wfull = torch.zeros((cout, xs.shape[1], 3, 3), dtype=torch.float64)
        wfull[:, :cin] = weff
        ref, s = LA.conv_ref(xs, wfull, b, stride, dil, A["leaky_slope"] is not None)
        r = half_ratio(got[:, :cout], ref, s, REL_F16, half_out=not out_f32)
        self._record("conv3x3_f16", route, x.shape, len(imgs), worst(r)[0], stray, pad_ok, layer=name)
        return out

    def _check_image_conv_s2(self, real, A):
        x, out = A["x"], A["out"]
        w, b = A["weight"].float().cpu(), A["bias"].float().cpu()
        assert torch.equal(w, self.conv1a[0]) and torch.equal(b, self.conv1a[1])
        imgs = self._imgs(x.shape[0])
        xs = x[imgs].cpu()
        guard = _Guard([out]) if out is not None else None
        out = real(**A)
        torch.cuda.synchronize()
        stray = guard.stray() if guard else 0
        ref, s = LA.conv_ref(xs, w, b, 2, 1, True)
        r = half_ratio(c8_to_nchw(out[imgs].cpu()), ref, s)
        self._record("image_conv_s2", "pyr1/image-s2", x.shape, len(imgs), worst(r)[0], stray, True)
        return out

    def _check_pyramid1_fused(self, real, A):
        x, out = A["x"], A["out"]
        layers = [(sat_half(w.float().cpu()), b.float().cpu(), s) for w, b, s in self.pyr1[id(A["packed"])]]
        imgs = self._imgs(x.shape[0])
        xs = x[imgs].cpu()
        guard = _Guard([out]) if out is not None else None
        out = real(**A)
        torch.cuda.synchronize()
        stray = guard.stray() if guard else 0
        ref, allow = pyr1_chain(xs, layers, A["leaky_slope"])
        r = bounded_ratio(c8_to_nchw(out[imgs].cpu()), ref, allow, 1.0)
        self._record("pyramid1_fused", "pyr1/fused", x.shape, len(imgs), worst(r)[0], stray, True)
        return out

    # ---- cost volume, warp, level entry --------------------------------------------------------------------------------------------
    @staticmethod
    def _corr_route(n, h, w):
        """the library's rule (pwc_corr81_c8_f16): one thread per output value below 100 workgroups of the tiled kernel"""
        below = int(os.environ.get("PWC_CORR16_DIRECT_BELOW") or 100)
        return "corr16/direct" if n * ((w + 31) // 32) * ((h + 7) // 8) < below else "corr16/tiled"

    def _check_correlation_c8(self, real, A):
        in1, in2, c, out = A["in1"], A["in2"], A["channels"], A["out"]
        assert A["corr_multiply"] == 1.0
        n, _, h, w, _ = in1.shape
        imgs = self._imgs(n)
        a = c8_to_nchw(in1[imgs].cpu())[:, :c].double()
        b = c8_to_nchw(in2[imgs].cpu())[:, :c].double()
        guard = _Guard([out]) if out is not None else None
        out = real(**A)
        torch.cuda.synchronize()
        stray = guard.stray() if guard else 0
        ref, s = corr_ref(a, b, A["normalize"], A["leaky_slope"] is not None)
        r = half_ratio(c8_to_nchw(out[imgs].cpu())[:, :81], ref, s)
        self._record("correlation_c8", self._corr_route(n, h, w), in1.shape, len(imgs), worst(r)[0], stray, _pad_lanes_zero(out, 81))
        return out

    def _check_warp_c8(self, real, A):
        x, flo, c, out = A["x"], A["flo"], A["channels"], A["out"]
        n = x.shape[0]
        imgs = self._imgs(n)
        xs = c8_to_nchw(x[imgs].cpu())[:, :c].double()
        k = A["flo_channel"]
        fs = flo[imgs, 0, :, :, k:k + 2].permute(0, 3, 1, 2).cpu().float()
        guard = _Guard([out]) if out is not None else None
        out = real(**A)
        torch.cuda.synchronize()
        stray = guard.stray() if guard else 0
        taps = warp_taps(fs, A["flow_scale"], A["align_corners"], A["mask_threshold"])
        near = near_threshold(taps, A["mask_threshold"])
        r = half_ratio(c8_to_nchw(out[imgs].cpu())[:, :c], warp_apply(xs, taps), torch.zeros(()), 0.0,
                       extra=REL_WARP * warp_apply(xs.abs(), taps), keep=(~near).unsqueeze(1))
        self._record("warp_c8", "warp16", x.shape, len(imgs), worst(r)[0], stray, _pad_lanes_zero(out, c), int(near.sum()), near.numel())
        return out

    def _entry_common(self, A, imgs, fg, c1_dst):
        """checks shared by both entry kernels: c1 copied bit for bit (every image, pad lanes included), the flow group; returns
        (ratio so far, up_flow32 of the picked images, c1 / c2 of the picked images, float64)"""
        c1, c2, c = A["c1"], A["c2"], A["channels"]
        ok = torch.equal(c1_dst.view(torch.int16), c1.view(torch.int16))
        up32 = entry_up_flow(A["flow32"][imgs, 0, :, :, 0:2].permute(0, 3, 1, 2).cpu(), A["deconv_w"].cpu(), A["deconv_b"].cpu())
        g = fg[imgs, 0].cpu()                                                          # [n,H,W,8]
        want = sat_half(up32).permute(0, 2, 3, 1)
        diff = g[..., 0:2].view(torch.int16) != want.view(torch.int16)
        nd = int(diff.sum())
        # a mismatch may only come from a tie of the fp64 restatement's double rounding: one half ulp, a handful per launch
        one_ulp = (g[..., 0:2].view(torch.int16).int() - want.view(torch.int16).int()).abs() <= 1
        ok = ok and nd <= ENTRY_DOUBLE_ROUNDING_MAX and bool(one_ulp.all())
        feat = sat_half(feat_shuffle(A["feat_phases"][imgs].cpu())).permute(0, 2, 3, 1)
        ok = ok and torch.equal(g[..., 2:4].view(torch.int16), feat.view(torch.int16)) and bool((g[..., 4:] == 0).all())
        ok = ok and bool((fg[:, 0, :, :, 4:] == 0).all())
        a = c8_to_nchw(c1[imgs].cpu())[:, :c].double()
        b = c8_to_nchw(c2[imgs].cpu())[:, :c].double()
        return (0.0 if ok else float("inf")), up32, a, b, nd

    def _check_level_entry(self, real, A):
        out, fg, c1_dst, c = A["out"], A["flow_group"], A["c1_dst"], A["channels"]
        n = out.shape[0]
        imgs = self._imgs(n)
        guard = _Guard([out, fg, c1_dst])
        out = real(**A)
        torch.cuda.synchronize()
        stray = guard.stray()
        r0, up32, a, b, nd = self._entry_common(A, imgs, fg, c1_dst)
        taps = warp_taps(up32, A["flow_scale"], A["align_corners"], A["mask_threshold"])
        near = near_threshold(taps, A["mask_threshold"])
        r = half_ratio(c8_to_nchw(out[imgs].cpu())[:, :c], warp_apply(b, taps), torch.zeros(()), 0.0,
                       extra=REL_WARP * warp_apply(b.abs(), taps), keep=(~near).unsqueeze(1))
        self._record("level_entry", "entry/two-launch", out.shape, len(imgs), max(r0, worst(r)[0]), stray,
                     _pad_lanes_zero(out, c), int(near.sum()), near.numel(), double_rounding=nd)
        return out

    def _check_level_entry_correlation(self, real, A):
        out, fg, c1_dst, c = A["out"], A["flow_group"], A["c1_dst"], A["channels"]
        assert A["corr_multiply"] == 1.0
        n, _, h, w, _ = out.shape
        imgs = self._imgs(n)
        guard = _Guard([out, fg, c1_dst])
        out = real(**A)
        torch.cuda.synchronize()
        stray = guard.stray()
        r0, up32, a, b, nd = self._entry_common(A, imgs, fg, c1_dst)
        taps = warp_taps(up32, A["flow_scale"], A["align_corners"], A["mask_threshold"])
        wref = warp_apply(b, taps)
        # the warped features are rounded to half in LDS: |half(blend) - wref| <= u|wref| + t + (1+u) REL_WARP sum|w_tap||x| = delta,
        # which reaches the cost volume as corr(|c1|, delta) (the one-ulp freedom of the rounded warp)
        delta = U16 * wref.abs() + T16 + (1 + U16) * REL_WARP * warp_apply(b.abs(), taps)
        ref, s = corr_ref(a, wref, A["normalize"], A["leaky_slope"] is not None)
        _, prop = corr_ref(a.abs(), delta, A["normalize"], False)
        near = near_threshold(taps, A["mask_threshold"])
        keep = ~(F.max_pool2d(near.double().unsqueeze(1), 9, 1, 4)[:, 0] > 0)
        r = half_ratio(c8_to_nchw(out[imgs].cpu())[:, :81], ref, s, REL_F16, extra=prop, keep=keep.unsqueeze(1))
        # bit-identical to level_entry + correlation_c8 on the same inputs (scratch outputs)
        dev = out.device
        sc1 = torch.zeros(A["c1"].shape, dtype=torch.float16, device=dev)
        sfg = torch.zeros(fg.shape, dtype=torch.float16, device=dev)
        swp = torch.zeros(A["c2"].shape, dtype=torch.float16, device=dev)
        scv = torch.zeros(out.shape, dtype=torch.float16, device=dev)
        self.real["level_entry"](A["c1"], A["c2"], A["flow32"], A["feat_phases"], A["deconv_w"], A["deconv_b"], c,
                                 c1_dst=sc1, flow_group=sfg, out=swp, flow_scale=A["flow_scale"],
                                 align_corners=A["align_corners"], mask_threshold=A["mask_threshold"])
        self.real["correlation_c8"](A["c1"], swp, c, normalize=A["normalize"], leaky_slope=A["leaky_slope"], out=scv)
        torch.cuda.synchronize()
        same = (torch.equal(scv.view(torch.int16), out.view(torch.int16)) and torch.equal(sfg.view(torch.int16), fg.view(torch.int16))
                and torch.equal(sc1.view(torch.int16), c1_dst.view(torch.int16)))
        self._record("level_entry_correlation", "entry/fused", out.shape, len(imgs), max(r0, worst(r)[0]) if same else float("inf"),
                     stray, _pad_lanes_zero(out, 81), int(near.sum()), near.numel(), double_rounding=nd)
        return out
