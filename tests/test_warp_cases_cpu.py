"""The case table of tests/warp_cases.py is held to its conditions here, on the CPU: every class a field is named for is populated
for every shape and configuration it is used with, the knife-edge share is capped or pinned, three independent statements of the
taps agree on every mask decision, and the gradient reference is held against float64 autograd and a hand-worked example."""
import numpy as np
import pytest
import torch

import launch_audit as LA
import warp_cases as WC
from oracle import pwc_oracle as O

# level_entry does not see these fields but the up-flow its deconvolution makes of them: test_entry_up_flow_* below
FAMILIES = [("warp", s) for s in WC.SHAPES_WARP] + [("c8", s) for s in WC.SHAPES_C8] + [("fused", s) for s in WC.SHAPES_FUSED]
CASES = [(fam, shape, cfg) for fam, shape in FAMILIES for cfg in WC.CONFIGS]
CASE_IDS = ["%s-%s-%s" % (fam, WC.shape_id(shape), WC.cfg_id(cfg)) for fam, shape, cfg in CASES]


def _fields(fam):
    return WC.FIELDS_FUSED if fam == "fused" else WC.FIELDS


def _hw(shape):
    return "%dx%d" % (shape[2], shape[3])


# Classes that cannot exist, by (field, class, HxW, align_corners or None for both) -> reason.  Nothing is skipped silently: a
# class missing from a field that is not listed here fails, and so does a listed class that turns out to be populated.
ABSENT = {
    ("zero", "kept", "1x8", False): "H == 1 without align_corners: iy = -0.5, the row weight is 0.5 -- the reference masks everything",
    ("zero", "kept", "6x1", False): "W == 1 without align_corners: ix = -0.5, the column weight is 0.5 -- everything is masked",
    ("border", "y0 == -1", "1x8", True): "H == 1 with align_corners: iy = (g + 1) / 2 * 0 = 0 whatever the flow",
    ("border", "x0 == -1", "6x1", True): "W == 1 with align_corners: ix = (g + 1) / 2 * 0 = 0 whatever the flow",
    ("zero", "kept", "2x2", False): "W == 2 without align_corners: ix = 2 x - 0.5 is -0.5 or 1.5, both columns half outside",
    ("zero", "kept", "6x2", False): "W == 2 without align_corners: ix = 2 x - 0.5 is -0.5 or 1.5, both columns half outside",
}
# fewer than 16 pixels: the threshold sweep cannot put four pixels on each side (one each is required instead)
TINY = 16
# W == 1 / H == 1 with align_corners: a finite flow of any size leaves ix (iy) at 0, so a wild pixel whose other coordinate is
# ordinary is KEPT there; the rule "a wild pixel is masked" holds for these shapes only where the product Inf * 0 = NaN arises
WILD_KEPT_OK = {("1x8", True), ("6x1", True)}


def _counts(name, shape, cfg):
    B, _, H, W = shape
    x0, y0, w, m64, mask, (ax1, ay1, inb) = WC.field_taps(name, shape, cfg)
    flo = WC.field(name, shape, cfg)
    c = {
        "lattice": int(((ax1 == 0) | (ay1 == 0)).sum()),
        "dyadic": int(((ax1 * 8 == torch.round(ax1 * 8)) & (ay1 * 8 == torch.round(ay1 * 8))).sum()),
        "x0 == -1": int(((x0 == -1) & mask).sum()), "x0 == W-1": int(((x0 == W - 1) & mask).sum()),
        "y0 == -1": int(((y0 == -1) & mask).sum()), "y0 == H-1": int(((y0 == H - 1) & mask).sum()),
        "kept": int(mask.sum()), "dropped": int((~mask).sum()),
        "clamp": int(((x0 == -16) | (x0 == W + 16) | (y0 == -16) | (y0 == H + 16)).sum()),
        "nonfinite": int((~torch.isfinite(flo)).any(1).sum()),
        "knife": int(WC.knife(WC.field_taps(name, shape, cfg), cfg[2]).sum()),
        "pixels": mask.numel(),
    }
    return c


def _need(name, cls, shape, cfg, count, floor=1):
    key = (name, cls, _hw(shape), cfg[1])
    if key in ABSENT:
        assert count == 0, "%s is listed as absent (%s) but has %d pixels" % (key, ABSENT[key], count)
    else:
        assert count >= floor, "%s %s %s: class '%s' has %d pixels, needs %d" % (name, WC.shape_id(shape), WC.cfg_id(cfg), cls, count, floor)


@pytest.mark.parametrize("fam,shape,cfg", CASES, ids=CASE_IDS)
def test_every_class_is_populated(fam, shape, cfg):
    B, _, H, W = shape
    align, thr = cfg[1], cfg[2]
    for name in _fields(fam):
        c = _counts(name, shape, cfg)
        print("%-11s %s" % (name, " ".join("%s=%d" % kv for kv in c.items())))
        flo = WC.field(name, shape, cfg)
        assert flo.dtype == torch.float32 and tuple(flo.shape) == (B, 2, H, W)
        t = WC.field_taps(name, shape, cfg)
        if name == "zero":
            assert not bool(flo.any())
            if align:
                # the identity: every pixel kept; x -> 2 x / (W - 1) - 1 -> x is not exact in float32 for every W, so some sample
                # points land an ulp beside their pixel (on either side: the cell left of it with a fraction just under 1 is one
                # of the cases the kernels must get right) -- most land on it
                assert c["kept"] == c["pixels"] and c["lattice"] >= c["pixels"] // 2
                ix, iy = WC.sample_coords(t)
                assert float((ix - ix.round()).abs().max()) < 1e-5 and float((iy - iy.round()).abs().max()) < 1e-5
            else:
                _need(name, "kept", shape, cfg, c["kept"])
        elif name == "integer":
            _need(name, "lattice", shape, cfg, c["lattice"], floor=min(c["pixels"], 4))
        elif name == "eighths":
            _need(name, "dyadic", shape, cfg, c["dyadic"], floor=min(c["pixels"], 4) if align else 1)
        elif name == "border":
            for cls in ("x0 == -1", "x0 == W-1", "y0 == -1", "y0 == H-1"):
                _need(name, cls, shape, cfg, c[cls])
            _need(name, "lattice", shape, cfg, c["lattice"])
        elif name == "threshold":
            floor = 4 if c["pixels"] >= TINY else 1
            _need(name, "kept", shape, cfg, c["kept"], floor)
            _need(name, "dropped", shape, cfg, c["dropped"], floor)
            # the float64 mask sum crosses thr inside the field
            assert float(t[3].min()) < thr < float(t[3][t[3] < 1].max() if bool((t[3] < 1).any()) else 1.0) or c["pixels"] < TINY
        elif name == "far":
            _need(name, "clamp", shape, cfg, c["clamp"])
        elif name == "wild":
            _need(name, "nonfinite", shape, cfg, c["nonfinite"])
            wild = WC.wild_pixels(B, H, W)
            kept_wild = int((wild & t[4]).sum())
            if (_hw(shape), align) in WILD_KEPT_OK:
                nan_px = torch.isnan(flo).any(1) | torch.isinf(flo[:, 0 if W == 1 else 1])
                assert not bool((nan_px & t[4]).any())
            else:
                assert kept_wild == 0, "%d wild pixels are kept" % kept_wild
        elif name == "converge":
            assert c["kept"] == c["pixels"]
            for b in range(B):
                cells = {(int(a), int(bb)) for a, bb in zip(t[0][b].flatten(), t[1][b].flatten())}
                assert cells == set(WC.converge_targets(B, H, W)[b]), cells
        elif name.startswith("tile_centre"):
            centres = [(b, r, cc) for b in range(B) for (r, cc) in WC.tile_centres(H, W)]
            assert len(centres) >= 2
            x0, y0, m64, mask = t[0], t[1], t[3], t[4]
            if name == "tile_centre":
                ordinary = WC.field("wild", shape, cfg)                          # its even squares are the ordinary flow
                placed = [(b, r, cc) for (b, r, cc) in centres if not bool((flo[b, :, r, cc].abs() < 1e29).all())]
                plain = [(b, r, cc) for (b, r, cc) in centres if (r + cc) % 2 == 0 and torch.equal(flo[b, :, r, cc], ordinary[b, :, r, cc])
                         or (r + cc) % 2 == 1 and bool((flo[b, :, r, cc].abs() < 1e29).all())]
                assert len(placed) >= 1 and len(plain) >= 1 and len(placed) + len(plain) == len(centres)      # both kinds of tile
                assert not bool(torch.isfinite(flo[placed[0][0], :, placed[0][1], placed[0][2]]).all())       # the first one is Inf
                for (b, r, cc) in plain:                                         # an ordinary centre has wild neighbours
                    nb = flo[b, :, max(r - 1, 0):r + 2, max(cc - 1, 0):cc + 2]
                    assert not bool((nb.abs() < 1e29).all())
            elif name == "tile_centre_far":
                # every centre beyond the taps' clamp; both 17 px and 1000 px (beyond the window origin's clamp at 64) occur
                out = [int(x0[c] in (-16, W + 16)) + int(y0[c] in (-16, H + 16)) for c in centres]
                reach = [float((flo[b, :, r, cc] * cfg[0]).abs().max()) for (b, r, cc) in centres]
                assert all(o == 1 for o in out), out
                assert min(reach) < 100 < 500 < max(reach), reach
                assert not any(bool(mask[c]) for c in centres)
            else:
                kept = [c for c in centres if bool(mask[c])]
                assert len(kept) >= 1 and len(centres) - len(kept) >= 1, (len(kept), len(centres))
                assert all(abs(float(m64[c]) - thr) < 0.75 * (1 - thr) for c in centres)


@pytest.mark.parametrize("fam,shape,cfg", CASES, ids=CASE_IDS)
def test_knife_edge_share_is_capped_or_pinned(fam, shape, cfg):
    """Pixels whose float64 mask sum lies within MASK_EPS of the threshold: at most MASK_EXCLUDED_MAX of a field, except for the
    fields built on the edge (threshold, border; tile_centre carries threshold values on its window pixels), whose count is a
    constant of the table."""
    B, _, H, W = shape
    for name in _fields(fam):
        t = WC.field_taps(name, shape, cfg)
        n = int(WC.knife(t, cfg[2]).sum())
        if name in WC.ON_THE_EDGE:
            assert n == WC.KNIFE_COUNTS[(name, "%dx%dx%d" % (B, H, W), WC.cfg_id(cfg))], (name, n)
        else:
            assert n <= LA.MASK_EXCLUDED_MAX * t[4].numel(), (name, n)


def _scalar_taps(u, v, x, y, H, W, scale, align, thr):
    """make_taps of pwc_warp_taps.h for one pixel, every operation one numpy.float32 operation"""
    f = np.float32
    with np.errstate(all="ignore"):
        px, py = f(x) + f(u) * f(scale), f(y) + f(v) * f(scale)
        gx = f(2.0) * px / f(max(W - 1, 1)) - f(1.0)
        gy = f(2.0) * py / f(max(H - 1, 1)) - f(1.0)
        if align:
            ix = (gx + f(1.0)) / f(2.0) * f(W - 1)
            iy = (gy + f(1.0)) / f(2.0) * f(H - 1)
        else:
            ix = ((gx + f(1.0)) * f(W) - f(1.0)) / f(2.0)
            iy = ((gy + f(1.0)) * f(H) - f(1.0)) / f(2.0)
        # fminf(fmaxf(x, lo), hi): a NaN operand loses against the number
        ix = f(-16.0) if np.isnan(ix) else min(max(ix, f(-16.0)), f(W) + f(16.0))
        iy = f(-16.0) if np.isnan(iy) else min(max(iy, f(-16.0)), f(H) + f(16.0))
        fx, fy = np.floor(ix), np.floor(iy)
        x0, y0 = int(fx), int(fy)
        ax1, ay1 = f(ix - fx), f(iy - fy)
        ax0, ay0 = f(1.0) - ax1, f(1.0) - ay1
        vx0, vx1 = 0 <= x0 < W, 0 <= x0 + 1 < W
        vy0, vy1 = 0 <= y0 < H, 0 <= y0 + 1 < H
        w = [ay0 * ax0 if (vx0 and vy0) else f(0), ay0 * ax1 if (vx1 and vy0) else f(0),
             ay1 * ax0 if (vx0 and vy1) else f(0), ay1 * ax1 if (vx1 and vy1) else f(0)]
        msum = f(f(f(w[0] + w[1]) + w[2]) + w[3])
        keep = bool(msum >= f(thr))
    if not keep:
        w = [f(0)] * 4
    return x0, y0, w, keep


@pytest.mark.parametrize("fam,shape,cfg", CASES, ids=CASE_IDS)
def test_three_statements_agree_on_the_mask(fam, shape, cfg):
    """launch_audit.warp_taps, oracle.pwc_oracle.warp of a ones tensor (its own float32 statement, no clamp) and a scalar
    numpy.float32 loop written out from pwc_warp_taps.h agree on EVERY mask decision of every field -- the loop on a handful of
    pixels per field, cells and weights included."""
    B, _, H, W = shape
    s, align, thr = cfg
    for name in _fields(fam):
        flo = WC.field(name, shape, cfg)
        x0, y0, w, m64, mask, _ = WC.field_taps(name, shape, cfg)
        raw = LA.warp_taps(flo, s, align, thr)
        assert torch.equal(raw[4], mask) and all(torch.equal(a, b) for a, b in zip(raw[2], w))
        ones = O.warp(torch.ones(B, 1, H, W), flo * s, align_corners=align, mask_threshold=thr)[:, 0]
        assert torch.equal(ones > 0, mask), "%s: oracle and warp_taps differ at %s" % (name, torch.nonzero((ones > 0) != mask)[:4].tolist())
        npx = B * H * W
        picks = sorted(set(int(i) for i in torch.linspace(0, npx - 1, 24)))
        knife = torch.nonzero(WC.knife(WC.field_taps(name, shape, cfg), thr).flatten()).flatten()[:8].tolist()
        for i in picks + knife:
            b, r = divmod(i, H * W)
            y, x = divmod(r, W)
            sx0, sy0, sw, keep = _scalar_taps(float(flo[b, 0, y, x]), float(flo[b, 1, y, x]), x, y, H, W, s, align, thr)
            assert keep == bool(mask[b, y, x]), (name, b, y, x)
            assert (sx0, sy0) == (int(x0[b, y, x]), int(y0[b, y, x])), (name, b, y, x)
            assert [float(v) for v in sw] == [float(t[b, y, x]) for t in w], (name, b, y, x)


def test_nan_sample_coordinate_has_no_valid_tap():
    """The non-finite rule, once: a pixel whose sample coordinate is NaN (a NaN flow, Inf * 0 at W == 1) has no valid tap.
    warp_taps implements it in its weights and mask although torch.clamp propagates the NaN; warp_cases.nan_rule fills in the cell
    the device computes, (-16, fraction 0)."""
    nan, inf = float("nan"), float("inf")
    for cfg in WC.CONFIGS:
        flo = torch.zeros(1, 2, 3, 4)
        flo[0, 0, 0, 0] = nan
        flo[0, 1, 0, 1] = nan
        flo[0, :, 1, 1] = nan
        flo[0, 0, 2, 2] = inf
        flo[0, 1, 2, 3] = -inf
        raw = LA.warp_taps(flo, *cfg)
        t = WC.taps(flo, cfg)
        bad = torch.isnan(flo).any(1)
        assert not bool(raw[4][bad].any()) and all(not bool(w[bad].any()) for w in raw[2]) and not bool(raw[3][bad].any())
        assert bool((t[0][0, 0, 0] == -16) and (t[1][0, 0, 1] == -16) and (t[0][0, 1, 1] == -16) and (t[1][0, 1, 1] == -16))
        assert not bool(torch.isnan(t[5][0]).any() or torch.isnan(t[5][1]).any())
        assert int(t[0][0, 2, 2]) == 4 + 16 and int(t[1][0, 2, 3]) == -16 and not bool(t[4][0, 2, 2:].any())
        for (y, x) in ((0, 0), (0, 1), (1, 1), (2, 2), (2, 3)):
            sx0, sy0, sw, keep = _scalar_taps(float(flo[0, 0, y, x]), float(flo[0, 1, y, x]), x, y, 3, 4, *cfg)
            assert not keep and (sx0, sy0) == (int(t[0][0, y, x]), int(t[1][0, y, x]))
    # Inf * 0 at W == 1 with align_corners
    one = torch.zeros(1, 2, 2, 1)
    one[0, 0, 1, 0] = inf
    t = WC.taps(one, (1.0, True, 0.9999))
    assert bool(t[4][0, 0, 0]) and not bool(t[4][0, 1, 0]) and int(t[0][0, 1, 0]) == -16


def test_grads_hand_worked_on_the_lattice():
    """2x2 map, zero flow, align_corners: every sample point on its own pixel.  One-sided: d/d ix is the slope toward the pixel to
    the right (the cell of floor(ix)), and the tap beyond the last column / row is the zero padding."""
    x = torch.tensor([[[[1.0, 2.0], [3.0, 5.0]]]])
    go = torch.tensor([[[[1.0, 10.0], [100.0, 1000.0]]]])
    cfg = (2.0, True, 0.9999)
    gx, gf, sx, sf = WC.grads(x, WC.taps(torch.zeros(1, 2, 2, 2), cfg), go, cfg)
    assert torch.equal(gx, go.double()) and torch.equal(sx, go.double())
    #                       d/du = scale * go * (right - own)                       d/dv = scale * go * (below - own)
    want = torch.tensor([[[[2 * 1 * (2 - 1), 2 * 10 * (0 - 2)], [2 * 100 * (5 - 3), 2 * 1000 * (0 - 5)]],
                          [[2 * 1 * (3 - 1), 2 * 10 * (5 - 2)], [2 * 100 * (0 - 3), 2 * 1000 * (0 - 5)]]]], dtype=torch.float64)
    assert torch.equal(gf, want)
    assert torch.equal(sf[0, 0], torch.tensor([[2 * 1 * 3.0, 2 * 10 * 2.0], [2 * 100 * 8.0, 2 * 1000 * 5.0]], dtype=torch.float64))
    # without align_corners the same map has the gain W / (W - 1) = 2, and a masked pixel has no gradient
    cfg = (1.0, False, 0.9999)
    flo = WC.flow_for(torch.tensor([[[0.0, 1.0], [0.0, 5.0]]], dtype=torch.float64), torch.tensor([[[0.0, 0.0], [1.0, 1.0]]], dtype=torch.float64), cfg)
    t = WC.taps(flo, cfg)
    assert t[4].tolist() == [[[True, True], [True, False]]] and bool((t[5][0] == 0).all() and (t[5][1] == 0).all())
    gx, gf, _, _ = WC.grads(x, t, go, cfg)
    assert torch.equal(gf[0, 0], torch.tensor([[2.0 * (2 - 1), 2.0 * 10 * (0 - 2)], [2.0 * 100 * (5 - 3), 0.0]], dtype=torch.float64))
    assert torch.equal(gx[0, 0], torch.tensor([[1.0, 10.0], [100.0, 0.0]], dtype=torch.float64))


@pytest.mark.parametrize("cfg", WC.CONFIGS, ids=WC.cfg_id)
def test_grads_match_float64_autograd_of_the_oracle(cfg):
    """Away from the tap boundaries and the threshold (the pixels test_gpu_train._away_from_edges would leave alone) float32 and
    float64 pick the same cell, and grads() is the derivative autograd takes through oracle.pwc_oracle.warp, up to the float32
    rounding of the sample coordinate that grads() shares with the kernels."""
    s, align, thr = cfg
    shape = (2, 9, 13, 21)
    B, C, H, W = shape
    x = WC.signed(shape, 11)
    go = WC.signed(shape, 12)
    flo = WC.signed((B, 2, H, W), 13) * 3
    t = WC.taps(flo, cfg)
    ix, iy = WC.sample_coords(t)
    calm = ((ix - ix.round()).abs() > 1e-4) & ((iy - iy.round()).abs() > 1e-4) & ((t[3] - thr).abs() > 1e-5)
    assert int(calm.sum()) > 0.9 * calm.numel()
    go = go * calm.unsqueeze(1)
    a = x.double().requires_grad_(True)
    f = flo.double().requires_grad_(True)
    O.warp(a, f * s, align_corners=align, mask_threshold=thr).backward(go.double())
    gx, gf, sx, sf = WC.grads(x, t, go, cfg)
    assert int(t[4].sum()) > 100 and bool(gf.abs().sum() > 0)
    # The two differ by the float32 rounding of the sample coordinate only: eight roundings of numbers below W + 8 on the way
    # (x + s u, 2 px / (W - 1), - 1, + 1, * W, - 1 and the flow's own product), d <= 8 * 2^-24 * (W + 8).  A weight moves by at
    # most 2 d; the bilinear slope by d times the sum of the four taps' magnitudes.
    d = 8 * 2.0 ** -24 * (max(H, W) + 8)
    u = torch.arange(W, dtype=torch.float64).view(1, 1, W) + flo[:, 0].double() * s
    v = torch.arange(H, dtype=torch.float64).view(1, H, 1) + flo[:, 1].double() * s
    ix64, iy64 = (u, v) if align else (u * W / (W - 1) - 0.5, v * H / (H - 1) - 0.5)
    inside = (ix64.abs() < W + 8) & (iy64.abs() < H + 8)
    assert float(((ix - ix64).abs() * inside).max()) <= d and float(((iy - iy64).abs() * inside).max()) <= d
    ones = (t[0], t[1], [(k & t[4]).float() for k in t[5][2]], t[3], t[4], t[5])                # every live tap with weight 1
    half = (t[0], t[1], t[2], t[3], t[4], (torch.full_like(t[5][0], 0.5), torch.full_like(t[5][1], 0.5), t[5][2]))
    all_go = WC.grads(x, ones, go, cfg)[2]
    all_taps = 2 * WC.grads(x, half, go, cfg)[3]                                               # gain * sum |go| (|s00| + ... + |s11|)
    assert bool(((gx - a.grad).abs() <= 2 * d * all_go + 1e-6 * sx).all())
    assert bool(((gf - f.grad).abs() <= d * all_taps + 1e-6 * sf).all())
    assert not bool(gf[~t[4].unsqueeze(1).expand_as(gf)].any())


# Classes the up-flow of an entry shape cannot hold, (field, class, HxW, align_corners) -> reason; same rule as ABSENT
SMALL = "6x2 is three 2x2 blocks, so three constructed pixels: they carry combinations 0, 5 and 10 of the border cycle -- the left side " \
        "one ulp outside, the top side on the pixel, the right side one ulp inside; 14x22 holds all four classes"
ENTRY_ABSENT = {
    ("zero", "kept", "6x2", False): ABSENT[("zero", "kept", "6x2", False)],
}
for _align in (False, True):
    for _cls in ("x0 == W-1", "y0 == -1", "y0 == H-1"):
        ENTRY_ABSENT[("border", _cls, "6x2", _align)] = SMALL


def _entry_need(name, cls, shape, cfg, count, floor=1):
    key = (name, cls, _hw(shape), cfg[1])
    if key in ENTRY_ABSENT:
        assert count == 0, "%s is listed as absent (%s) but has %d pixels" % (key, ENTRY_ABSENT[key], count)
    else:
        assert count >= floor, "entry %s %s %s: class '%s' has %d pixels, needs %d" % (name, WC.shape_id(shape), WC.cfg_id(cfg), cls, count, floor)


@pytest.mark.parametrize("shape", WC.SHAPES_ENTRY, ids=WC.shape_id)
@pytest.mark.parametrize("cfg", WC.CONFIGS, ids=WC.cfg_id)
def test_entry_up_flow_is_exact_and_keeps_its_classes(shape, cfg):
    """level_entry warps by deconvL(flow): with the identity-phase filter the up-flow is the half-resolution field, pixel for pixel
    of each 2x2 block, bit for bit (conv_transpose2d in float32: every other product is 0 * finite).  The classes are asserted on
    THAT tensor -- the one the kernel sees -- for every field and both shapes; what three blocks cannot hold is listed in
    ENTRY_ABSENT.  The three statements of the taps agree on its masks, and its knife-edge counts are capped or pinned."""
    B, _, H, W = shape
    s, align, thr = cfg
    dw, db = WC.identity_deconv()
    blocks = B * (H // 2) * (W // 2)
    for name in WC.FIELDS:
        low, up = WC.entry_flow(name, shape, cfg)
        assert bool(torch.isfinite(low).all())
        assert torch.equal(torch.nn.functional.conv_transpose2d(low, dw, db, stride=2, padding=1), up)
        assert torch.equal(up[:, :, 0::2, 0::2], low) and torch.equal(up[:, :, 1::2, 1::2], low)
        t = WC.taps(up, cfg)
        x0, y0, w, m64, mask, (ax1, ay1, inb) = t
        ones = O.warp(torch.ones(B, 1, H, W), up * s, align_corners=align, mask_threshold=thr)[:, 0]
        assert torch.equal(ones > 0, mask), name
        knife = int(WC.knife(t, thr).sum())
        if name in WC.ON_THE_EDGE:
            assert knife == WC.ENTRY_KNIFE_COUNTS[(name, "%dx%dx%d" % (B, H, W), WC.cfg_id(cfg))], (name, knife)
        else:
            assert knife <= LA.MASK_EXCLUDED_MAX * mask.numel(), (name, knife)
        huge = (up.abs() > 1e29).any(1)
        targets = WC.converge_targets(B, H, W)
        on_target = sum(int(((x0[b] == p[0]) & (y0[b] == p[1])).sum() + ((x0[b] == q[0]) & (y0[b] == q[1])).sum()) for b, (p, q) in enumerate(targets))
        c = {"lattice": int(((ax1 == 0) | (ay1 == 0)).sum()),
             "dyadic": int(((ax1 * 8 == torch.round(ax1 * 8)) & (ay1 * 8 == torch.round(ay1 * 8))).sum()),
             "x0 == -1": int(((x0 == -1) & mask).sum()), "x0 == W-1": int(((x0 == W - 1) & mask).sum()),
             "y0 == -1": int(((y0 == -1) & mask).sum()), "y0 == H-1": int(((y0 == H - 1) & mask).sum()), "kept": int(mask.sum()),
             "dropped": int((~mask).sum()), "clamp": int(((x0 == -16) | (x0 == W + 16) | (y0 == -16) | (y0 == H + 16)).sum()),
             "huge": int(huge.sum()), "on target": on_target, "pixels": mask.numel()}
        print("%-11s %s" % (name, " ".join("%s=%d" % kv for kv in c.items())))
        need = lambda cls, floor=1: _entry_need(name, cls, shape, cfg, c[cls], floor)      # noqa: E731
        if name == "zero":
            assert not bool(up.any())
            if align:
                assert c["kept"] == c["pixels"] and c["lattice"] >= c["pixels"] // 2
            else:
                need("kept")
        elif name == "integer":
            need("lattice", min(blocks, 4))
            need("kept")
        elif name == "eighths":
            need("dyadic")
            need("kept")
        elif name == "border":
            for cls in ("x0 == -1", "x0 == W-1", "y0 == -1", "y0 == H-1", "lattice"):
                need(cls)
        elif name == "threshold":
            floor = 4 if blocks >= TINY else 1
            need("kept", floor)
            need("dropped", floor)
        elif name == "far":
            need("clamp")
            assert c["kept"] == 0
        elif name == "wild":
            need("huge")
            assert not bool((huge & mask).any()) and not bool(torch.isnan(up).any() or torch.isinf(up).any())
        elif name == "converge":
            need("on target", blocks)                       # the constructed pixel of every block samples one of the two sources
            need("kept", blocks)


@pytest.mark.parametrize("shape", [(2, 9, 13, 20), (2, 9, 13, 21)], ids=WC.shape_id)
@pytest.mark.parametrize("cfg", WC.CONFIGS, ids=WC.cfg_id)
def test_half_storage_fields_hold_what_a_half_flow_can(shape, cfg):
    """The fields of the fp16-storage and c8 tests (field(half=True)) are steered over HALF flows.  With align_corners (ix = x + s u)
    a pixel near a side reaches it with a small flow, which a half resolves finely: both sides of the threshold and all four border
    classes stay populated.  Without it the map stretches by W / (W - 1), so pixel x needs a flow of about x / (W - 1) px to stay
    in place; its half spacing is coarser than the 1e-4 px band of the threshold field, whose sample points then all land outside
    it (everything dropped) -- listed here, not skipped: make_taps8 meets the knife edge of that configuration through level_entry."""
    B, _, H, W = shape
    s, align, thr = cfg
    for name in WC.FIELDS:
        flo = WC.field(name, shape, cfg, half=True)
        assert torch.equal(flo, flo.half().float()) or name == "wild"                 # (NaN != NaN)
        x0, y0, w, m64, mask, (ax1, ay1, inb) = WC.taps(flo, cfg)
        ones = O.warp(torch.ones(B, 1, H, W), flo * s, align_corners=align, mask_threshold=thr)[:, 0]
        assert torch.equal(ones > 0, mask), name
        sides = [int(((x0 == -1) & mask).sum()), int(((x0 == W - 1) & mask).sum()), int(((y0 == -1) & mask).sum()), int(((y0 == H - 1) & mask).sum())]
        print("%-10s lattice=%d sides=%s kept=%d dropped=%d" % (name, int(((ax1 == 0) | (ay1 == 0)).sum()), sides, int(mask.sum()), int((~mask).sum())))
        if name == "threshold":
            if align:
                assert int(mask.sum()) >= 4 and int((~mask).sum()) >= 4 and min(sides) >= 1
            else:
                assert int(mask.sum()) == 0
        elif name == "border":
            assert min(sides) >= 1 if align else max(sides) == 0
        elif name == "integer":
            assert int(((ax1 == 0) | (ay1 == 0)).sum()) >= 4
        elif name == "wild":
            assert not bool((WC.wild_pixels(B, H, W) & mask).any())
        elif name == "converge":
            assert bool(mask.all())
