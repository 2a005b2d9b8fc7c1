"""Constructed flow fields and float64 references for the warp family (tests/test_warp_cases_cpu.py holds the table to its
conditions on the CPU, tests/test_gpu_warp_edges.py runs the kernels on it).

The coordinate, tap and mask arithmetic of PWCDCNet.warp (PWCNet.py:141-177) is stated five times on the device (make_taps,
make_taps8, the inline copies of warp_bwd_kernel and warp_corr81_bwd_kernel, window_origin_from).  With -ffp-contract=off and
correctly rounded fp32 division it is a fixed list of single-rounded float32 operations, which launch_audit.warp_taps restates on
the CPU: every mask bit and every tap weight is decided there.  The fields below put the sample points where those statements can
differ: on the lattice, on the image border, on the mask threshold, at the clamp and at non-finite flows.

Every field is built IN SAMPLE COORDINATES: the wanted (ix, iy) is chosen in float64, the kernel's map (align_corners or not, the
division by flow_scale) is inverted, and the flow is rounded to float32 -- then steered by a few float32 steps to the value whose
float32 sample coordinate lies closest to the wanted one (built in pixel coordinates, an align_corners=False field lands on one
side of the threshold everywhere).
"""
import os
import re

import numpy as np
import torch

import launch_audit as LA

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (flow_scale, align_corners, mask_threshold)
CONFIGS = [(1.25, False, 0.9999), (2.5, True, 0.999), (1.0, True, 0.9999)]


def cfg_id(cfg):
    return "s%g-a%d-t%g" % (cfg[0], int(cfg[1]), cfg[2])


# the smallest shapes at which each path is taken
SHAPES_WARP = [(2, 9, 13, 20),      # ragged channel block of 8, W % 4 == 0: vector stores
               (2, 9, 13, 21),      # ragged last quad: scalar stores
               (1, 3, 1, 8),        # H == 1
               (1, 3, 6, 1),        # W == 1
               (1, 8, 2, 2)]        # smallest map with an interior
SHAPES_C8 = [(2, 21, 13, 21), (1, 8, 1, 8), (1, 16, 6, 2)]
SHAPES_ENTRY = [(1, 16, 6, 2), (2, 21, 14, 22)]          # level_entry needs even sizes
SHAPES_FUSED = [(2, 32, 20, 72),    # more than one tile each way, ragged in both; C = 32: the window route
                (1, 13, 11, 40),    # ragged channel chunk: the r2 route
                (1, 8, 9, 4)]       # one column of quads narrower than a tile

FIELDS = ("zero", "integer", "eighths", "border", "threshold", "far", "wild", "converge")
FIELDS_FUSED = FIELDS + ("tile_centre", "tile_centre_far", "tile_centre_thr")

WILD_VALUES = (1e30, -1e30, 3e38, -3e38, float("inf"), -float("inf"), float("nan"))
# (u, v) of the wild pixels, cycled over the checkerboard: each value in u, in v, in both; Inf against -Inf; None = ordinary
WILD_PAIRS = tuple([(a, None) for a in WILD_VALUES] + [(None, a) for a in WILD_VALUES] + [(a, a) for a in WILD_VALUES]
                   + [(float("inf"), -float("inf")), (-float("inf"), float("inf")), (float("nan"), 1e30)])


def shape_id(shape):
    return "x".join(str(s) for s in shape)


def fused_tile():
    """(rows, columns) of the fused warp + correlation kernels' tile, and the (row, column) inside it of the pixel whose flow places
    the LDS window (window_centre), read from pwc_corr_pipe.hip."""
    src = open(os.path.join(REPO, "opticalflow_amd", "csrc", "pwc_corr_pipe.hip")).read()
    found = [re.search(pat, src) for pat in (r"constexpr int kTH = (\d+)", r"kTG = (\d+)", r"constexpr int kPX = (\d+)",
                                             r"c\.gxc = min\(t\.x0 \+ (\d+), a\.W - 1\);\s*c\.gyc = min\(t\.y0 \+ (\d+), a\.H - 1\)")]
    assert all(found), "tests/warp_cases.py reads kTH, kTG, kPX and window_centre's `c.gxc = min(t.x0 + N, a.W - 1); c.gyc = " \
                       "min(t.y0 + M, a.H - 1)` from opticalflow_amd/csrc/pwc_corr_pipe.hip and no longer finds them: restate fused_tile()"
    th, tg, px, m = int(found[0].group(1)), int(found[1].group(1)), int(found[2].group(1)), found[3]
    return (th, tg * px), (int(m.group(2)), int(m.group(1)))


# ---- the kernel's map and its inverse ------------------------------------------------------------------------------------------
def taps(flo, cfg):
    """launch_audit.warp_taps for a configuration, with the non-finite rule applied to the items torch leaves undefined."""
    return nan_rule(LA.warp_taps(flo, cfg[0], cfg[1], cfg[2]))


def nan_rule(t):
    """A pixel whose sample coordinate is NaN has no valid tap: fminf(fmaxf(NaN, -16), .) is -16 on the device (and !(x > lo) in
    window_origin_from).  torch.clamp propagates the NaN instead, which leaves warp_taps' weights and mask right (no tap of an
    undefined column is in bounds) but its cell index and fraction undefined: they are set to the device's (-16, 0) here."""
    x0, y0, w, m64, mask, (ax1, ay1, inb) = t
    nx, ny = torch.isnan(ax1), torch.isnan(ay1)
    x0 = torch.where(nx, torch.full_like(x0, -16), x0)
    y0 = torch.where(ny, torch.full_like(y0, -16), y0)
    ax1 = torch.where(nx, torch.zeros_like(ax1), ax1)
    ay1 = torch.where(ny, torch.zeros_like(ay1), ay1)
    return x0, y0, w, m64, mask, (ax1, ay1, inb)


def sample_coords(t):
    """float64 (ix, iy) after the clamp, exactly: ix - floor(ix) is exact in float32"""
    return t[0].double() + t[5][0].double(), t[1].double() + t[5][1].double()


def _invert(ix, iy, cfg):
    """float64 flow [B,2,H,W] whose sample point is (ix, iy) [B,H,W] in exact arithmetic"""
    s, align, _ = cfg
    B, H, W = ix.shape
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1)
    if align:                                                   # ix = px (W > 1); W == 1: ix = 0 whatever the flow
        px, py = ix, iy
    else:                                                       # ix = px * W / max(W - 1, 1) - 0.5
        px, py = (ix + 0.5) * max(W - 1, 1) / W, (iy + 0.5) * max(H - 1, 1) / H
    return torch.stack([(px - xs) / s, (py - ys) / s], 1)


_HALF = [False]        # set while a field is built for half-precision storage (field(..., half=True))


def _store(f64):
    """the float32 value of a float64 flow as the tensor will hold it: rounded to float32, or to half"""
    return f64.half().float() if _HALF[0] else f64.float()


def flow_for(ix, iy, cfg):
    """float32 flow whose FLOAT32 sample point is as close to (ix, iy) as a float32 flow gets, inside the target's own cell where one
    is in reach: the rounded inverse and neighbours from a quarter of the target's float32 spacing to 16 spacings away are run
    through warp_taps; per pixel and axis the closest one with floor(got) == floor(wanted) is kept, else the closest.  (One ulp
    outside pixel 0 is not in reach of align_corners=True: g + 1 has the spacing of 1.0 there, the nearest negative ix is
    -2^-24 (W - 1).)"""
    f64 = _invert(ix, iy, cfg)
    best = _store(f64)
    s = cfg[0]
    B, H, W = ix.shape
    gain = (1.0, 1.0) if cfg[1] else (W / max(W - 1, 1), H / max(H - 1, 1))
    want = torch.stack([ix, iy], 1)
    spacing = torch.from_numpy(np.spacing(np.maximum(np.abs(want.float().numpy()), 1.0).astype(np.float32))).double()
    step = spacing / 4
    step[:, 0] /= s * gain[0]
    step[:, 1] /= s * gain[1]
    own = np.spacing(np.abs(best.numpy()).astype(np.float16)).astype(np.float64) if _HALF[0] else np.spacing(np.abs(best.numpy()))
    step = torch.maximum(step, torch.from_numpy(own).double())                                    # never less than the flow's own ulp
    err = torch.full_like(want, float("inf"))
    reach = list(range(0, 7)) + [8, 12, 16, 24, 32, 48, 64]
    for j in sorted(set(reach + [-r for r in reach]), key=abs):
        cand = _store(f64 + j * step)
        got = torch.stack(sample_coords(taps(cand, cfg)), 1)
        e = (got - want).abs() + 1.0e3 * (torch.floor(got) != torch.floor(want)).double()
        better = e < err
        best = torch.where(better, cand, best)
        err = torch.where(better, e, err)
    return best.contiguous()


def _grid(B, H, W):
    xs = torch.arange(W, dtype=torch.float64).view(1, 1, W).expand(B, H, W).clone()
    ys = torch.arange(H, dtype=torch.float64).view(1, H, 1).expand(B, H, W).clone()
    return xs, ys


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _ulp(v, direction):
    """float32 neighbour of v (as float64) one step toward +-inf; around 0 the step is that of 1.0 (2^-23): a sample coordinate
    comes out of sums and products of numbers near 1, it does not reach the subnormals"""
    if v == 0.0:
        return float(direction) * float(np.spacing(np.float32(1.0)))
    return float(np.nextafter(np.float32(v), np.float32(direction * np.inf)))


def _interior(n, g):
    """an ordinary coordinate of an axis of n pixels: a multiple of 1/8 at least 1/4 inside (0 for n == 1)"""
    if n < 2:
        return 0.0
    k = int(torch.randint(2, 8 * (n - 1) - 1, (1,), generator=g))
    return k / 8.0


# ---- the fields ------------------------------------------------------------------------------------------------------------------
def f_zero(B, H, W, cfg, seed=0):
    return torch.zeros(B, 2, H, W)


def f_integer(B, H, W, cfg, seed=1):
    xs, ys = _grid(B, H, W)
    g = _gen(seed)
    r = min(3, max(min(H, W) - 1, 1))                           # up to 3 px, 1 px on the maps of one or two rows / columns
    dx = torch.randint(-r, r + 1, (B, H, W), generator=g).double()
    dy = torch.randint(-r, r + 1, (B, H, W), generator=g).double()
    return flow_for(xs + dx, ys + dy, cfg)


def f_eighths(B, H, W, cfg, seed=2):
    xs, ys = _grid(B, H, W)
    g = _gen(seed)
    r = min(24, 4 * max(min(H, W) - 1, 1))                      # up to 3 px, half a pixel on the maps of one or two rows / columns
    dx = torch.randint(-r, r + 1, (B, H, W), generator=g).double() / 8
    dy = torch.randint(-r, r + 1, (B, H, W), generator=g).double() / 8
    return flow_for(xs + dx, ys + dy, cfg)


def _edge_values(n):
    """[(coordinate, which)]: exactly on, one ulp inside and one ulp outside the first and the last pixel of an axis"""
    lo, hi = 0.0, float(n - 1)
    return [(_ulp(lo, -1), "lo_out"), (hi, "hi_on"), (lo, "lo_on"), (_ulp(hi, +1), "hi_out"), (_ulp(lo, +1), "lo_in"), (_ulp(hi, -1), "hi_in")]


def f_border(B, H, W, cfg, seed=3):
    """sample points at exactly 0, W-1, H-1 and one float32 ulp inside / outside them: the four sides (other coordinate ordinary),
    then the four corners with every pair of the three variants"""
    g = _gen(seed)
    ex, ey = _edge_values(W), _edge_values(H)
    combos = []
    for k in range(6):                                         # interleaved so that the first four pixels touch all four sides
        combos.append((ex[k][0], None))
        combos.append((None, ey[k][0]))
    for a in ex:
        for b in ey:
            combos.append((a[0], b[0]))
    ix, iy = _grid(B, H, W)
    n = 0
    for b in range(B):
        for y in range(H):
            for x in range(W):
                cx, cy = combos[(n + 5 * b) % len(combos)]
                ix[b, y, x] = _interior(W, g) if cx is None else cx
                iy[b, y, x] = _interior(H, g) if cy is None else cy
                n += 1
    return flow_for(ix, iy, cfg)


def f_threshold(B, H, W, cfg, seed=4):
    """sample points d outside each side, d sweeping [0.5, 1.5] (1 - thr) with the other coordinate on a pixel (weight exactly 1),
    and a corner where both partial weights are below 1 and their product crosses thr"""
    thr = cfg[2]
    npx = B * H * W
    ix, iy = _grid(B, H, W)
    g = _gen(seed)
    n = 0
    for b in range(B):
        for y in range(H):
            for x in range(W):
                side = n % 5
                d = (0.5 + (n + 0.5) / npx) * (1.0 - thr)          # one sweep over the field; every side samples all of it
                ox = float(torch.randint(0, W, (1,), generator=g))
                oy = float(torch.randint(0, H, (1,), generator=g))
                if side == 0:
                    ix[b, y, x], iy[b, y, x] = -d, oy
                elif side == 1:
                    ix[b, y, x], iy[b, y, x] = W - 1 + d, oy
                elif side == 2:
                    ix[b, y, x], iy[b, y, x] = ox, -d
                elif side == 3:
                    ix[b, y, x], iy[b, y, x] = ox, H - 1 + d
                else:                                           # (1 - dx)(1 - dy) ~ 1 - d with dx = 0.4 d, dy = 0.6 d
                    ix[b, y, x], iy[b, y, x] = -0.4 * d, H - 1 + 0.6 * d
                n += 1
    return flow_for(ix, iy, cfg)


FAR = (15.0, 16.0, 17.0, 1000.0)


def f_far(B, H, W, cfg, seed=5):
    """sample points 15, 16, 17 and 1000 px outside each side: the clamp at -16 / W + 16"""
    ix, iy = _grid(B, H, W)
    g = _gen(seed)
    n = 0
    for b in range(B):
        for y in range(H):
            for x in range(W):
                side, d = n % 4, FAR[(n // 4 + n) % 4]
                if side == 0:
                    ix[b, y, x], iy[b, y, x] = -d, _interior(H, g)
                elif side == 1:
                    ix[b, y, x], iy[b, y, x] = W - 1 + d, _interior(H, g)
                elif side == 2:
                    ix[b, y, x], iy[b, y, x] = _interior(W, g), -d
                else:
                    ix[b, y, x], iy[b, y, x] = _interior(W, g), H - 1 + d
                n += 1
    return flow_for(ix, iy, cfg)


def _ordinary(B, H, W, cfg):
    """0.25 px: every sample point a quarter of a cell right of and below its own pixel"""
    xs, ys = _grid(B, H, W)
    return flow_for(xs + 0.25, ys + 0.25, cfg)


def wild_pixels(B, H, W):
    """bool [B,H,W]: the checkerboard squares of f_wild that hold a wild flow"""
    xs, ys = _grid(B, H, W)
    return ((xs + ys) % 2) == 1


def f_wild(B, H, W, cfg, seed=6):
    """checkerboard of ordinary flows and +-1e30, +-3e38, +-Inf, NaN in u, in v and in both"""
    flo = _ordinary(B, H, W, cfg)
    wild = wild_pixels(B, H, W)
    n = seed
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if wild[b, y, x]:
                    u, v = WILD_PAIRS[n % len(WILD_PAIRS)]
                    if u is not None:
                        flo[b, 0, y, x] = u
                    if v is not None:
                        flo[b, 1, y, x] = v
                    n += 1
    return flo


def converge_targets(B, H, W):
    """the two source pixels (x, y) of each image of f_converge"""
    return [((min(1 + b, W - 1), min(1, H - 1)), (max(W - 2 - b, 0), max(H - 2, 0))) for b in range(B)]


def f_converge(B, H, W, cfg, seed=7):
    """every pixel of an image samples one of two source pixels, exactly on them: hundreds of contributions to one element of the
    backward scatter, each with weight 1"""
    ix, iy = _grid(B, H, W)
    for b, (p, q) in enumerate(converge_targets(B, H, W)):
        sel = ((torch.arange(H).view(H, 1) + torch.arange(W).view(1, W)) % 2) == 0
        ix[b] = torch.where(sel, torch.tensor(float(p[0]), dtype=torch.float64), torch.tensor(float(q[0]), dtype=torch.float64))
        iy[b] = torch.where(sel, torch.tensor(float(p[1]), dtype=torch.float64), torch.tensor(float(q[1]), dtype=torch.float64))
    return flow_for(ix, iy, cfg)


def tile_centres(H, W):
    """[(row, column)] of the pixel whose flow places each fused tile's LDS window (window_centre: clamped to the map)"""
    (th, tw), (cr, cc) = fused_tile()
    return [(min(ty + cr, H - 1), min(tx + cc, W - 1)) for ty in range(0, H, th) for tx in range(0, W, tw)]


def _set_wild(flo, b, y, x, pair):
    u, v = pair
    if u is not None:
        flo[b, 0, y, x] = u
    if v is not None:
        flo[b, 1, y, x] = v


def f_tile_centre(B, H, W, cfg, seed=8):
    """ordinary flow; on even tiles (tile index + image) the pixel that places the tile's window carries a wild value, indexed by
    the ordinal of the tile so that the first one is +Inf whatever the shape; on odd tiles the opposite: an ordinary centre whose
    eight neighbours are wild"""
    flo = _ordinary(B, H, W, cfg)
    k = m = 0
    for b in range(B):
        for t, (r, c) in enumerate(tile_centres(H, W)):
            if (t + b) % 2 == 0:
                _set_wild(flo, b, r, c, WILD_PAIRS[(4 + 5 * k) % len(WILD_PAIRS)])       # (Inf, .), (., 3e38), (1e30, 1e30), (-Inf, -Inf), ...
                k += 1
            else:
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        yy, xx = r + dy, c + dx
                        if (dy or dx) and 0 <= yy < H and 0 <= xx < W:
                            _set_wild(flo, b, yy, xx, WILD_PAIRS[m % len(WILD_PAIRS)])
                            m += 1
    return flo


def _centre_specials(B, H, W, cfg, specials):
    """ordinary flow; the window-placing pixel of EVERY tile samples specials[ordinal of the tile] (sample coordinates, None = the
    centre's own row / column), built through the inverse like every other field"""
    ix, iy = _grid(B, H, W)
    ix, iy = ix + 0.25, iy + 0.25
    k = 0
    for b in range(B):
        for (r, c) in tile_centres(H, W):
            sx, sy = specials[k % len(specials)]
            ix[b, r, c] = float(c) if sx is None else sx          # the other coordinate ON the pixel: its weight is exactly 1
            iy[b, r, c] = float(r) if sy is None else sy
            k += 1
    return flow_for(ix, iy, cfg)


def f_tile_centre_far(B, H, W, cfg, seed=9):
    """every window-placing pixel samples 17 or 1000 px outside a side, alternating: beyond the taps' clamp at -16 / W + 16, and
    (1000) beyond the clamp of the window origin at -64 / W + 64"""
    return _centre_specials(B, H, W, cfg, [(-17.0, None), (None, H - 1 + 1000.0), (W - 1 + 17.0, None), (None, -1000.0),
                                           (-1000.0, None), (None, H - 1 + 17.0), (W - 1 + 1000.0, None), (None, -17.0)])


def f_tile_centre_thr(B, H, W, cfg, seed=10):
    """every window-placing pixel samples 0.5 (1 - thr) (kept) or 1.5 (1 - thr) (dropped) outside a side, alternating"""
    e = 1.0 - cfg[2]
    return _centre_specials(B, H, W, cfg, [(-0.5 * e, None), (None, H - 1 + 1.5 * e), (W - 1 + 0.5 * e, None), (None, -1.5 * e),
                                           (-1.5 * e, None), (None, H - 1 + 0.5 * e), (W - 1 + 1.5 * e, None), (None, -0.5 * e)])


BUILDERS = {"zero": f_zero, "integer": f_integer, "eighths": f_eighths, "border": f_border, "threshold": f_threshold, "far": f_far,
            "wild": f_wild, "converge": f_converge, "tile_centre": f_tile_centre, "tile_centre_far": f_tile_centre_far,
            "tile_centre_thr": f_tile_centre_thr}

_CACHE = {}


def field(name, shape, cfg, half=False):
    """float32 [B,2,H,W] (a fresh copy; the table itself is built once per process).  half: the field for half-precision storage --
    every value is a half (as float32), and the steering ran over halves, so that a sample point lands in its cell and as close to
    its target as a HALF flow gets (rounding the float32 field would move a flow of 3 px by up to 1e-3 px)."""
    B, _, H, W = shape
    key = (name, B, H, W, cfg, half)
    if key not in _CACHE:
        _HALF[0] = half
        try:
            f = BUILDERS[name](B, H, W, cfg)
        finally:
            _HALF[0] = False
        _CACHE[key] = f.half().float() if half else f
    return _CACHE[key].clone()


_TAPS = {}


def field_taps(name, shape, cfg):
    B, _, H, W = shape
    key = (name, B, H, W, cfg)
    if key not in _TAPS:
        _TAPS[key] = taps(field(name, shape, cfg), cfg)
    return _TAPS[key]


# ---- level_entry: the field reaches the warp through the level's deconvolution ----------------------------------------------------
SAT = 3.0e38          # stands in for +-Inf and NaN in an entry field (0 * Inf in the deconvolution would spread NaN to the neighbours)


def identity_deconv():
    """ConvTranspose2d(2, 2, 4, 2, 1) parameters whose output pixel (2Y + py, 2X + px) is input pixel (Y, X): weight 1 on kernel
    rows / columns 1 and 2 of the own channel, bias 0.  Every other product is 0 * finite = 0, so the up-flow is exact."""
    w = torch.zeros(2, 2, 4, 4)
    for c in range(2):
        w[c, c, 1:3, 1:3] = 1.0
    return w, torch.zeros(2)


def entry_flow(name, shape, cfg):
    """(half-resolution flow [B,2,H/2,W/2], the up-flow [B,2,H,W] the identity deconvolution makes of it).  Each 2x2 block of the
    up-flow carries the constructed value of ONE of its pixels -- the phase rotates with the block index, so every residue of the
    builders' pixel cycles is met -- and that pixel samples exactly where the field wants it; the other three carry the same flow
    from another pixel, which is as good an input as any (the reference taps are computed from the up-flow itself).  Non-finite
    values become +-SAT: they still overflow to Inf inside the warp's own arithmetic (2 * (x + SAT))."""
    B, _, H, W = shape
    full = field(name, shape, cfg)
    full = torch.where(torch.isnan(full), torch.full_like(full, SAT), full).clamp(-SAT, SAT)
    hh, wh = H // 2, W // 2
    low = torch.empty(B, 2, hh, wh)
    for i in range(hh):
        for j in range(wh):
            py, px = divmod((i * wh + j) % 4, 2)
            low[:, :, i, j] = full[:, :, 2 * i + py, 2 * j + px]
    up = low.repeat_interleave(2, 2).repeat_interleave(2, 3).contiguous()
    return low, up


# ---- references ------------------------------------------------------------------------------------------------------------------
def forward(x, t):
    return LA.warp_apply(x, t)


def knife(t, thr):
    return LA.near_threshold(t, thr)


def msum32(t):
    """float32 mask sum times the mask: what the warp of a ones tensor is, bit for bit (blend4 of four ones adds in this order)"""
    w = t[2]
    return ((w[0] + w[1]) + w[2]) + w[3]


def flow_gain(cfg, H, W):
    """d(ix, iy) / d(u, v): flow_scale * W / max(W-1, 1) (align_corners False), flow_scale * (W-1) / max(W-1, 1) (True)"""
    s, align, _ = cfg
    if align:
        return s * (W - 1) / max(W - 1, 1), s * (H - 1) / max(H - 1, 1)
    return s * W / max(W - 1, 1), s * H / max(H - 1, 1)


def grads(x, t, grad_out, cfg):
    """float64 (grad_x, grad_flo, sum_abs_x, sum_abs_flo) of out = warp(x, flo) for the upstream gradient grad_out, from the FLOAT32
    cell indices, fractions and in-bounds flags of warp_taps.  One-sided like the kernels: a sample point exactly on a pixel belongs
    to the cell to its right and below (floor), so d/d ix there is the slope toward the next pixel.  Zero where the mask is zero
    (the reference thresholds its mask in place, which cuts the graph: the mask is a constant).  sum_abs_*: the same sums over the
    absolute values of every term, the scale of the error bounds."""
    x0, y0, w, _, mask, (ax1, ay1, inb) = t
    B, C, H, W = x.shape
    xd, gd = x.double(), grad_out.double()
    flat = xd.reshape(B, C, H * W)
    gx = torch.zeros(B, C, H * W, dtype=torch.float64)
    sx = torch.zeros_like(gx)
    s = []
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        idx = ((y0 + dy).clamp(0, H - 1) * W + (x0 + dx).clamp(0, W - 1)).reshape(B, 1, H * W).expand(B, C, H * W)
        wk = w[k].double().reshape(B, 1, H * W)               # masked weights: zero out of bounds and under the threshold
        gx.scatter_add_(2, idx, gd.reshape(B, C, H * W) * wk)
        sx.scatter_add_(2, idx, gd.reshape(B, C, H * W).abs() * wk)
        v = torch.gather(flat, 2, idx).reshape(B, C, H, W)
        s.append(torch.where(inb[k].unsqueeze(1), v, torch.zeros_like(v)))
    one = torch.ones_like(ax1)
    ax0, ay0 = (one - ax1).double().unsqueeze(1), (one - ay1).double().unsqueeze(1)     # the kernels' float32 1 - a
    bx1, by1 = ax1.double().unsqueeze(1), ay1.double().unsqueeze(1)
    fx, fy = flow_gain(cfg, H, W)
    keep = mask.unsqueeze(1)
    z = torch.zeros(B, 1, H, W, dtype=torch.float64)
    dix = (gd * (ay0 * (s[1] - s[0]) + by1 * (s[3] - s[2]))).sum(1, keepdim=True)
    diy = (gd * (ax0 * (s[2] - s[0]) + bx1 * (s[3] - s[1]))).sum(1, keepdim=True)
    aix = (gd.abs() * (ay0 * (s[1].abs() + s[0].abs()) + by1 * (s[3].abs() + s[2].abs()))).sum(1, keepdim=True)
    aiy = (gd.abs() * (ax0 * (s[2].abs() + s[0].abs()) + bx1 * (s[3].abs() + s[1].abs()))).sum(1, keepdim=True)
    gf = torch.cat([torch.where(keep, dix * fx, z), torch.where(keep, diy * fy, z)], 1)
    sf = torch.cat([torch.where(keep, aix * abs(fx), z), torch.where(keep, aiy * abs(fy), z)], 1)
    return gx.reshape(B, C, H, W), gf, sx.reshape(B, C, H, W), sf


def positive(shape, seed):
    """features bounded away from zero: a warped value is zero only where the mask is"""
    g = _gen(seed)
    return torch.rand(tuple(shape), generator=g, dtype=torch.float32) + 0.5


def signed(shape, seed):
    g = _gen(seed)
    return torch.rand(tuple(shape), generator=g, dtype=torch.float32) * 2 - 1

# fields built on the mask threshold: their knife() count is a constant of the table, asserted in tests/test_warp_cases_cpu.py
# (key: field, BxHxW, configuration); ENTRY_KNIFE_COUNTS: the same for the up-flow entry_flow() makes of them
ON_THE_EDGE = ("border", "threshold", "tile_centre_thr")
KNIFE_COUNTS = {
    ("border", "1x1x8", "s1.25-a0-t0.9999"): 0, ("border", "1x1x8", "s2.5-a1-t0.999"): 0, ("border", "1x1x8", "s1-a1-t0.9999"): 0,
    ("border", "1x2x2", "s1.25-a0-t0.9999"): 0, ("border", "1x2x2", "s2.5-a1-t0.999"): 0, ("border", "1x2x2", "s1-a1-t0.9999"): 0,
    ("border", "1x6x1", "s1.25-a0-t0.9999"): 0, ("border", "1x6x1", "s2.5-a1-t0.999"): 0, ("border", "1x6x1", "s1-a1-t0.9999"): 0,
    ("border", "1x6x2", "s1.25-a0-t0.9999"): 0, ("border", "1x6x2", "s2.5-a1-t0.999"): 0, ("border", "1x6x2", "s1-a1-t0.9999"): 0,
    ("border", "1x9x4", "s1.25-a0-t0.9999"): 0, ("border", "1x9x4", "s2.5-a1-t0.999"): 0, ("border", "1x9x4", "s1-a1-t0.9999"): 0,
    ("border", "1x11x40", "s1.25-a0-t0.9999"): 0, ("border", "1x11x40", "s2.5-a1-t0.999"): 0, ("border", "1x11x40", "s1-a1-t0.9999"): 0,
    ("border", "2x13x20", "s1.25-a0-t0.9999"): 0, ("border", "2x13x20", "s2.5-a1-t0.999"): 0, ("border", "2x13x20", "s1-a1-t0.9999"): 0,
    ("border", "2x13x21", "s1.25-a0-t0.9999"): 0, ("border", "2x13x21", "s2.5-a1-t0.999"): 0, ("border", "2x13x21", "s1-a1-t0.9999"): 0,
    ("border", "2x20x72", "s1.25-a0-t0.9999"): 0, ("border", "2x20x72", "s2.5-a1-t0.999"): 0, ("border", "2x20x72", "s1-a1-t0.9999"): 0,
    ("threshold", "1x1x8", "s1.25-a0-t0.9999"): 0, ("threshold", "1x1x8", "s2.5-a1-t0.999"): 0, ("threshold", "1x1x8", "s1-a1-t0.9999"): 0,
    ("threshold", "1x2x2", "s1.25-a0-t0.9999"): 0, ("threshold", "1x2x2", "s2.5-a1-t0.999"): 0, ("threshold", "1x2x2", "s1-a1-t0.9999"): 0,
    ("threshold", "1x6x1", "s1.25-a0-t0.9999"): 0, ("threshold", "1x6x1", "s2.5-a1-t0.999"): 0, ("threshold", "1x6x1", "s1-a1-t0.9999"): 0,
    ("threshold", "1x6x2", "s1.25-a0-t0.9999"): 0, ("threshold", "1x6x2", "s2.5-a1-t0.999"): 0, ("threshold", "1x6x2", "s1-a1-t0.9999"): 0,
    ("threshold", "1x9x4", "s1.25-a0-t0.9999"): 0, ("threshold", "1x9x4", "s2.5-a1-t0.999"): 0, ("threshold", "1x9x4", "s1-a1-t0.9999"): 0,
    ("threshold", "1x11x40", "s1.25-a0-t0.9999"): 12, ("threshold", "1x11x40", "s2.5-a1-t0.999"): 0, ("threshold", "1x11x40", "s1-a1-t0.9999"): 12,
    ("threshold", "2x13x20", "s1.25-a0-t0.9999"): 10, ("threshold", "2x13x20", "s2.5-a1-t0.999"): 0, ("threshold", "2x13x20", "s1-a1-t0.9999"): 11,
    ("threshold", "2x13x21", "s1.25-a0-t0.9999"): 15, ("threshold", "2x13x21", "s2.5-a1-t0.999"): 1, ("threshold", "2x13x21", "s1-a1-t0.9999"): 12,
    ("threshold", "2x20x72", "s1.25-a0-t0.9999"): 78, ("threshold", "2x20x72", "s2.5-a1-t0.999"): 7, ("threshold", "2x20x72", "s1-a1-t0.9999"): 75,
    ("tile_centre_thr", "1x9x4", "s1.25-a0-t0.9999"): 0, ("tile_centre_thr", "1x9x4", "s2.5-a1-t0.999"): 0, ("tile_centre_thr", "1x9x4", "s1-a1-t0.9999"): 0,
    ("tile_centre_thr", "1x11x40", "s1.25-a0-t0.9999"): 0, ("tile_centre_thr", "1x11x40", "s2.5-a1-t0.999"): 0, ("tile_centre_thr", "1x11x40", "s1-a1-t0.9999"): 0,
    ("tile_centre_thr", "2x20x72", "s1.25-a0-t0.9999"): 0, ("tile_centre_thr", "2x20x72", "s2.5-a1-t0.999"): 0, ("tile_centre_thr", "2x20x72", "s1-a1-t0.9999"): 0,
}
ENTRY_KNIFE_COUNTS = {
    ("border", "1x6x2", "s1.25-a0-t0.9999"): 0, ("border", "1x6x2", "s2.5-a1-t0.999"): 0, ("border", "1x6x2", "s1-a1-t0.9999"): 0,
    ("border", "2x14x22", "s1.25-a0-t0.9999"): 0, ("border", "2x14x22", "s2.5-a1-t0.999"): 0, ("border", "2x14x22", "s1-a1-t0.9999"): 0,
    ("threshold", "1x6x2", "s1.25-a0-t0.9999"): 0, ("threshold", "1x6x2", "s2.5-a1-t0.999"): 0, ("threshold", "1x6x2", "s1-a1-t0.9999"): 0,
    ("threshold", "2x14x22", "s1.25-a0-t0.9999"): 5, ("threshold", "2x14x22", "s2.5-a1-t0.999"): 0, ("threshold", "2x14x22", "s1-a1-t0.9999"): 6,
}
