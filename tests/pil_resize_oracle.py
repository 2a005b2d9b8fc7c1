"""NumPy restatement of Pillow's Image.resize(..., BILINEAR) for 8-bit RGB images and float32 ("F") planes, and the case tables shared
by tools/gen_golden_pil_resize*.py, tests/test_pil_resize*_cpu.py and tests/test_gpu_pil_resize*.py.  The coefficient tables are the
product's (opticalflow_amd.pil_resize.coeff_tables / fixed_point, pure host code); the fixtures tests/golden/g17_pil_resize.npz and
g20_pil_resize_edges.npz, made by Pillow itself, arbitrate between this file and the library.

Two rules of Image.resize sit above the passes and are restated here: the pass of an axis whose length does not change is skipped
(nothing is computed, so -0.0, infinities and NaN stay where they are), and a source with H > 100 * W whose height shrinks takes the
vertical pass first."""
import hashlib

import numpy as np

from opticalflow_amd.pil_resize import coeff_tables, fixed_point

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# name -> (n, source (H, W), target (h, w), seed)
FRAME_CASES = {
    "hd_ratio": (1, (270, 480), (96, 128), 101),          # the 1080p ratio: 9 and 7 taps
    "kitti_ratio": (1, (94, 311), (96, 320), 102),        # inference.py's KITTI ratio, slight upscale on both axes
    "odd_up": (1, (47, 61), (64, 64), 103),
    "mixed": (1, (200, 130), (64, 128), 104),             # x3.125 down on one axis, x1.016 on the other
    "h_only": (1, (64, 100), (64, 64), 105),
    "v_only": (1, (100, 64), (64, 64), 106),
    "identity": (1, (64, 64), (64, 64), 107),
    "clamped": (1, (129, 5), (64, 64), 108),              # 5-pixel-wide source: every horizontal bound clamped
    "one_pixel": (1, (1, 1), (8, 8), 109),
    "down8": (1, (512, 520), (64, 65), 110),              # the edge of the supported range
    "ragged": (1, (150, 201), (70, 67), 111),             # output not a multiple of any tile
    "batch3": (3, (90, 75), (40, 52), 112),
}
# name -> (B, source (h, w), target (H, W), seed)
FLOW_CASES = {
    "kitti_up": (1, (24, 80), (94, 311), 201),
    "odd_up": (2, (16, 20), (61, 77), 202),
    "down": (1, (40, 64), (17, 23), 203),
    "identity": (1, (24, 40), (24, 40), 204),
    "mixed": (1, (7, 9), (30, 5), 205),
}
NORM_CASE = "odd_up"      # the frame case whose normalised float output (torch CPU operators) is in the fixture

# ---- g20: the edges.  name -> (n, source (H, W), target (h, w), seed)
FRAME_EDGE_CASES = {
    "near8": (1, (263, 1037), (33, 130), 401),            # scales 7.97 / 7.98: ksize 17 on both axes, 3 x 3 tiles
    "frac5": (2, (171, 333), (35, 71), 402),
    "up_tiles": (1, (3, 5), (40, 200), 403),              # every tile reads the same 3 rows and 5 columns, bounds clamped
    "up_thin": (1, (2, 2), (130, 3), 404),
    "narrow3": (2, (37, 29), (19, 3), 405),               # narrower than one 4-pixel quad
    "to_one": (1, (16, 16), (1, 1), 406),
    "down8_small": (1, (9, 40), (2, 5), 407),
    "row_src": (1, (1, 300), (20, 70), 408),
    "col_src": (1, (300, 1), (70, 20), 409),
    "tile_over": (1, (50, 140), (17, 65), 410),           # one row / column past a tile
    "tile_under": (1, (48, 130), (15, 63), 411),
    "tile_exact": (1, (64, 256), (16, 64), 412),
    "group_ragged": (3, (45, 50), (18, 21), 413),
    "group_vec": (5, (45, 50), (20, 24), 414),
    "tall": (1, (648, 6), (130, 5), 415),                 # H > 100 * W and h < H: Pillow takes the vertical pass first
    "tall_upx": (2, (913, 7), (130, 9), 416),
    "tall_edge_in": (1, (601, 6), (130, 5), 417),
    "tall_edge_out": (1, (600, 6), (130, 5), 418),        # the inequality is strict: horizontal first
    "tall_no_down": (1, (648, 6), (700, 5), 419),         # h > H: horizontal first
}
# name -> (n, c, source (h, w), target (H, W), seed)
PLANE_EDGE_CASES = {
    "down_tiles": (1, 2, (100, 333), (37, 141), 501),     # 3 x 3 tiles with ksize 7
    "down8": (1, 1, (264, 1040), (33, 130), 502),         # the largest staging: 138 rows
    "near8": (1, 2, (263, 1037), (33, 130), 503),
    "chan3": (2, 3, (20, 30), (33, 70), 504),
    "chan5": (1, 5, (20, 30), (9, 70), 505),
    "tiny_up": (1, 1, (1, 1), (5, 7), 506),
    "tiny_down": (1, 2, (2, 1), (1, 1), 507),
    "to_one": (1, 1, (9, 9), (1, 1), 508),
    "tile_over": (1, 1, (50, 140), (17, 65), 509),
    "tile_under": (1, 1, (48, 130), (15, 63), 510),
    "row_src": (1, 1, (1, 300), (20, 70), 511),
    "col_src": (1, 1, (300, 1), (70, 20), 512),
    "tall": (1, 2, (648, 6), (130, 5), 513),
    "tall_edge_in": (1, 2, (601, 6), (130, 5), 514),
    "tall_edge_out": (1, 2, (600, 6), (130, 5), 515),
}
CHAN3_FACTORS = (1.5, -0.25, 3.0)
# name -> (source, target, seed): one plane pair over make_flow data with special values planted (make_special)
PLANE_SPECIAL_CASES = {
    "identity": ((24, 40), (24, 40), 601),
    "y_unchanged": ((24, 40), (24, 90), 602),
    "x_unchanged": ((24, 40), (50, 40), 603),
    "upscale": ((24, 40), (50, 90), 604),
    "downscale": ((40, 64), (17, 23), 605),
}
UNCHANGED_AXIS_SPECIALS = ("identity", "y_unchanged", "x_unchanged")
SWEEP_OUT = (1, 15, 16, 17, 63, 64, 65, 130)
SWEEP_SEED = 7000


def sweep_lengths(O):
    """The input lengths of AXIS_SWEEP for one output length: around O, its multiples up to the edge of the range, and below it."""
    got = []
    for I in (1, 2, O - 1, O, O + 1, 2 * O - 1, 2 * O, 3 * O + 1, 5 * O - 2, 7 * O + 3, 8 * O - 1, 8 * O, 3 * O // 5, O // 7):
        if 1 <= I <= 8 * O and I not in got:
            got.append(I)
    return got


def _axis_sweep():
    out = []
    for O in SWEEP_OUT:
        for I in sweep_lengths(O):
            out.append((O, (6, I), (5, O)))               # the pair as the horizontal axis
            out.append((O, (I, 6), (O, 5)))               # ... and as the vertical one (I >= 601 with O = 130: the tall regime)
    return tuple(out)


AXIS_SWEEP = _axis_sweep()     # (O, source, target); entry i takes its inputs from seed SWEEP_SEED + i


def sweep_inputs(i):
    """(frame uint8 [1,H,W,3], plane float32 [H,W]) of sweep entry i."""
    _, src, _ = AXIS_SWEEP[i]
    return make_frames(1, src, SWEEP_SEED + i), make_flow(1, src, SWEEP_SEED + i)[0, 0]


def vertical_first(src, dst):
    """Image.resize's order: the vertical pass first for a source more than 100 times as tall as wide whose height shrinks."""
    return src[0] > 100 * src[1] and dst[0] < src[0]


def make_frames(n, hw, seed):
    """uint8 [n,H,W,3]: noise over a gradient, the top third replaced by 0 / 255 blocks so that saturated sums occur."""
    H, W = hw
    rng = np.random.RandomState(seed)
    ramp = (np.arange(W)[None, :, None] * 3 + np.arange(H)[:, None, None] * 2 + np.arange(3)[None, None, :] * 50) % 256
    img = (ramp[None] // 2 + rng.randint(0, 128, (n, H, W, 3))).astype(np.uint8)
    th = (H + 2) // 3
    blocks = rng.randint(0, 2, (n, (th + 3) // 4, (W + 3) // 4, 3)).astype(np.uint8) * 255
    img[:, :th] = np.repeat(np.repeat(blocks, 4, axis=1), 4, axis=2)[:, :th, :W]
    return np.ascontiguousarray(img)


def make_flow(B, hw, seed):
    """float32 [B,2,h,w] ~ N(0, 30) with a few values at +-1e4."""
    h, w = hw
    rng = np.random.RandomState(seed)
    f = (rng.randn(B, 2, h, w) * 30.0).astype(np.float32)
    flat = f.reshape(-1)
    idx = rng.choice(flat.size, size=max(2, flat.size // 97), replace=False)
    flat[idx] = np.where(rng.randint(0, 2, idx.size) == 1, 1e4, -1e4).astype(np.float32)
    return f


def make_planes(n, c, hw, seed):
    """float32 [n,c,h,w]: make_flow's channels for c <= 2, plain N(0, 30) for more."""
    if c <= 2:
        return np.ascontiguousarray(make_flow(n, hw, seed)[:, :c])
    return (np.random.RandomState(seed).randn(n, c, hw[0], hw[1]) * 30).astype(np.float32)


def make_special(hw, seed):
    """float32 [1,2,h,w] (h >= 24, w >= 40): make_flow data with -0.0 and +inf inside, -inf in column 0, a 2 x 2 block of 3e38, one
    denormal, and NaN as the last element."""
    f = make_flow(1, hw, seed)
    f[0, 0, 5, 7] = -0.0
    f[0, 0, 11, 19] = np.inf
    f[0, 0, 15:17, 30:32] = 3e38
    f[0, 1, 9, 0] = -np.inf
    f[0, 1, 3, 12] = 1e-42
    f[0, 1, -1, -1] = np.nan
    return f


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest_bytes(a):
    """sha256 as uint8 [32], the form the sweep's digests are stored in."""
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def _order(src, dst, tall_rule):
    """(axis, new length) of the two passes in Pillow's order."""
    first = (0, 1) if tall_rule and vertical_first(src, dst) else (1, 0)
    return [(axis, dst[axis]) for axis in first]


def _pass_u8(img, out_size, axis):
    """One 8-bit pass along `axis` of [H,W,C]: clip8((2^21 + sum src * k) >> 22), in int32 like the C code."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    bounds, coeffs = coeff_tables(src.shape[0], out_size)
    k = fixed_point(coeffs)
    out = np.empty((out_size,) + src.shape[1:], np.uint8)
    for i in range(out_size):
        first, cnt = bounds[i]
        ss = np.full(src.shape[1:], 1 << 21, np.int32)
        for t in range(cnt):
            ss = ss + src[first + t] * k[i, t]
        out[i] = np.clip(ss >> 22, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize_u8(img, size, skip_unchanged=True, tall_rule=True):
    """[H,W,3] uint8 -> [h,w,3]: the horizontal pass first (the vertical one for a tall source, vertical_first), rounded to bytes,
    then the other; no pass on an axis whose length stays.  The two switches exist to show that a case exercises a rule: with one
    off, the cases of that rule must differ from the fixture."""
    for axis, length in _order(img.shape[:2], size, tall_rule):
        if not skip_unchanged or img.shape[axis] != length:
            img = _pass_u8(img, length, axis)
    return np.ascontiguousarray(img)


def _pass_f32(plane, out_size, axis):
    """One float pass: ss = 0.0; ss += (double)src * w in tap order (multiply and add separate); stored as float32."""
    src = np.moveaxis(plane, axis, 0).astype(np.float64)
    bounds, coeffs = coeff_tables(src.shape[0], out_size)
    out = np.empty((out_size,) + src.shape[1:], np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(out_size):
            first, cnt = bounds[i]
            ss = np.zeros(src.shape[1:], np.float64)
            for t in range(cnt):
                ss = ss + src[first + t] * coeffs[i, t]
            out[i] = ss.astype(np.float32)
    return np.moveaxis(out, 0, axis)


def resize_f32(plane, size, skip_unchanged=True, tall_rule=True):
    """[h,w] float32 -> [H,W] as Pillow resizes a mode "F" image: passes, order and switches as in resize_u8."""
    for axis, length in _order(plane.shape, size, tall_rule):
        if not skip_unchanged or plane.shape[axis] != length:
            plane = _pass_f32(plane, length, axis)
    return np.ascontiguousarray(plane)


def resize_planes(x, size, **kw):
    """[n,c,h,w] float32 -> [n,c,H,W], every plane on its own."""
    return np.stack([np.stack([resize_f32(p, size, **kw) for p in item]) for item in x])


def resize_flow(flow, size, scale_vectors=True):
    """inference.py's resize_flow for [B,2,h,w] -> [B,2,H,W]."""
    H, W = size
    B, _, h, w = flow.shape
    out = np.stack([np.stack([resize_f32(flow[b, c], size) for c in range(2)]) for b in range(B)])
    if scale_vectors:
        out[:, 0] *= (W / w)
        out[:, 1] *= (H / h)
    return out


def normalise(u8, mean=None, std=None):
    """ToTensor + Normalize of resized bytes [n,h,w,3] with torch's CPU operators -> float32 [n,3,h,w] (numpy)."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(u8)).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    if mean is not None:
        m = torch.as_tensor(mean, dtype=torch.float32)[None, :, None, None]
        s = torch.as_tensor(std, dtype=torch.float32)[None, :, None, None]
        t = t.sub_(m).div_(s)
    return t.numpy()
