"""NumPy statement of cv2.resize (INTER_LINEAR) as the scripts around the model use it (script_pwc.py:43-83, topview.py:79-119), from
OpenCV's published algorithm (modules/imgproc/src/resize.cpp): int64 / float32 arithmetic on arrays, no torch and no import of the
product.  It is held to harness.cv2_resize_linear and to the hand-worked vectors of tests/test_harness.py by tests/test_cv_resize_cpu.py;
cv2 itself is absent here, so cv2 parity is unpinned.  Also the case tables and seeded input makers the CPU and GPU tests share."""
import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# name -> (n, source (H, W), destination (h, w), seed)
FRAME_CASES = {
    "up_small": (1, (13, 17), (64, 64), 11),
    "pair": (2, (50, 70), (64, 128), 12),
    "harness": (1, (100, 150), (128, 192), 13),
    "identity": (3, (64, 128), (64, 128), 14),
    "one_axis": (1, (64, 100), (64, 128), 15),
    "one_pixel_axis": (1, (1, 5), (64, 64), 16),
    "tie_x": (1, (3, 517), (64, 576), 7),           # 517 -> 576 holds an 11-bit coefficient exactly on .5
    "tie_y": (1, (38, 5), (129, 64), 7),            # explicit size, the tie on the vertical axis
}
# bytes of these cases that change when the coefficients are rounded half up instead of half to even (counted on the CPU; the count
# belongs to the seeded bytes, what matters is that it is not zero)
TIE_CASES = {"tie_x": 31, "tie_y": 6}

# name -> (n, source (h, w), destination (H, W), seed)
FLOW_CASES = {
    "down_odd": (1, (16, 16), (13, 17), 21),
    "harness": (1, (32, 48), (100, 150), 22),
    "batch_x4": (2, (16, 32), (64, 128), 23),
    "identity": (3, (24, 40), (24, 40), 24),        # holds -0.0, +-inf and NaN
    "one_axis": (1, (16, 32), (16, 71), 25),
    "down": (1, (40, 64), (9, 14), 26),
    "one_pixel_axis": (1, (1, 5), (3, 11), 27),
}
SPECIALS_CASE = "identity"


def make_frames(n, hw, seed):
    """uint8 [n,H,W,3]."""
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + tuple(hw) + (3,), dtype=np.uint8)


def make_flow(n, hw, seed, specials=False):
    """float32 [n,2,h,w] in [-1, 1), the scale of the network's output (pixels / 20) and of the planes tests/test_harness.py bounds at
    2e-4 (|flow * 20| up to 20); specials: -0.0, +-inf and NaN at fixed places."""
    f = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 2) + tuple(hw)).astype(np.float32)
    if specials:
        f[0, 0, 1, 2] = np.float32(-0.0)
        f[0, 1, 3, 5] = np.float32(np.inf)
        f[-1, 0, 7, 11] = np.float32(-np.inf)
        f[-1, 1, 2, 1] = np.float32(np.nan)
        f[0, 1, 0, 0] = np.float32(-0.0)
    return f


def axis(src, dst):
    """(s0 int64 [dst], s1 = min(s0 + 1, src - 1), fx float32 [dst]): double scale, float fx, a clamped tap gets fx = 0."""
    scale = 1.0 / (float(dst) / float(src))
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx)
    fx = (fx - sx).astype(np.float32)
    sx = sx.astype(np.int64)
    lo, hi = sx < 0, sx >= src - 1
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    sx = np.where(lo, 0, np.where(hi, src - 1, sx))
    return sx, np.minimum(sx + 1, src - 1), fx


def axis_scalar(src, dst):
    """The same table by a plain loop over destination indices."""
    import math
    scale = 1.0 / (float(dst) / float(src))
    s0, fx = [], []
    for d in range(dst):
        f = np.float32((d + 0.5) * scale - 0.5)
        s = int(math.floor(float(f)))
        f = np.float32(f - np.float32(s))
        if s < 0:
            s, f = 0, np.float32(0)
        if s >= src - 1:
            s, f = src - 1, np.float32(0)
        s0.append(s)
        fx.append(f)
    return np.asarray(s0, np.int32), np.asarray(fx, np.float32)


def coef11(w, half_up=False):
    """cvRound(w * 2048) for float32 weights: round half to even.  half_up: floor(v + 0.5) instead (NOT OpenCV; the tie cases use it
    to show that they tell the two apart)."""
    v = (np.asarray(w, np.float32) * np.float32(2048)).astype(np.float32)
    return (np.floor(v.astype(np.float64) + 0.5) if half_up else np.rint(v)).astype(np.int64)


def resize_u8(img, out_hw, half_up=False):
    """uint8 [H,W] or [H,W,C] -> [h,w(,C)]: the 11-bit fixed-point passes.  Equal sizes go through them too (weight 2048 is exact)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    H, W = img.shape[:2]
    h, w = out_hw
    x0, x1, fx = axis(W, w)
    y0, y1, fy = axis(H, h)
    tail = (1,) * (img.ndim - 2)
    a0 = coef11(np.float32(1) - fx, half_up).reshape((1, w) + tail)
    a1 = coef11(fx, half_up).reshape((1, w) + tail)
    b0 = coef11(np.float32(1) - fy, half_up).reshape((h, 1) + tail)
    b1 = coef11(fy, half_up).reshape((h, 1) + tail)
    s = img.astype(np.int64)
    rows = s[:, x0] * a0 + s[:, x1] * a1
    out = (((b0 * (rows[y0] >> 4)) >> 16) + ((b1 * (rows[y1] >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def resize_f32(img, out_hw):
    """float32 [H,W] -> [h,w]: the two float32 passes, every product and sum rounded; a copy when the size does not change."""
    img = np.asarray(img)
    assert img.dtype == np.float32 and img.ndim == 2
    H, W = img.shape
    h, w = out_hw
    if (H, W) == (h, w):
        return img.copy()
    x0, x1, fx = axis(W, w)
    y0, y1, fy = axis(H, h)
    one = np.float32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        rows = (img[:, x0] * (one - fx)[None] + img[:, x1] * fx[None]).astype(np.float32)
        return (rows[y0] * (one - fy)[:, None] + rows[y1] * fy[:, None]).astype(np.float32)


def byte_lut(mean=None, std=None):
    """float32 [3,256]: float32(float64(v) / 255.0) (script_pwc.py:58), then (lut - mean[c]) / std[c] in float32 per output channel."""
    lut = np.repeat((np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)[None], 3, axis=0)
    if mean is not None:
        m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
        lut = ((lut - m[:, None]).astype(np.float32) / s[:, None]).astype(np.float32)
    return lut


def ingest(frames, out_hw, flip=True, mean=None, std=None, half_up=False):
    """uint8 [n,H,W,3] -> float32 [n,3,h,w]: resize, [:, :, ::-1] when flip, the byte table by output channel, HWC -> CHW."""
    lut = byte_lut(mean, std)
    out = []
    for f in frames:
        r = resize_u8(f, out_hw, half_up)
        if flip:
            r = r[:, :, ::-1]
        out.append(np.stack([lut[c][r[:, :, c]] for c in range(3)]))
    return np.stack(out).astype(np.float32)


def ingest_pairs(pairs, out_hw, flip=True):
    """uint8 [n,2,H,W,3] -> float32 [n,6,h,w]."""
    n = pairs.shape[0]
    x = ingest(pairs.reshape((2 * n,) + pairs.shape[2:]), out_hw, flip)
    return x.reshape((n, 6) + tuple(out_hw))


def flow_exit(flow, out_hw, gain, fu, fv, hwc=False):
    """float32 [n,2,h,w] -> [n,2,H,W] (or [n,H,W,2]): (flow * gain) resized, u * float32(fu), v * float32(fv), all in float32."""
    flow = np.asarray(flow)
    assert flow.dtype == np.float32
    fac = (np.float32(fu), np.float32(fv))
    with np.errstate(invalid="ignore", over="ignore"):
        t = (flow * np.float32(gain)).astype(np.float32)
        out = np.stack([np.stack([(resize_f32(t[b, c], out_hw) * fac[c]).astype(np.float32) for c in range(2)]) for b in range(len(t))])
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1)) if hwc else out


def script_factors(out_hw, flow_hw):
    """u * W / W_, v * H / H_ with (H_, W_) = 4 x the flow's size (script_pwc.py:79-80)."""
    return out_hw[1] / float(4 * flow_hw[1]), out_hw[0] / float(4 * flow_hw[0])


def real_bilinear(img, out_hw):
    """float64 [H,W] -> [h,w]: the real-valued interpolation (centre (i + 0.5) * H / h - 0.5, clamped taps)."""
    H, W = img.shape
    h, w = out_hw
    ys = (np.arange(h) + 0.5) * H / h - 0.5
    xs = (np.arange(w) + 0.5) * W / w - 0.5
    y0, x0 = np.floor(ys).astype(int), np.floor(xs).astype(int)
    wy, wx = ys - y0, xs - x0
    y0c, y1c = np.clip(y0, 0, H - 1), np.clip(y0 + 1, 0, H - 1)
    x0c, x1c = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1)
    top = img[y0c][:, x0c] * (1 - wx)[None] + img[y0c][:, x1c] * wx[None]
    bot = img[y1c][:, x0c] * (1 - wx)[None] + img[y1c][:, x1c] * wx[None]
    return top * (1 - wy)[:, None] + bot * wy[:, None]


def same_bits_nan_by_position(got, want):
    """Bit equality everywhere except NaN, which only has to sit at the same places (payloads differ between processors)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(gn, wn) and np.array_equal(got.view(np.int32)[~gn], want.view(np.int32)[~wn]))
