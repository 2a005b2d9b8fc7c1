"""Independent NumPy statement of the KITTI training augmentation (the definition in include/pwc_hip.h): int64 / float64 / float32
arithmetic on arrays of coordinates, no torch and no call into the product.

cv2.warpAffine(src, M, (W, H), INTER_LINEAR, BORDER_REFLECT_101) is restated from OpenCV's published classic fixed-point path (the one
used through 4.10); parity against an actual cv2 build is unpinned.  `warp_affine` is that function for uint8 and float32 sources;
`augment` is one sample of KittiFlowDataset.__getitem__ computed on the crop window only; CASES is the named table of the GPU tests."""
import math

import numpy as np

f32 = np.float32


def reflect101(p, length):
    """BORDER_REFLECT_101 index for any integer p (array or scalar): period 2(len-1), len == 1 -> 0."""
    p = np.asarray(p, dtype=np.int64)
    if length == 1:
        return np.zeros_like(p)
    period = 2 * (length - 1)
    m = np.mod(p, period)                       # numpy's mod is non-negative for a positive divisor
    return np.where(m < length, m, period - m)


def affine_matrix(center_xy, rot_deg, sx, sy):
    """(M float32 2x3, A float32 2x2): A = R S from float64 cos / sin rounded to float32, t = c - A c with every product and sum
    rounded to float32."""
    theta = float(rot_deg) * (math.pi / 180.0)
    c, s = math.cos(theta), math.sin(theta)
    A = np.array([[f32(sx * c), f32(-sy * s)], [f32(sx * s), f32(sy * c)]], dtype=f32)
    cx, cy = f32(center_xy[0]), f32(center_xy[1])
    tx = f32(cx - f32(f32(A[0, 0] * cx) + f32(A[0, 1] * cy)))
    ty = f32(cy - f32(f32(A[1, 0] * cx) + f32(A[1, 1] * cy)))
    M = np.array([[A[0, 0], A[0, 1], tx], [A[1, 0], A[1, 1], ty]], dtype=f32)
    return M, A


def invert_affine(M):
    """cv::warpAffine's inversion of the 2x3 matrix, in double."""
    m0, m1, m2, m3, m4, m5 = (float(v) for v in np.asarray(M, dtype=np.float64).ravel())
    D = m0 * m4 - m1 * m3
    D = 1.0 / D if D != 0.0 else 0.0
    a11 = m4 * D
    a22 = m0 * D
    m0 = a11
    m1 = m1 * -D
    m3 = m3 * -D
    m4 = a22
    b1 = -m0 * m2 - m1 * m5
    b2 = -m3 * m2 - m4 * m5
    return np.array([m0, m1, b1, m3, m4, b2], dtype=np.float64)


def taps(m, Y, X, H, W):
    """Fixed-point source coordinates of the frame positions (Y, X) (int64 arrays of one shape) under the inverted matrix m ->
    (ya, yb, xa, xb reflected tap rows / columns, fy, fx in 0..31)."""
    Y = np.asarray(Y, dtype=np.int64)
    X = np.asarray(X, dtype=np.int64)
    Yd, Xd = Y.astype(np.float64), X.astype(np.float64)
    ad = np.rint(m[0] * Xd * 1024.0).astype(np.int64)          # np.rint rounds half to even
    bd = np.rint(m[3] * Xd * 1024.0).astype(np.int64)
    X0 = np.rint((m[1] * Yd + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((m[4] * Yd + m[5]) * 1024.0).astype(np.int64) + 16
    Xq = (X0 + ad) >> 5                                         # arithmetic shifts on int64
    Yq = (Y0 + bd) >> 5
    sx, sy, fx, fy = Xq >> 5, Yq >> 5, Xq & 31, Yq & 31
    return reflect101(sy, H), reflect101(sy + 1, H), reflect101(sx, W), reflect101(sx + 1, W), fy, fx


def blend_u8(src, t):
    """uint8 [H,W] or [H,W,C] source at the taps -> uint8, OpenCV's 15-bit table blend in its short form."""
    ya, yb, xa, xb, fy, fx = t
    if src.ndim == 3:
        fy, fx = fy[..., None], fx[..., None]
    s = src.astype(np.int64)
    v = s[ya, xa] * (32 - fy) * (32 - fx) + s[ya, xb] * (32 - fy) * fx + s[yb, xa] * fy * (32 - fx) + s[yb, xb] * fy * fx
    return ((v + 512) >> 10).astype(np.uint8)


def blend_f32(src, t):
    """float32 [H,W] source at the taps -> float32: ((p00*w00 + p01*w01) + p10*w10) + p11*w11, every operation rounded to float32."""
    ya, yb, xa, xb, fy, fx = t
    assert src.dtype == f32 and src.ndim == 2
    gx, gy = fx.astype(f32) / f32(32), fy.astype(f32) / f32(32)
    one = f32(1)
    w00, w01, w10, w11 = (one - gy) * (one - gx), (one - gy) * gx, gy * (one - gx), gy * gx
    out = ((src[ya, xa] * w00 + src[ya, xb] * w01) + src[yb, xa] * w10) + src[yb, xb] * w11
    assert out.dtype == f32
    return out


def warp_affine(src, M, out_hw):
    """cv2.warpAffine(src, M, (W, H), flags=INTER_LINEAR, borderMode=BORDER_REFLECT_101) for uint8 [h,w] / [h,w,C] and float32 [h,w]."""
    H, W = out_hw
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    t = taps(invert_affine(M), Y, X, src.shape[0], src.shape[1])
    if src.dtype == np.uint8:
        return blend_u8(src, t)
    if src.dtype == f32:
        if src.ndim == 3:
            return np.stack([blend_f32(np.ascontiguousarray(src[..., c]), t) for c in range(src.shape[2])], axis=-1)
        return blend_f32(src, t)
    raise TypeError("warp_affine: uint8 or float32 sources only, got %s" % src.dtype)


def decode_png(png):
    """uint16 [H,W,3] (R, G, B) -> (u, v float32, valid float32 0/1)."""
    u = (png[..., 0].astype(f32) - f32(32768)) / f32(64)
    v = (png[..., 1].astype(f32) - f32(32768)) / f32(64)
    return u, v, (png[..., 2] != 0).astype(f32)


def augment(im1, im2, u, v, valid, rec, crop_hw, rows=None):
    """One sample on its crop window.  im1 / im2 uint8 [H,W,3]; u, v float32 [H,W]; valid [H,W] (non-zero = valid) or None; rec a dict
    with m (six doubles), a (four float32), y0, x0, warp, flip.  rows: optional list of window rows to compute (the others are not).
    -> x float32 [6,h,w], flow float32 [2,h,w], valid float32 [1,h,w] with h = len(rows) or crop_h."""
    H, W = im1.shape[:2]
    ch, cw = crop_hw
    y0, x0 = int(rec["y0"]), int(rec["x0"])
    assert H >= ch and W >= cw and 0 <= y0 <= H - ch and 0 <= x0 <= W - cw
    ys = np.arange(ch, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    xs = np.arange(cw, dtype=np.int64)
    if rec["flip"]:
        xs = cw - 1 - xs
    Y, X = np.meshgrid(y0 + ys, x0 + xs, indexing="ij")
    m = f32(1) if valid is None else (np.asarray(valid) != 0).astype(f32)
    u, v = np.ascontiguousarray(u, dtype=f32), np.ascontiguousarray(v, dtype=f32)
    if not rec["warp"]:
        a, b = im1[Y, X], im2[Y, X]
        fu, fv = u[Y, X], v[Y, X]
        fm = np.ones(Y.shape, f32) if valid is None else m[Y, X]
    else:
        t = taps(np.asarray(rec["m"], dtype=np.float64), Y, X, H, W)
        a, b = blend_u8(im1, t), blend_u8(im2, t)
        ru, rv = blend_f32(u, t), blend_f32(v, t)
        A = np.asarray(rec["a"], dtype=f32).reshape(4)
        fu = A[0] * ru + A[1] * rv
        fv = A[2] * ru + A[3] * rv
        rm = blend_f32(np.ones((H, W), f32) if valid is None else m, t)
        fm = (rm > f32(0.5)).astype(f32)
    if rec["flip"]:
        fu = fu * f32(-1.0)
    x = np.concatenate([a, b], axis=-1).astype(f32) / f32(255.0)
    assert x.dtype == f32 and fu.dtype == f32 and fv.dtype == f32
    return np.ascontiguousarray(x.transpose(2, 0, 1)), np.stack([fu, fv]), fm[None]


def record(size_hw, y0=0, x0=0, warp=None, flip=False):
    """A parameter record as a dict; warp = (rot_deg, sx, sy) about the frame's centre, or None."""
    H, W = size_hw
    rec = {"m": np.array([1, 0, 0, 0, 1, 0], np.float64), "a": np.array([1, 0, 0, 1], f32), "y0": y0, "x0": x0, "h": H, "w": W,
           "warp": 0, "flip": int(bool(flip))}
    if warp is not None:
        M, A = affine_matrix((W * 0.5, H * 0.5), *warp)
        rec.update(m=invert_affine(M), a=A.reshape(4).copy(), warp=1)
    return rec


def make_sample(size_hw, seed):
    """Seeded (im1, im2 uint8 [H,W,3], png uint16 [H,W,3]): textured frames, a smooth flow on the 1/64 grid, ~25 % invalid pixels."""
    H, W = size_hw
    g = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    ims = []
    for _ in range(2):
        base = 127 + 80 * np.sin(0.31 * xx + 0.17 * yy + g.uniform(0, 6))[..., None] * np.array([1.0, 0.7, -0.8])
        ims.append(np.clip(base + g.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8))
    u = 6.0 * np.sin(0.11 * xx + 0.07 * yy + g.uniform(0, 6)) + g.normal(0, 0.5, (H, W))
    v = 3.0 * np.cos(0.09 * xx - 0.13 * yy + g.uniform(0, 6)) + g.normal(0, 0.5, (H, W))
    png = np.stack([np.clip(np.rint(u * 64.0 + 32768.0), 0, 65535), np.clip(np.rint(v * 64.0 + 32768.0), 0, 65535),
                    g.random((H, W)) > 0.25], axis=-1).astype(np.uint16)
    return ims[0], ims[1], png


# The GPU cases: name -> (crop_hw, [(size_hw, record keywords), ...]); every sample of a case goes into one batch whose slot is the
# largest size.  Extremes of the reference's draw: |rot| <= 2 degrees, sx, sy in [0.95 * 0.97, 1.05 * 1.03] = [0.9215, 1.0815].
CASES = {
    # (a) no warp: the odd width 41 takes the 4-byte store path and its ragged last lane
    "skip_flip": ((24, 41), [((37, 53), dict(y0=5, x0=7)), ((37, 53), dict(y0=13, x0=12, flip=True)), ((37, 53), dict())]),
    # (b) the extremes of the reduced augmentation, the window in the two opposite corners
    "extremes": ((32, 64), [((48, 80), dict(warp=(2.0, 1.0815, 0.9215))), ((48, 80), dict(y0=16, x0=16, warp=(-2.0, 0.9215, 1.0815))),
                            ((48, 80), dict(y0=16, x0=16, warp=(2.0, 0.9215, 0.9215), flip=True)),
                            ((48, 80), dict(warp=(-2.0, 1.0815, 1.0815), flip=True))]),
    # (c) far out of range: the taps reflect over more than one period of a 9 x 13 source
    "far": ((8, 12), [((9, 13), dict(y0=1, x0=1, warp=(75.0, 0.3, 0.3))), ((9, 13), dict(warp=(-120.0, 0.2, 0.35), flip=True))]),
    # (d) skip, warp, flip and warp + flip over three different sizes in 40 x 64 slots
    "mixed": ((24, 40), [((40, 64), dict(y0=3, x0=9)), ((37, 61), dict(y0=13, x0=21, warp=(1.3, 1.02, 0.97))),
                         ((33, 64), dict(y0=9, x0=0, flip=True)), ((40, 47), dict(y0=0, x0=7, warp=(-1.7, 0.95, 1.06), flip=True)),
                         ((37, 61), dict(y0=0, x0=0, warp=(0.4, 1.0, 1.0)))]),
    # a window that is a multiple of 4 wide but spans two tiles in x and two in y with a ragged bottom
    "tiles": ((19, 132), [((21, 140), dict(y0=2, x0=8, warp=(1.1, 1.01, 0.99), flip=True)), ((21, 140), dict(y0=0, x0=3))]),
    # single-row / single-column sources: reflect101 with len == 1
    "line": ((1, 8), [((1, 9), dict(x0=1, warp=(0.0, 0.9, 1.0))), ((1, 9), dict(warp=(2.0, 1.05, 1.0), flip=True))]),
}


def case_inputs(name):
    """The seeded samples and records of a case: ([(im1, im2, png)], [record dict], crop_hw, slot_hw)."""
    crop, items = CASES[name]
    seed0 = 1400 + 17 * sorted(CASES).index(name)
    samples = [make_sample(size, seed0 + i) for i, (size, _) in enumerate(items)]
    recs = [record(size, **kw) for size, kw in items]
    slot = (max(s[0] for s, _ in items), max(s[1] for s, _ in items))
    return samples, recs, crop, slot


def case_expected(samples, recs, crop, with_valid=True):
    """Oracle outputs of a batch -> (x [n,6,h,w], flow [n,2,h,w], valid [n,1,h,w])."""
    outs = []
    for (im1, im2, png), rec in zip(samples, recs):
        u, v, m = decode_png(png)
        outs.append(augment(im1, im2, u, v, m if with_valid else None, rec, crop))
    return tuple(np.stack([o[i] for o in outs]) for i in range(3))
