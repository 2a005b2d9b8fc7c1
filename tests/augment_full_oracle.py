"""Independent NumPy statement of train2.py's KittiAugmentationPipeline (the definition of pwc_kitti_augment_full in include/pwc_hip.h):
int64 / float64 / float32 arithmetic on whole windows, no torch and no call into the product.

The stages run in the REFERENCE'S FORWARD ORDER on whole crop windows -- crop, flip, rotation, translation, brightness / contrast, blur,
/255 -- each through a generic function (`warp_affine`, `gaussian_blur_u8`); that is deliberately not the kernel's read-side composition,
so the two agreeing bit for bit proves the composition.  The translation goes through the generic fixed-point warp like the rotation.

cv2.warpAffine (INTER_LINEAR, BORDER_REFLECT, float32 sources), cv2.getRotationMatrix2D and the bit-exact 8U cv2.GaussianBlur are
restated from OpenCV's published sources; parity against an actual cv2 build is unpinned, and the blur weights are rounded from a float64
Gaussian where OpenCV uses softdouble.  CASES is the named table of the GPU tests."""
import math

import numpy as np

from augment_oracle import decode_png, invert_affine, make_sample, reflect101  # noqa: F401  (tests/augment_oracle.py, NumPy only)

f32 = np.float32
f64 = np.float64


def reflect(p, length):
    """BORDER_REFLECT index (fedcba|abcdef|fedcba) for any integer p (array or scalar): period 2 len."""
    p = np.asarray(p, dtype=np.int64)
    period = 2 * length
    m = np.mod(p, period)                       # numpy's mod is non-negative for a positive divisor
    return np.where(m < length, m, period - 1 - m)


def rotation_matrix(center_xy, angle_deg):
    """cv2.getRotationMatrix2D(center, angle, 1.0): float64 2x3."""
    rad = float(angle_deg) * (math.pi / 180.0)
    al, be = math.cos(rad), math.sin(rad)
    cx, cy = float(center_xy[0]), float(center_xy[1])
    return np.array([[al, be, (1.0 - al) * cx - be * cy], [-be, al, be * cx + (1.0 - al) * cy]], dtype=f64)


def warp_affine(src, M, out_hw, border="reflect", inverse_map=False):
    """cv2.warpAffine(src, M, (W, H), flags=INTER_LINEAR [| WARP_INVERSE_MAP], borderMode=BORDER_REFLECT) for float32 [h,w] / [h,w,C]:
    the classic fixed-point coordinates (ten fraction bits rounded to five), four taps folded over the source, the float blend
    ((p00*w00 + p01*w01) + p10*w10) + p11*w11 with every operation rounded to float32."""
    assert src.dtype == f32 and border == "reflect"
    m = np.asarray(M, dtype=f64).reshape(6) if inverse_map else invert_affine(M)
    H, W = out_hw
    h, w = src.shape[:2]
    Y, X = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    Yd, Xd = Y.astype(f64), X.astype(f64)
    ad = np.rint(m[0] * Xd * 1024.0).astype(np.int64)          # np.rint rounds half to even
    bd = np.rint(m[3] * Xd * 1024.0).astype(np.int64)
    X0 = np.rint((m[1] * Yd + m[2]) * 1024.0).astype(np.int64) + 16
    Y0 = np.rint((m[4] * Yd + m[5]) * 1024.0).astype(np.int64) + 16
    Xq, Yq = (X0 + ad) >> 5, (Y0 + bd) >> 5                    # arithmetic shifts on int64
    sx, sy, fx, fy = Xq >> 5, Yq >> 5, Xq & 31, Yq & 31
    ya, yb, xa, xb = reflect(sy, h), reflect(sy + 1, h), reflect(sx, w), reflect(sx + 1, w)
    gx, gy = fx.astype(f32) / f32(32), fy.astype(f32) / f32(32)
    one = f32(1)
    w00, w01, w10, w11 = (one - gy) * (one - gx), (one - gy) * gx, gy * (one - gx), gy * gx
    if src.ndim == 3:
        w00, w01, w10, w11 = (t[..., None] for t in (w00, w01, w10, w11))
    out = ((src[ya, xa] * w00 + src[ya, xb] * w01) + src[yb, xa] * w10) + src[yb, xb] * w11
    assert out.dtype == f32
    return out


def gaussian_weights(sigma):
    """(k, uint16 [k]): k = ceil(4 sigma) made odd; the float64 Gaussian normalised to 1, converted to Q8.8 from the outside in with
    the rounding error carried, the centre = 256 - the rest."""
    k = int(np.ceil(4 * sigma))
    if k % 2 == 0:
        k += 1
    x = np.arange(k, dtype=f64) - (k - 1) * 0.5
    g = np.exp(-(x * x) / (2.0 * sigma * sigma))
    g = g / g.sum()
    w = np.zeros(k, np.int64)
    err = 0.0
    for i in range(k // 2):
        adj = g[i] * 256.0 + err
        v = np.rint(adj)
        err = adj - v
        w[i] = w[k - 1 - i] = int(v)
    w[k // 2] = 256 - w.sum()
    assert w.min() >= 0 and w.sum() == 256
    return k, w.astype(np.uint16)


def gaussian_blur_u8(src, weights):
    """cv2.GaussianBlur of a uint8 [h,w] / [h,w,C] image with the given Q8.8 weights in both directions, BORDER_REFLECT_101: OpenCV's
    bit-exact path -- horizontal sums in uint16, vertical sums in uint32, (v + 32768) >> 16."""
    assert src.dtype == np.uint8
    wk = [int(v) for v in weights]
    k = len(wk)
    assert k % 2 == 1 and sum(wk) == 256
    r = k // 2
    h, w = src.shape[:2]
    xs = reflect101(np.arange(-r, w + r), w)
    ys = reflect101(np.arange(-r, h + r), h)
    s = src.astype(np.int64)
    hp = sum(wk[i] * s[:, xs[i:i + w]] for i in range(k))
    assert hp.max() <= 65535
    hp = hp.astype(np.uint16).astype(np.int64)
    vp = sum(wk[j] * hp[ys[j:j + h]] for j in range(k))
    assert vp.max() + 32768 < 1 << 32
    return ((vp + 32768) >> 16).astype(np.uint8)


def augment_full(sample, rec, crop_hw, rows=None):
    """One sample through the reference's stages in the reference's order.  sample = (im1, im2 uint8 [H,W,3], u, v float32 [H,W],
    valid [H,W] (non-zero = valid) or None); rec: a mapping with the fields of pwc_augment_full_params.  rows: optional list of window
    rows to return (every stage still runs on the whole window: a blurred, shifted, rotated row depends on all of it).
    -> x float32 [6,h,w], flow float32 [2,h,w], mask float32 [1,h,w] with h = len(rows) or crop_h."""
    im1, im2, u, v, valid = sample
    H, W = im1.shape[:2]
    ch, cw = crop_hw
    y0, x0 = int(rec["y0"]), int(rec["x0"])
    assert H >= ch and W >= cw and 0 <= y0 <= H - ch and 0 <= x0 <= W - cw
    win = (slice(y0, y0 + ch), slice(x0, x0 + cw))
    imgs = np.concatenate([im1[..., :3], im2[..., :3]], axis=2).astype(f32)[win]
    flow = np.stack([np.asarray(u, f32), np.asarray(v, f32)], axis=-1)[win].copy()
    mask = (np.ones((H, W), f32) if valid is None else (np.asarray(valid) != 0).astype(f32))[win]
    if rec["flip"]:
        imgs = np.ascontiguousarray(imgs[:, ::-1])
        flow = np.ascontiguousarray(flow[:, ::-1])
        flow[:, :, 0] *= f32(-1)
        mask = np.ascontiguousarray(mask[:, ::-1])
    if rec["rot"]:
        m = np.asarray(rec["m"], dtype=f64)
        imgs = warp_affine(imgs, m, (ch, cw), inverse_map=True)
        flow = warp_affine(flow, m, (ch, cw), inverse_map=True)
        mask = warp_affine(mask, m, (ch, cw), inverse_map=True)
        c, s = f64(rec["cs"][0]), f64(rec["cs"][1])
        fu, fv = flow[:, :, 0].astype(f64), flow[:, :, 1].astype(f64)
        ru = (fu * c - fv * s).astype(f32)                       # float64 arithmetic, stored as float32 ...
        rv = (ru.astype(f64) * s + fv * c).astype(f32)          # ... and the second line reads the stored u
        flow = np.stack([ru, rv], axis=-1)
    if rec["trans"]:
        M = np.array([[1, 0, int(rec["tx"])], [0, 1, int(rec["ty"])]], dtype=f32)
        imgs = warp_affine(imgs, M, (ch, cw))
        flow = warp_affine(flow, M, (ch, cw))
        mask = warp_affine(mask, M, (ch, cw))
    if rec["bright"]:
        g = f32(rec["gain"])
        imgs = np.clip(g * (imgs - f32(127.5)) + f32(127.5), f32(0), f32(255))
        assert imgs.dtype == f32
    if rec["blur"]:
        k = int(rec["ksize"])
        imgs = gaussian_blur_u8(imgs.astype(np.uint8), np.asarray(rec["wk"])[:k]).astype(f32)
    x = imgs / f32(255.0)
    assert x.dtype == f32 and flow.dtype == f32 and mask.dtype == f32
    x, flow, mask = x.transpose(2, 0, 1), flow.transpose(2, 0, 1), mask[None]
    if rows is not None:
        rows = np.asarray(rows, dtype=np.int64)
        x, flow, mask = x[:, rows], flow[:, rows], mask[:, rows]
    return np.ascontiguousarray(x), np.ascontiguousarray(flow), np.ascontiguousarray(mask)


def record(size_hw, crop_hw, y0=0, x0=0, flip=False, rot=None, trans=None, bright=None, blur=None):
    """A parameter record as a dict.  rot: degrees about (crop_w // 2, crop_h // 2); trans: (tx, ty); bright: the gain; blur: sigma."""
    H, W = size_hw
    ch, cw = crop_hw
    rec = {"m": np.array([1, 0, 0, 0, 1, 0], f64), "cs": np.array([1, 0], f64), "gain": f32(1), "wk": np.array([0, 256, 0, 0, 0, 0, 0], np.uint16),
           "ksize": 3, "y0": y0, "x0": x0, "h": H, "w": W, "tx": 0, "ty": 0, "flip": int(bool(flip)), "rot": 0, "trans": 0, "bright": 0,
           "blur": 0}
    if rot is not None:
        theta = np.radians(rot)
        rec.update(m=invert_affine(rotation_matrix((cw // 2, ch // 2), rot)), cs=np.array([np.cos(theta), np.sin(theta)], f64), rot=1)
    if trans is not None:
        rec.update(tx=int(trans[0]), ty=int(trans[1]), trans=1)
    if bright is not None:
        rec.update(gain=f32(bright), bright=1)
    if blur is not None:
        k, w = gaussian_weights(blur)
        wk = np.zeros(7, np.uint16)
        wk[:k] = w
        rec.update(wk=wk, ksize=k, blur=1)
    return rec


ALL = dict(rot=11.0, trans=(7, -5), bright=1.13, blur=1.1)
SIG_ABOVE = float(np.nextafter(0.75, 1.0))             # the first sigma with five taps

# The GPU cases: name -> (crop_hw, [(size_hw, record keywords), ...]); every sample of a case goes into one batch whose slot is the
# largest size.  The reference draws |angle| <= 17, |tx|, |ty| <= 10, gain in [0.64, 1.44], sigma in [0.5, 1.5).
CASES = {
    # each stage alone and all five together, flip off and on, three frame sizes in one batch
    "stages": ((32, 64), [((48, 80), dict(y0=3, x0=5)), ((45, 77), dict(y0=13, x0=13, flip=True)),
                          ((50, 72), dict(y0=9, x0=2, rot=9.5)), ((48, 80), dict(y0=0, x0=16, rot=-13.0, flip=True)),
                          ((45, 77), dict(y0=1, x0=0, trans=(4, -9))), ((50, 72), dict(y0=18, x0=8, trans=(-10, 3), flip=True)),
                          ((48, 80), dict(y0=16, x0=0, bright=1.3)), ((45, 77), dict(y0=5, x0=6, bright=0.7, flip=True)),
                          ((50, 72), dict(y0=7, x0=7, blur=0.9)), ((48, 80), dict(y0=2, x0=11, blur=1.4, flip=True)),
                          ((45, 77), dict(y0=6, x0=3, **ALL)), ((50, 72), dict(y0=11, x0=1, flip=True, **ALL))]),
    # width 53 is no multiple of 4 and the tile's edge is not the window's: guarded stores, ragged last lane; the tests also hand
    # this case misaligned output views
    "ragged": ((37, 53), [((41, 60), dict(y0=2, x0=3, **ALL)), ((37, 53), dict(flip=True, rot=-17.0, blur=0.6)),
                          ((40, 57), dict(y0=3, x0=4, trans=(-3, 8), bright=0.8))]),
    # windows smaller than the halo and the shift: several reflections of both border kinds
    "tiny": ((5, 7), [((9, 11), dict(y0=2, x0=1, rot=17.0, trans=(10, -10), blur=1.5)),
                      ((5, 7), dict(rot=-17.0, trans=(-10, 10), bright=1.2, blur=1.5, flip=True)),
                      ((6, 9), dict(y0=1, x0=2, trans=(10, 10), blur=1.3)), ((5, 7), dict(trans=(-10, -10))),
                      ((7, 7), dict(y0=2, blur=1.5))]),
    # a single row: len == 1 in reflect101, period 2 in reflect
    "line": ((1, 9), [((3, 12), dict(y0=1, x0=2, rot=17.0, trans=(10, -10), blur=1.5)),
                      ((1, 9), dict(rot=-17.0, trans=(-10, 10), blur=1.5, flip=True)), ((1, 9), dict(blur=1.26)),
                      ((2, 10), dict(y0=1, trans=(3, 10), bright=0.64))]),
    # 8 x 128 tiles: 2 full + a ragged third in both directions, blur on: the halo crosses tile borders and window borders
    "tiles": ((19, 260), [((21, 264), dict(y0=2, x0=4, **ALL)), ((19, 260), dict(blur=1.5, flip=True)),
                          ((20, 262), dict(y0=1, x0=1, rot=-6.0, blur=0.7))]),
    # the extremes of each draw: +-17 and 0 degrees; gain 0.64 and 1.44 (the clamp at both ends); sigma at the tap-count switches
    "extremes": ((32, 64), [((48, 80), dict(y0=16, x0=16, rot=17.0)), ((48, 80), dict(rot=-17.0, flip=True)), ((48, 80), dict(y0=4, x0=4, rot=0.0)),
                            ((48, 80), dict(y0=1, x0=9, bright=0.64)), ((48, 80), dict(y0=9, x0=1, bright=1.44)),
                            ((48, 80), dict(blur=0.5)), ((48, 80), dict(blur=0.75)), ((48, 80), dict(blur=SIG_ABOVE)),
                            ((48, 80), dict(blur=1.25)), ((48, 80), dict(blur=1.5)), ((48, 80), dict(rot=17.0, bright=1.44, blur=1.5))]),
    # blurred and plain samples side by side in one launch
    "mixed": ((24, 40), [((40, 64), dict(y0=3, x0=9, blur=1.0)), ((37, 61), dict(y0=13, x0=21, rot=5.0)),
                         ((33, 64), dict(y0=9, x0=0, flip=True, blur=0.55, trans=(1, 1))), ((40, 47), dict(y0=0, x0=7)),
                         ((37, 61), dict(bright=1.1, rot=-3.0, blur=1.45))]),
}


def case_inputs(name):
    """The seeded samples and records of a case: ([(im1, im2, png)], [record dict], crop_hw, slot_hw)."""
    crop, items = CASES[name]
    seed0 = 1500 + 19 * sorted(CASES).index(name)
    samples = [make_sample(size, seed0 + i) for i, (size, _) in enumerate(items)]
    recs = [record(size, crop, **kw) for size, kw in items]
    slot = (max(s[0] for s, _ in items), max(s[1] for s, _ in items))
    return samples, recs, crop, slot


def case_expected(samples, recs, crop, with_valid=True, rows=None):
    """Oracle outputs of a batch -> (x [n,6,h,w], flow [n,2,h,w], mask [n,1,h,w])."""
    outs = []
    for (im1, im2, png), rec in zip(samples, recs):
        u, v, m = decode_png(png)
        outs.append(augment_full((im1, im2, u, v, m if with_valid else None), rec, crop, rows=rows))
    return tuple(np.stack([o[i] for o in outs]) for i in range(3))
