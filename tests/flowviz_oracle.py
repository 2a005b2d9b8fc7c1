"""Float64 restatement of the flow pictures (opticalflow_amd/flowviz.py, csrc/pwc_flowviz.hip) for the tests: flow_to_color of
pwc_extract_flow.py:58-123, calculate_dominant_direction and draw_flow_arrows of topview.py:122-178, create_quiver_frame of
pwc_extract_flow_video.py:94-135.  Inputs are the float32 fields; everything after them is float64, except the two places where
float32 is part of the definition: cv::resize casts its source coordinate to float, and the flow itself.

Every function also returns its KNIFE-EDGE set: the outputs whose float64 value lies so close to a decision point that fp32
arithmetic may fall on the other side.  These are properties of the inputs alone (tools/gen_golden_flowviz.py asserts how few there
are); a test lets the code under test differ from the reference there, by one level / one pixel / the flag, and nowhere else.
  colour   the pre-truncation value is not an integer and lies within COLOR_DELTA = 1e-3 levels of an integer in 1..255.  1e-3 is 4 x
           the largest pre-truncation error of an all-fp32 emulation of the chain (<= 2.6e-4 levels; the generator re-measures it on
           the fixture's fields and asserts <= COLOR_DELTA / 3)
  tips     the float64 coordinate is within TIP_DELTA = 1e-3 px of k + 0.5 (round) or of an integer (truncate); 1e-3 px is 8 ulp of
           fp32 at 2048, the widest frame covered
  keep, aligned, dominant membership   within FLAG_DELTA = 1e-4 (px; degrees for the angle) of the threshold
"""
import numpy as np

COLOR_DELTA = 1e-3
TIP_DELTA = 1e-3
FLAG_DELTA = 1e-4


def colorwheel():
    """uint8 [55,3]: RY 15, YG 6, GC 4, CB 11, BM 13, MR 6."""
    w = np.zeros((55, 3), np.int64)
    seg = [(15, 0, 1, +1), (6, 1, 0, -1), (4, 1, 2, +1), (11, 2, 1, -1), (13, 2, 0, +1), (6, 0, 2, -1)]    # (n, full, ramp, direction)
    col = 0
    for n, full, ramp, sign in seg:
        r = (255 * np.arange(n)) // n
        w[col:col + n, full] = 255
        w[col:col + n, ramp] = r if sign > 0 else 255 - r
        col += n
    return w.astype(np.uint8)


def clip_uv(flow, clip_flow):
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    if clip_flow is not None:
        rad = np.sqrt(u * u + v * v)
        k = clip_flow / np.maximum(np.maximum(rad, 1e-5), clip_flow)
        u, v = u * k, v * k
    return u, v


def color(flow, clip_flow=None):
    """flow float32 [h,w,2] -> (rgb uint8 [h,w,3], pre float64 [h,w,3] the values before truncation, knife bool [h,w,3])."""
    u, v = clip_uv(flow, clip_flow)
    rad = np.sqrt(u * u + v * v)
    ang = np.arctan2(-v, -u) / np.pi
    fk = (ang + 1.0) / 2.0 * 54.0 + 1.0
    k0 = np.floor(fk)
    f = (fk - k0)[..., None]
    k0 = (k0.astype(np.int64) - 1) % 55
    k1 = (k0 + 1) % 55
    wheel = colorwheel() / 255.0
    c0, c1 = wheel[k0], wheel[k1]
    col = c0 + f * (c1 - c0)                   # exactly c0 where both entries agree, as the reference's exact (1 - f) + f
    rn = np.clip(rad / (rad.max() + 1e-5), 0.0, 1.0)[..., None]
    col = 1.0 - rn * (1.0 - col)
    pre = np.clip(col, 0.0, 1.0) * 255.0
    near = np.rint(pre)
    knife = (pre != near) & (np.abs(pre - near) < COLOR_DELTA) & (near >= 1) & (near <= 255)
    return pre.astype(np.uint8), pre, knife


def stats(flow, threshold=1.0, clip_flow=None):
    """-> (max radius after the clip, count, mean [2] float64, number of pixels within FLAG_DELTA of the threshold)."""
    u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    mag = np.sqrt(u * u + v * v)
    sel = mag > threshold
    n = int(np.count_nonzero(sel))
    mean = np.array([u[sel].mean(), v[sel].mean()]) if n else np.zeros(2)
    cu, cv = clip_uv(flow, clip_flow)
    return float(np.sqrt(cu * cu + cv * cv).max()), n, mean, int(np.count_nonzero(np.abs(mag - threshold) < FLAG_DELTA))


def _axis(src, dst):
    """xofs / alpha of cv::resize INTER_LINEAR: the coordinate is computed in double and CAST TO FLOAT (part of the definition)."""
    scale = 1.0 / (float(dst) / float(src))
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx)
    fx = (fx - sx).astype(np.float64)
    sx = sx.astype(np.int64)
    lo, hi = sx < 0, sx >= src - 1
    fx[lo | hi] = 0.0
    sx = np.where(lo, 0, np.where(hi, src - 1, sx))
    return sx, np.minimum(sx + 1, src - 1), fx


def resize_at(plane, H, W, ys, xs):
    """cv2.resize(plane, (W, H)) (float path) at rows ys and columns xs, blended in float64 -> [len(ys), len(xs)]."""
    p = plane.astype(np.float64)
    h, w = p.shape
    if (h, w) == (H, W):
        return p[np.ix_(ys, xs)]
    x0, x1, fx = _axis(w, W)
    y0, y1, fy = _axis(h, H)
    x0, x1, fx, y0, y1, fy = x0[xs], x1[xs], fx[xs], y0[ys], y1[ys], fy[ys]
    rows = p[:, x0] * (1.0 - fx) + p[:, x1] * fx
    return rows[y0] * (1.0 - fy)[:, None] + rows[y1] * fy[:, None]


def quiver(flow, frame_hw, step, gain, tip_rule, min_mag, vec_scale=None, dominant=None, angle_threshold=30.0):
    """flow float32 [h,w,2] -> dict of vec float64 [Gy,Gx,2], tip int64 [Gy,Gx,2], keep / aligned bool [Gy,Gx] and the knife-edge sets
    knife_tip [Gy,Gx,2], knife_keep, knife_aligned [Gy,Gx]."""
    H, W = frame_hw
    h, w = flow.shape[:2]
    if vec_scale is None:
        vec_scale = (float(W) / float(w), float(H) / float(h))
    ys, xs = np.arange(0, H, step), np.arange(0, W, step)
    dx = resize_at(flow[..., 0], H, W, ys, xs) * float(np.float32(vec_scale[0]))
    dy = resize_at(flow[..., 1], H, W, ys, xs) * float(np.float32(vec_scale[1]))
    mag = np.sqrt(dx * dx + dy * dy)
    g = float(np.float32(gain))
    t = np.stack([xs[None, :] + dx * g, ys[:, None] + dy * g], axis=-1)
    if tip_rule == 0:
        tip = np.rint(t).astype(np.int64)
        knife_tip = np.abs(np.abs(t - np.floor(t)) - 0.5) < TIP_DELTA
    else:
        tip = np.trunc(t).astype(np.int64)
        knife_tip = np.abs(t - np.rint(t)) < TIP_DELTA
    aligned = np.ones(mag.shape, bool)
    knife_aligned = np.zeros(mag.shape, bool)
    if dominant is not None and np.linalg.norm(np.asarray(dominant, np.float64)) > 0:
        d = np.asarray(dominant, np.float64)
        d = d / np.linalg.norm(d)
        with np.errstate(invalid="ignore", divide="ignore"):
            deg = np.degrees(np.arccos(np.clip((dx * d[0] + dy * d[1]) / mag, -1.0, 1.0)))
        aligned = deg < angle_threshold
        knife_aligned = np.abs(deg - angle_threshold) < FLAG_DELTA
    return dict(vec=np.stack([dx, dy], axis=-1), tip=tip, keep=~(mag < min_mag), aligned=aligned, knife_tip=knife_tip,
                knife_keep=np.abs(mag - min_mag) < FLAG_DELTA, knife_aligned=knife_aligned)


# ---- the cases of tests/golden/g13_flowviz.npz (tools/gen_golden_flowviz.py builds the fields and runs the reference on them) ----
# field name -> (h, w); the arrays are in the fixture as "field/<name>" float32 [h,w,2]
FIELDS = {"smooth": (96, 160), "noise": (48, 80), "radial": (48, 80), "tiny": (48, 80), "huge": (48, 80), "odd": (37, 53),
          "one": (1, 1), "zero": (8, 12), "axis": (2, 4)}
CLIPS = (None, 4.0)
# colour case -> (field, crop or None); every case runs with both CLIPS; fixture "color/<case>/<0|1>" uint8 [h,w,3]
COLOR_CASES = {name: (name, None) for name in FIELDS}
COLOR_CASES["crop"] = ("smooth", (77, 130))
# dominant-direction case -> (field, crop, threshold); fixture "dom/<case>" = float32 [2] mean, "domn/<case>" = count
DOMINANT_CASES = {"smooth": ("smooth", None, 1.0), "noise": ("noise", None, 1.0), "radial": ("radial", None, 1.0),
                  "odd": ("odd", None, 1.0), "crop": ("smooth", (77, 130), 1.0), "tiny": ("tiny", None, 1.0), "huge": ("huge", None, 250.0)}
# arrow case -> (field, crop, frame (H, W), step, style, scale, min_mag, dominant case or None, angle threshold, vec_scale or None)
#   "video": create_quiver_frame on the cropped flow; "topview": draw_flow_arrows on the stub-resized flow (min_mag is its fixed 0.5,
#   vec_scale (1, 1): topview.py rescales after resizing).  Fixture "q/<case>/keep|tip|aligned".
QUIVER_CASES = {
    "odd16": ("odd", None, (148, 212), 16, "video", 1.0, 5.0, None, 30.0, None),             # ragged last row and column
    "odd20": ("odd", None, (148, 212), 20, "video", 0.5, 0.5, None, 30.0, None),
    "odd20_top": ("odd", None, (148, 212), 20, "topview", 5.0, 0.5, "odd", 30.0, (1.0, 1.0)),
    "n16": ("noise", (16, 32), (64, 128), 16, "video", 1.0, 4.0, None, 30.0, None),
    "n20_top": ("noise", (16, 32), (64, 128), 20, "topview", 5.0, 0.5, "noise", 45.0, (1.0, 1.0)),
    "crop20": ("smooth", (77, 130), (148, 212), 20, "video", 2.0, 0.5, None, 30.0, None),
    "low": ("noise", (3, 32), (12, 128), 16, "video", 1.0, 4.0, None, 30.0, None),             # a frame lower than one step: one grid row
    "same16": ("odd", None, (37, 53), 16, "video", 1.0, 1.5, None, 30.0, None),                # flow size == frame size: no resize
    "same20_top": ("odd", None, (37, 53), 20, "topview", 5.0, 0.5, "odd", 30.0, (1.0, 1.0)),
    "wide": ("radial", (8, 80), (32, 2048), 16, "video", 0.25, 0.5, None, 30.0, None),         # the widest frame TIP_DELTA is sized for
}


def cropped(field, crop):
    return np.ascontiguousarray(field if crop is None else field[:crop[0], :crop[1]])


def gain_rule(style, scale):
    return (1.0 / max(scale, 1e-6), 0) if style == "video" else (float(scale), 1)
