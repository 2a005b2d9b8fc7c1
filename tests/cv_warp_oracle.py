"""NumPy statement of cv2.warpPerspective on 8-bit frames as topview.py:218,232 calls it (INTER_LINEAR, BORDER_CONSTANT, border value 0),
from OpenCV's published algorithm (imgproc's warpPerspective plus the 8-bit bilinear remap): float64 / int64 arithmetic on arrays, no
torch and no import of the product.  tests/test_cv_warp_cpu.py holds it to a plain scalar loop and to hand-worked vectors; cv2 itself
is absent here, so cv2 parity is unpinned -- and with it how OpenCV's int16 weight table stores the single weight 32768 at a zero
fraction on both axes (taken as 32768: an identity warp returns the image).  Also the case table and seeded makers the CPU and GPU
tests share."""
import math

import numpy as np

INT_MAX, INT_MIN = 2147483647.0, -2147483648.0

# name -> (n, source (H, W), destination (h, w), seed); the matrices: case_matrices(name)
WARP_CASES = {
    "identity": (3, (64, 128), (64, 128), 41),      # every weight 0 or 1024; rows of whole dwords
    "topview": (2, (100, 150), (100, 150), 42),     # the script's warp; rows of 450 bytes; three 64-pixel blocks
    "short": (1, (5, 150), (5, 150), 43),           # bh0 = 5, bw0 = 150: one block
    "narrow": (1, (37, 5), (37, 5), 44),            # rows shorter than a thread's run
    "dsize": (1, (40, 50), (33, 70), 45),           # destination size differs from the source's
    "shift": (1, (20, 70), (20, 70), 46),           # border taps are 0, whole rows and columns outside
    "subpix": (1, (20, 70), (20, 70), 47),          # exact fractional weights
    "tie": (1, (9, 70), (9, 70), 48),               # both coordinates exactly on .5 before cvRound
    "zoomout": (1, (48, 64), (48, 64), 49),         # mixed in and out taps along slanted edges
    "horizon": (1, (9, 70), (9, 70), 50),           # Wd == 0, negative denominators; INT_MIN / INT_MAX and int16 clamps
    "per_frame": (2, (37, 64), (37, 64), 51),       # one matrix per frame
}
# bytes of these cases that change when the fixed-point coordinates are rounded half up instead of half to even (counted on the CPU;
# the count belongs to the seeded bytes, what matters is that it is not zero)
TIE_CASES = {"tie": 1770}


def make_frames(n, hw, seed):
    """uint8 [n,H,W,3]."""
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + tuple(hw) + (3,), dtype=np.uint8)


# ------------------------------------------------------------------ matrices
def invert3x3(M):
    """OpenCV's closed 3x3 inverse in float64: determinant by cofactor expansion along the first row, d = 1.0 / det, adjugate * d."""
    S = np.asarray(M, np.float64)
    d = (S[0, 0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) - S[0, 1] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0])
         + S[0, 2] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]))
    assert d != 0.0
    d = 1.0 / d
    t = np.empty((3, 3), np.float64)
    t[0, 0] = (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) * d
    t[0, 1] = (S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]) * d
    t[0, 2] = (S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]) * d
    t[1, 0] = (S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]) * d
    t[1, 1] = (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) * d
    t[1, 2] = (S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]) * d
    t[2, 0] = (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]) * d
    t[2, 1] = (S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]) * d
    t[2, 2] = (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) * d
    return t


def perspective_matrix(src_pts, dst_pts):
    """cv2.getPerspectiveTransform: the 8x8 system on the float32 points widened to double, c22 = 1."""
    src = np.asarray(src_pts, np.float32).astype(np.float64)
    dst = np.asarray(dst_pts, np.float32).astype(np.float64)
    A, b = np.zeros((8, 8)), np.zeros(8)
    for i in range(4):
        A[i, 0] = A[i + 4, 3] = src[i, 0]
        A[i, 1] = A[i + 4, 4] = src[i, 1]
        A[i, 2] = A[i + 4, 5] = 1.0
        A[i, 6] = -src[i, 0] * dst[i, 0]
        A[i, 7] = -src[i, 1] * dst[i, 0]
        A[i + 4, 6] = -src[i, 0] * dst[i, 1]
        A[i + 4, 7] = -src[i, 1] * dst[i, 1]
        b[i], b[i + 4] = dst[i, 0], dst[i, 1]
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def topview_points(width, height):
    """The eight points of topview.py:57-76 as float32: (source [4,2], destination [4,2])."""
    src = np.float32([[width * 0.2, height * 0.8], [width * 0.8, height * 0.8], [width * 0.3, height * 0.4], [width * 0.7, height * 0.4]])
    dst = np.float32([[width * 0.2, height * 0.9], [width * 0.8, height * 0.9], [width * 0.2, height * 0.1], [width * 0.8, height * 0.1]])
    return src, dst


def topview_matrix(width, height):
    return perspective_matrix(*topview_points(width, height))


def translation(tx, ty):
    """The inverse map (x, y) -> (x + tx, y + ty)."""
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def case_matrices(name):
    """The runs of a case: a list of (M, inverse_map), M [3,3] or [n,3,3] in float64."""
    n, (H, W), _, _ = WARP_CASES[name]
    if name == "identity":
        return [(np.eye(3), False)]
    if name in ("topview", "short", "narrow", "dsize"):
        return [(topview_matrix(W, H), False)]
    if name == "shift":
        return [(translation(-7.0, 3.0), True)]
    if name == "subpix":
        return [(translation(13.0 / 32.0, 5.0 / 32.0), True)]
    if name == "tie":
        return [(translation(1.0 / 64.0, 0.25 + 1.0 / 64.0), True)]
    if name == "zoomout":
        a, s, cx, cy = math.radians(20.0), 1.7, (W - 1) / 2.0, (H - 1) / 2.0
        c, d = s * math.cos(a), s * math.sin(a)
        return [(np.array([[c, -d, cx - (c * cx - d * cy)], [d, c, cy - (d * cx + c * cy)], [0.0, 0.0, 1.0]]), True)]
    if name == "horizon":
        return [(np.array([[1.0, 0.0, 5.0], [0.0, 1.0, 5.0], [1.0, 0.0, w22]]), True) for w22 in (-3.0, -3.0000000001)]
    if name == "per_frame":
        return [(np.stack([invert3x3(topview_matrix(W, H)), translation(-7.0, 3.0)]), True)]
    raise KeyError(name)


# ------------------------------------------------------------------ the statement
def coords(Mi, h, w, half_up=False):
    """Fixed-point source coordinates of every destination pixel: (sx, sy, ax, ay), int64 [h,w].  half_up: floor(v + 0.5) instead of
    cvRound (NOT OpenCV; the tie case uses it to show that it tells the two apart)."""
    M = np.asarray(Mi, np.float64).reshape(9)
    bh0 = min(16, h)
    bw0 = min(1024 // bh0, w)
    x = np.arange(w)
    xb = ((x // bw0) * bw0).astype(np.float64)[None]
    x1 = (x - (x // bw0) * bw0).astype(np.float64)[None]
    y = np.arange(h, dtype=np.float64)[:, None]
    X0 = (M[0] * xb + M[1] * y) + M[2]
    Y0 = (M[3] * xb + M[4] * y) + M[5]
    W0 = (M[6] * xb + M[7] * y) + M[8]
    Wd = W0 + M[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wd = np.where(Wd != 0, 32.0 / np.where(Wd != 0, Wd, 1.0), 0.0)
        out = []
        for v in ((X0 + M[0] * x1) * Wd, (Y0 + M[3] * x1) * Wd):
            f = np.where(v < INT_MAX, v, INT_MAX)                   # std::min(INT_MAX, v): a NaN becomes INT_MAX
            f = np.where(INT_MIN < f, f, INT_MIN)                   # std::max(INT_MIN, f)
            out.append((np.floor(f + 0.5) if half_up else np.rint(f)).astype(np.int64))
    X, Y = out
    return np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767), X & 31, Y & 31


def warp(img, M, dsize, inverse=False, half_up=False):
    """uint8 [H,W] or [H,W,C] -> [h,w(,C)] with dsize = (h, w)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    H, W = img.shape[:2]
    h, w = dsize
    Mi = np.asarray(M, np.float64) if inverse else invert3x3(M)
    sx, sy, ax, ay = coords(Mi, h, w, half_up)
    acc = np.zeros((h, w) + img.shape[2:], np.int64)
    tail = (1,) * (img.ndim - 2)
    for dy, wy in ((0, 32 - ay), (1, ay)):
        for dx, wx in ((0, 32 - ax), (1, ax)):
            yy, xx = sy + dy, sx + dx
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64)
            acc += (ok * wx * wy).reshape((h, w) + tail) * v
    out = (acc + 512) >> 10
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def warp_frames(frames, M, dsize, inverse=False, half_up=False):
    """uint8 [n,H,W,3] -> [n,h,w,3]; M [3,3] for all frames or [n,3,3]."""
    M = np.asarray(M, np.float64)
    return np.stack([warp(f, M if M.ndim == 2 else M[i], dsize, inverse, half_up) for i, f in enumerate(frames)])


def warp_scalar(img, Mi, dsize):
    """The same statement as a plain loop over destination pixels on Python floats and ints (IEEE doubles, each operation rounded;
    round() is half to even); Mi is the inverse map."""
    H, W = img.shape[:2]
    h, w = dsize
    m = [float(v) for v in np.asarray(Mi, np.float64).reshape(9)]
    bh0 = min(16, h)
    bw0 = min(1024 // bh0, w)
    out = np.zeros((h, w) + img.shape[2:], np.uint8)
    flat = img.reshape(H, W, -1)
    res = out.reshape(h, w, -1)
    for y in range(h):
        for x in range(w):
            xb = (x // bw0) * bw0
            x1 = x - xb
            X0 = (m[0] * xb + m[1] * y) + m[2]
            Y0 = (m[3] * xb + m[4] * y) + m[5]
            W0 = (m[6] * xb + m[7] * y) + m[8]
            Wd = W0 + m[6] * x1
            Wd = 32.0 / Wd if Wd != 0 else 0.0
            fX = max(INT_MIN, min(INT_MAX, (X0 + m[0] * x1) * Wd))
            fY = max(INT_MIN, min(INT_MAX, (Y0 + m[3] * x1) * Wd))
            X, Y = round(fX), round(fY)
            sx, sy = max(-32768, min(32767, X >> 5)), max(-32768, min(32767, Y >> 5))
            ax, ay = X & 31, Y & 31
            for c in range(flat.shape[2]):
                acc = 0
                for dy, wy in ((0, 32 - ay), (1, ay)):
                    for dx, wx in ((0, 32 - ax), (1, ax)):
                        if 0 <= sx + dx < W and 0 <= sy + dy < H:
                            acc += wx * wy * int(flat[sy + dy, sx + dx, c])
                res[y, x, c] = (acc + 512) >> 10
    return out
