"""Ragged cases of the supervised losses (csrc/pwc_sup_loss.hip) and the comparators their GPU tests use.  A helper, not a test
module: tests/test_supervised_loss_cases_cpu.py pins the conditions on the inputs under which a passing GPU test means something
and shows that every comparator can fail; tests/test_gpu_supervised_loss_edges.py runs the kernels on the cases against the fp64
oracle (tests/supervised_loss_oracle.py).

tests/test_gpu_supervised_loss.py runs the oracle at the g10 fixture (at most 768 pixels per level) and at training sizes (whole
1024-pixel chunks, ratios 4, 3.9, 4.1 and 1), always with an upstream gradient of 1, dense operands and all terms summed.  The
geometries here are the smallest at which each path of the kernels can still go wrong.

Flow-loss cases (B, H, W, h, w), FLOW_CASES:
  tail-1        2 x 17 x 65 from 5 x 17: ratios 3.4 / 3.82; the image boundary falls inside a chunk; the last chunk holds 162 px
  chunk-exact   1 x 32 x 32 from 8 x 8: B H W = 1024, one whole chunk
  chunk-plus-1  1 x 25 x 41 from 5 x 9: 1025, the second chunk holds one pixel
  same          1 x 15 x 63 at full size: the path without upsampling
  min-2x2       2 x 2 x 2 from 2 x 2: the smallest accepted call
  min-3-from-2  1 x 3 x 3 from 2 x 2: the smallest upsampling call
  coarse-2x2    1 x 40 x 130 from 2 x 2: four gather lanes walk the whole image
  near-1        1 x 33 x 70 from 32 x 69: first_user's estimate and both of its walks
  row-same      2 x 24 x 96 from 24 x 24: rh = 1.0 with w < W
  col-same      2 x 24 x 96 from 6 x 96: rw = 1.0 with h < H
Settings (FLOW_SETTINGS): rule "threshold" (MaskedCharbonnier, eps 1e-3) with no mask, a random binary mask, the "edge" mask
(only the last row and column valid) and "off" (all zero: the clamp, an exactly zero gradient); rule "raw" (compute_epe, eps 0)
with no mask and with a fractional mask a fifth of which is exactly 0.  The ground truth is the scaled upsampled prediction plus
an offset of 3 to 5 pixels (6 to 8 in the last row and column) in a random direction, so the end-point error is nowhere near 0.

Multiscale cases (B, H, W, levels, weights), MS_CASES:
  ms-ragged     2 x 37 x 83; (10,21) (5,11) (3,6) (2,3): every level one partial chunk; non-integer bilinear and nearest ratios
  ms-chunks     1 x 64 x 96; (32,32) (25,41) (64,96) (2,2): 1024 then 1025 pixels, a full-resolution level, not in decreasing order
  ms-chunks-b2  the same at B = 2, for the batch-strided test (a batch stride means nothing at B = 1)
  ms-8          1 x 40 x 56; (40,56) (20,28) (13,19) (10,14) (7,9) (5,7) (3,4) (2,2), the default five weights: kMaxLevels, and
                w[-1] reused for levels 5 to 7
  ms-8w         ms-8 with eight distinct weights: a level table that mixed up weights past the fifth would show
  ms-1          2 x 17 x 65; one 5 x 17 tensor, not a list: L = 1
  ms-64         1 x 128 x 192; (2,3): ratio 64
  ms-twins      1 x 12 x 20; (6,10) (6,10) with different contents and weights: two levels that could be taken for each other
Term settings (TERMS): "charb" (both lambdas 0, a binary mask), "photo" (mask 0.4 everywhere, lambda_photo 0.4: no pixel is valid,
the Charbonnier denominator is clamped and the gradient is the photometric term's alone), "smooth" (mask 0, lambda_smooth 0.2) and
"all" (a fractional random mask, a fifth of it exactly 0, both lambdas on).  Images: the smooth sines of
test_multiscale_regularisers_vs_oracle plus noise.  Predictions ("rough") are in level pixels: a pull towards the level's centre
plus noise of twice its size, so most photometric samples land inside the level and some outside on each side.  Two more
prediction kinds give exact zeros: "const" (one vector everywhere: the smoothness gradient is 0) and "oob" (a flow larger than
the level: every photometric tap is padding, the photometric gradient is 0 and the photometric loss is that of a black im2).

What was chosen and nudged so that the conditions of tests/test_supervised_loss_cases_cpu.py hold with no element left out of any
comparison:
  - flow cases: the GT offset is 3 px longer in the last image row and column, so that they stand out of the mean (condition f);
  - multiscale GT: smooth sines plus 0.3 px of noise.  The level's GT is a bilinear sample of it; under noise of several pixels
    the float32 rounding of the sample coordinate (the kernels' and the oracle's, not torch's float64 resize) showed in d / epe
    at 4e-5 of max|g| against the torch route;
  - multiscale predictions: the last row and column of every level are pulled inwards by another 0.9 of the noise's size and
    im1 alone brightens towards the bottom and the right, so that Charbonnier, photometric and smoothness terms of the last row
    and column stand out of the level's mean (f); every pixel is kept 0.75 px from the level's GT (the Charbonnier slope d / epe
    is then well conditioned); then a pixel whose photometric sample lies within 2e-3 of an integer coordinate (a), whose
    residual |im1_s - warped| is under 2e-4 max|img| in a channel (b), or which differs from a neighbour by less than 2e-4
    without being equal to it (c), is moved by 0.013 (then 0.026, ...) in both components until none is left (_nudge);
  - masks: fractional values within 0.01 of 0.5 are moved to 0.49 / 0.51 (d); in the binary and fractional masks of the
    multiscale cases the pixels that the last row and the last column of any level read are on (f);
  - ms-8w: its seed was moved on by one (RESEED), the smoothness loss of one level having sat at 9.5 bounds under (f).
The conditions are then computed afresh from the final inputs, on the fp64 oracle's quantities alone (conditions(),
flow_sensitivity(), ms_sensitivity()).  Condition (f) for a multiscale case is stated per level on what the level's last row
(column) reads, since only a full-resolution level reads the last image row: see ms_sensitivity.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import supervised_loss_oracle as O

NAN = float("nan")
CHUNK = 1024                                  # pixels per workgroup (kChunk of the kernels)
MAX_LEVELS = 8                                # kMaxLevels
DEFAULT_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)

FlowCase = namedtuple("FlowCase", "B H W h w")
FLOW_CASES = {
    "tail-1": FlowCase(2, 17, 65, 5, 17),
    "chunk-exact": FlowCase(1, 32, 32, 8, 8),
    "chunk-plus-1": FlowCase(1, 25, 41, 5, 9),
    "same": FlowCase(1, 15, 63, 15, 63),
    "min-2x2": FlowCase(2, 2, 2, 2, 2),
    "min-3-from-2": FlowCase(1, 3, 3, 2, 2),
    "coarse-2x2": FlowCase(1, 40, 130, 2, 2),
    "near-1": FlowCase(1, 33, 70, 32, 69),
    "row-same": FlowCase(2, 24, 96, 24, 24),
    "col-same": FlowCase(2, 24, 96, 6, 96),
}
# (rule, eps, mask kind)
FLOW_SETTINGS = (("threshold", 1e-3, None), ("threshold", 1e-3, "binary"), ("threshold", 1e-3, "edge"), ("threshold", 1e-3, "off"),
                 ("raw", 0.0, None), ("raw", 0.0, "frac"))

MsCase = namedtuple("MsCase", "B H W levels w one_tensor")
_L8 = ((40, 56), (20, 28), (13, 19), (10, 14), (7, 9), (5, 7), (3, 4), (2, 2))
MS_CASES = {
    "ms-ragged": MsCase(2, 37, 83, ((10, 21), (5, 11), (3, 6), (2, 3)), None, False),
    "ms-chunks": MsCase(1, 64, 96, ((32, 32), (25, 41), (64, 96), (2, 2)), None, False),
    "ms-chunks-b2": MsCase(2, 64, 96, ((32, 32), (25, 41), (64, 96), (2, 2)), None, False),
    "ms-8": MsCase(1, 40, 56, _L8, None, False),
    "ms-8w": MsCase(1, 40, 56, _L8, (0.32, 0.08, 0.02, 0.01, 0.005, 0.004, 0.003, 0.002), False),
    "ms-1": MsCase(2, 17, 65, ((5, 17),), None, True),
    "ms-64": MsCase(1, 128, 192, ((2, 3),), None, False),
    "ms-twins": MsCase(1, 12, 20, ((6, 10), (6, 10)), (0.3, 0.1), False),
}
# term -> (mask kind, lambda_photo, lambda_smooth)
TERMS = {"charb": ("binary", 0.0, 0.0), "photo": ("0.4", 0.4, 0.0), "smooth": ("zero", 0.0, 0.2), "all": ("frac", 0.4, 0.2)}
MS_EPS = 1e-3                                 # MaskedCharbonnier's default, the only one supervised_multiscale_loss uses
# (case, term, prediction kind) of the exact-zero checks
ZERO_KINDS = (("ms-ragged", "smooth", "const"), ("ms-8", "smooth", "const"), ("ms-ragged", "photo", "oob"), ("ms-chunks", "photo", "oob"))

LOSS_RTOL, LOSS_ATOL = 1e-5, 1e-9             # _close_loss of test_gpu_supervised_loss.py
GRAD_TOL = 1e-4                               # of max|g_ref|, per level: _close_grad of test_gpu_supervised_loss.py
SENSITIVITY = 10.0                            # condition (f): in units of the bound the quantity is compared under
COORD_MARGIN, RESID_MARGIN, DIFF_MARGIN, MASK_MARGIN = 1e-3, 1e-4, 1e-4, 1e-3      # conditions (a), (b), (c), (d)


def geometry_ok(H, W, h, w):
    """The kernels' acceptance rule (geometry_ok of pwc_sup_loss.hip, ops._sup_geometry_ok): 2 <= h <= H and 2 <= w <= W."""
    return 2 <= h <= H and 2 <= w <= W


def blocks_of(n):
    return -(-n // CHUNK)


def blk0(name):
    """First workgroup of every level in the flattened grid, and the grid's size."""
    c = MS_CASES[name]
    n = [blocks_of(c.B * h * w) for h, w in c.levels]
    return [sum(n[:k]) for k in range(len(n))], sum(n)


def level_weights(name):
    """One weight per level, as supervised_multiscale_loss hands them to the kernel: w[i], w[-1] past the end of w."""
    c = MS_CASES[name]
    w = list(DEFAULT_WEIGHTS if c.w is None else c.w)
    return tuple(float(w[i] if i < len(w) else w[-1]) for i in range(len(c.levels)))


RESEED = {"ms-8w": 1}        # seeds moved on until condition (f) held (one level's smoothness loss sat at 9.5 bounds)


def _seed(table, name):
    return 1000 + 10 * list(table).index(name) + (500 if table is MS_CASES else 0) + RESEED.get(name, 0)


def _ro(a):
    a.setflags(write=False)
    return a


# ---------------------------------------------------------------- masks
def _frac_mask(rng, shape):
    """Uniform values, a fifth of them exactly 0, none within 0.01 of 0.5 (condition d)."""
    m = rng.random(shape).astype(np.float32)
    near = np.abs(m - 0.5) < 0.01
    m[near] = np.where(m[near] < 0.5, np.float32(0.49), np.float32(0.51))
    m[rng.random(shape) < 0.2] = 0.0
    return m


def _mask(kind, seed, B, H, W):
    """float32 [B,H,W] values of a mask kind (None: no mask)."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    if kind == "binary":
        m = (rng.random((B, H, W)) > 0.4).astype(np.float32)
    elif kind == "edge":
        m = np.zeros((B, H, W), np.float32)
        m[:, H - 1, :] = 1.0
        m[:, :, W - 1] = 1.0
    elif kind in ("off", "zero"):
        m = np.zeros((B, H, W), np.float32)
    elif kind == "0.4":
        m = np.full((B, H, W), 0.4, np.float32)
    else:
        assert kind == "frac", kind
        m = _frac_mask(rng, (B, H, W))
    return m


def mask_forms(values):
    """[(tag, tensor)] of a 0 / 1 float32 mask [B,H,W]: float32, bool and uint8 (on = 1, every third on-pixel 255), each as
    [B,H,W] and [B,1,H,W].  The first entry is the float32 [B,H,W] one."""
    on = values > 0.5
    assert np.array_equal(on.astype(np.float32), values), "only a 0 / 1 mask has the same meaning in every dtype"
    u8 = on.astype(np.uint8)
    u8.ravel()[np.flatnonzero(on.ravel())[::3]] = 255
    B, H, W = values.shape
    return [("%s-%dd" % (tag, len(shape)), torch.from_numpy(arr.copy()).view(shape))
            for tag, arr in (("float32", values), ("bool", on), ("uint8", u8)) for shape in ((B, H, W), (B, 1, H, W))]


# ---------------------------------------------------------------- flow-loss inputs and oracle
@functools.lru_cache(maxsize=None)
def _flow_inputs(name):
    c = FLOW_CASES[name]
    rng = np.random.default_rng(_seed(FLOW_CASES, name))
    pred = (2.0 * rng.standard_normal((c.B, 2, c.h, c.w))).astype(np.float32)
    sc = np.array([float(np.float32(c.W / c.w)), float(np.float32(c.H / c.h))]).reshape(1, 2, 1, 1)
    up = O.resize(pred, c.H, c.W) * sc
    r, th = 3.0 + 2.0 * rng.random((c.B, c.H, c.W)), 2.0 * np.pi * rng.random((c.B, c.H, c.W))
    r[:, c.H - 1, :] += 3.0                     # the last row and column stand out of the mean: condition (f)
    r[:, :, c.W - 1] += 3.0
    gt = (up + np.stack((r * np.cos(th), r * np.sin(th)), 1)).astype(np.float32)
    return _ro(pred), _ro(gt)


def flow_inputs(name):
    """(pred [B,2,h,w], gt [B,2,H,W]) float32 on the CPU (fresh copies)."""
    return tuple(torch.from_numpy(a.copy()) for a in _flow_inputs(name))


@functools.lru_cache(maxsize=None)
def _flow_mask(name, kind):
    c = FLOW_CASES[name]
    m = _mask(kind, _seed(FLOW_CASES, name) + 1, c.B, c.H, c.W)
    return None if m is None else _ro(m)


def flow_mask(name, kind):
    """float32 [B,H,W] on the CPU (a fresh copy), or None."""
    m = _flow_mask(name, kind)
    return None if m is None else torch.from_numpy(m.copy())


def _flow_den(mask, rule, n):
    if mask is None:
        return float(n)
    m = mask.astype(np.float64)
    return max(float((m > 0.5).sum()), 1.0) if rule == "threshold" else float(m.sum()) + 1e-8


def _flow_result(pred, gt, mask, rule, eps):
    loss, grad = O.flow_loss(pred, gt, mask, eps=eps, rule=rule)
    return {"loss": float(loss), "den": _flow_den(mask, rule, gt.shape[0] * gt.shape[2] * gt.shape[3]), "grad": _ro(grad)}


@functools.lru_cache(maxsize=None)
def _flow_oracle(name, rule, eps, mask_kind):
    pred, gt = _flow_inputs(name)
    return _flow_result(pred, gt, _flow_mask(name, mask_kind), rule, eps)


def flow_oracle(name, rule="threshold", eps=1e-3, mask_kind=None):
    """{"loss", "den", "grad" (read-only float64 [B,2,h,w])} of the fp64 oracle, computed once per process."""
    return _flow_oracle(name, rule, float(eps), mask_kind)


def flow_min_epe(name):
    pred, gt = _flow_inputs(name)
    c = FLOW_CASES[name]
    sc = np.array([float(np.float32(c.W / c.w)), float(np.float32(c.H / c.h))]).reshape(1, 2, 1, 1)
    return float(np.sqrt(((O.resize(pred, c.H, c.W) * sc - gt) ** 2).sum(1)).min())


def flow_sensitivity(name):
    """Condition (f) for a flow case: (loss, gradient) changes of the oracle, in units of the comparators' bounds, when the last
    image row is masked out, then the last column: ((row loss, row grad), (column loss, column grad))."""
    c = FLOW_CASES[name]
    pred, gt = _flow_inputs(name)
    full = np.ones((c.B, c.H, c.W), np.float32)
    ref = _flow_result(pred, gt, full, "threshold", 1e-3)
    out = []
    for sl in ((slice(None), c.H - 1, slice(None)), (slice(None), slice(None), c.W - 1)):
        m = full.copy()
        m[sl] = 0.0
        got = _flow_result(pred, gt, m, "threshold", 1e-3)
        out.append((abs(got["loss"] - ref["loss"]) / (LOSS_ATOL + LOSS_RTOL * abs(ref["loss"])),
                    float(np.abs(got["grad"] - ref["grad"]).max() / (GRAD_TOL * np.abs(ref["grad"]).max()))))
    return tuple(out)


# ---------------------------------------------------------------- multiscale inputs
def _level_state(pred, ims):
    """fp64 quantities of one level that conditions (a)-(c), (e) are stated on: sample coordinates, residuals, neighbour
    differences.  pred [B,2,h,w], ims [B,6,h,w] (the resized images)."""
    B, _, h, w = pred.shape
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ix, iy = xx[None] + pred[:, 0], yy[None] + pred[:, 1]
    resid = np.stack([ims[b, :3] - O._sample_zeros(ims[b, 3:], ix[b], iy[b])[0] for b in range(B)])      # [B,3,h,w]
    return ix, iy, resid, pred[:, :, :, :-1] - pred[:, :, :, 1:], pred[:, :, :-1, :] - pred[:, :, 1:, :]


def _violators(pred, ims, amax, k):
    """bool [B,h,w]: prediction pixels that miss k times the margin of condition (a), (b) or (c)"""
    ix, iy, resid, dx, dy = _level_state(pred.astype(np.float64), ims)
    bad = (np.abs(ix - np.round(ix)) < k * COORD_MARGIN) | (np.abs(iy - np.round(iy)) < k * COORD_MARGIN)
    bad |= (np.abs(resid) < k * RESID_MARGIN * amax).any(1)
    sx, sy = ((dx != 0) & (np.abs(dx) < k * DIFF_MARGIN)).any(1), ((dy != 0) & (np.abs(dy) < k * DIFF_MARGIN)).any(1)
    bad[:, :, :-1] |= sx
    bad[:, :-1, :] |= sy
    return bad


def _nudge(pred, ims, amax):
    for step in range(1, 20):
        bad = _violators(pred, ims, amax, 2.0)
        if not bad.any():
            return pred
        pred = pred + np.float32(0.013 * step) * bad[:, None].astype(np.float32)
    raise AssertionError("the nudge did not settle")


@functools.lru_cache(maxsize=None)
def _ms_common(name):
    """(images [B,6,H,W], gt [B,2,H,W]) float32, and the fp64 resized images of every level"""
    c = MS_CASES[name]
    rng = np.random.default_rng(_seed(MS_CASES, name))
    yy, xx = np.meshgrid(np.arange(c.H, dtype=np.float64), np.arange(c.W, dtype=np.float64), indexing="ij")
    img = np.stack([np.sin(0.11 * (ch + 1) * xx + 0.07 * yy + ch) for ch in range(6)])[None]
    img = img + 0.1 * rng.standard_normal((c.B, 6, c.H, c.W))
    # im1 alone brightens towards the bottom and the right: the photometric residual of a level's last row and column stands
    # out of the level's mean (condition f)
    img[:, :3] += 0.8 * ((yy / (c.H - 1)) ** 6 + (xx / (c.W - 1)) ** 6)
    img = img.astype(np.float32)
    # a smooth GT with a little noise, as flow is: the level's GT is a bilinear sample of it, and under noise of several pixels
    # the float32 rounding of the sample coordinate (which torch's float64 resize does not have) would show in d / epe
    gt = np.stack((7.0 + 4.0 * np.sin(0.05 * xx + 0.08 * yy), -5.0 + 4.0 * np.cos(0.07 * xx - 0.04 * yy)))[None]
    gt = (gt + 0.3 * rng.standard_normal((c.B, 2, c.H, c.W))).astype(np.float32)
    ims = tuple(_ro(O.resize(img, h, w)) for h, w in c.levels)
    return _ro(img), _ro(gt), ims


def _inv_scale(c, h, w):
    """1 / (W / w, H / h) as the reference divides the level's GT: float32 reciprocals"""
    return np.array([float(np.float32(1.0) / np.float32(c.W / w)), float(np.float32(1.0) / np.float32(c.H / h))]).reshape(1, 2, 1, 1)


@functools.lru_cache(maxsize=None)
def _ms_preds(name, kind="rough"):
    c = MS_CASES[name]
    img, gt, ims = _ms_common(name)
    amax = float(np.abs(img).max())
    rng = np.random.default_rng(_seed(MS_CASES, name) + 1)
    out = []
    for li, (h, w) in enumerate(c.levels):
        if kind == "const":
            p = np.empty((c.B, 2, h, w), np.float32)
            p[:, 0], p[:, 1] = 0.37 + li, -0.21
        elif kind == "oob":
            p = np.empty((c.B, 2, h, w), np.float32)
            p[:, 0], p[:, 1] = w + 3.25, -(h + 3.25)            # past the right edge from every column, above the top from every row
        else:
            assert kind == "rough", kind
            ax, ay = min(0.3 * w, 1.7), min(0.3 * h, 1.7)
            yn, xn = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
            pull = np.stack((ax * (0.5 - xn), ay * (0.5 - yn)))[None]           # half the noise's size at the border, inward
            p = pull + np.array([ax, ay]).reshape(1, 2, 1, 1) * rng.standard_normal((c.B, 2, h, w))
            p[:, 1, h - 1, :] -= 0.9 * ay         # the last row and column stand out of the level's mean, inwards: condition (f)
            p[:, 0, :, w - 1] -= 0.9 * ax
            d = p - O.resize(gt, h, w) * _inv_scale(c, h, w)                    # kept 0.75 px from the level's GT: the
            n = np.sqrt((d ** 2).sum(1, keepdims=True))                         # Charbonnier slope d / epe is well conditioned
            p = (p + d / n * np.maximum(0.75 - n, 0.0)).astype(np.float32)
            p = _nudge(p, ims[li], amax)
        out.append(_ro(p))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _ms_mask(name, term):
    c = MS_CASES[name]
    m = _mask(TERMS[term][0], _seed(MS_CASES, name) + 2, c.B, c.H, c.W)
    if TERMS[term][0] in ("binary", "frac"):
        # what the last row and the last column of every level read is on, so that taking it away shows (condition f)
        for h, w in c.levels:
            ys, xs = O.nearest_index(c.H, h), O.nearest_index(c.W, w)
            m[:, ys[-1], xs] = 1.0
            m[:, ys, xs[-1]] = 1.0
    return _ro(m)


def ms_inputs(name, term, kind="rough"):
    """(preds [float32 [B,2,h,w]], images [B,6,H,W], gt [B,2,H,W], mask float32 [B,H,W], lambda_photo, lambda_smooth) on the
    CPU, fresh copies."""
    img, gt, _ = _ms_common(name)
    t = lambda a: torch.from_numpy(a.copy())                                    # noqa: E731
    return [t(p) for p in _ms_preds(name, kind)], t(img), t(gt), t(_ms_mask(name, term)), TERMS[term][1], TERMS[term][2]


def _ms_result(preds, img, gt, mask, weights, lp, ls):
    H, W = gt.shape[-2:]
    total, grads = O.multiscale_loss(preds, img, gt, mask, list(weights), lp, ls, MS_EPS)
    m = mask.astype(np.float64)
    levels, den_c, den_p = [], [], []
    for p in preds:
        h, w = p.shape[-2:]
        levels.append(float(O.multiscale_loss([p], img, gt, mask, [1.0], lp, ls, MS_EPS)[0]))
        ms = m[:, O.nearest_index(H, h)][:, :, O.nearest_index(W, w)]
        den_c.append(max(float((ms > 0.5).sum()), 1.0))
        den_p.append(float(ms.sum()) + 1e-8)
    return {"total": float(total), "levels": np.array(levels), "den_c": np.array(den_c), "den_p": np.array(den_p),
            "grads": [_ro(np.ascontiguousarray(g)) for g in grads], "photo_on": lp > 0}


def ms_oracle(name, term, kind="rough"):
    """{"total", "levels" [L], "den_c" [L], "den_p" [L], "grads" (read-only float64 [B,2,h,w] per level), "photo_on"} of the fp64
    oracle, computed once per process.  Level losses are the oracle's total of the level alone with weight 1."""
    return _ms_oracle(name, term, kind)


@functools.lru_cache(maxsize=None)
def _ms_oracle(name, term, kind):
    img, gt, _ = _ms_common(name)
    return _ms_result(list(_ms_preds(name, kind)), img, gt, _ms_mask(name, term), level_weights(name), TERMS[term][1], TERMS[term][2])


# ---------------------------------------------------------------- conditions on the multiscale inputs
def conditions(name):
    """Conditions (a)-(e) of a multiscale case with the rough predictions, on fp64 quantities alone:
      coord   (a) least distance of a photometric sample coordinate from an integer
      resid   (b) least |im1_s - warped| over every (pixel, channel), over max|img| (every pixel: the mask's support or not)
      diff    (c) least non-zero |neighbour difference| of a prediction that the smoothness term reads
      mask    (d) least |m - 0.5| over the raw values of the case's four masks
      taps    (e) (photometric taps inside the level, taps outside it); sides: samples past the (left, right, top, bottom) edge
      epe     least |pred - gt_s| over every level: the Charbonnier slope d / epe is far from its kink"""
    c = MS_CASES[name]
    img, gt, ims = _ms_common(name)
    amax = float(np.abs(img).max())
    coord = resid = diff = epe = np.inf
    inside = outside = 0
    sides = np.zeros(4, np.int64)
    for li, p in enumerate(_ms_preds(name)):
        h, w = p.shape[-2:]
        ix, iy, r, dx, dy = _level_state(p.astype(np.float64), ims[li])
        coord = min(coord, np.abs(ix - np.round(ix)).min(), np.abs(iy - np.round(iy)).min())
        resid = min(resid, np.abs(r).min() / amax)
        for d in (dx, dy):
            if (d != 0).any():
                diff = min(diff, np.abs(d[d != 0]).min())
        x0, y0 = np.floor(ix), np.floor(iy)
        for ty in (y0, y0 + 1):
            for tx in (x0, x0 + 1):
                ok = (tx >= 0) & (tx < w) & (ty >= 0) & (ty < h)
                inside += int(ok.sum())
                outside += int((~ok).sum())
        sides += np.array([(ix < 0).sum(), (ix > w - 1).sum(), (iy < 0).sum(), (iy > h - 1).sum()])
        epe = min(epe, np.sqrt(((p.astype(np.float64) - O.resize(gt, h, w) * _inv_scale(c, h, w)) ** 2).sum(1)).min())
    mask = min(float(np.abs(_ms_mask(name, t).astype(np.float64) - 0.5).min()) for t in TERMS)
    return {"coord": float(coord), "resid": float(resid), "diff": float(diff), "mask": mask, "taps": (inside, outside),
            "sides": tuple(int(s) for s in sides), "epe": float(epe)}


def ms_sensitivity(name, term):
    """Condition (f) for a multiscale case and term setting: per level, the (loss, gradient) changes of the oracle's result for
    that level alone, in units of the comparators' bounds, when what its last row reads is taken away, then its last column:
    [((row loss, row grad), (column loss, column grad)) per level].  Only a full-resolution level reads the last image row; a
    level's last row reads the mask at image row nearest_index(H, h)[-1] and the images at the bilinear taps of its last row.
    So for "charb", "photo" and "all" that mask row (column) is set to 0, and for "smooth", which reads no mask, those image
    rows (columns) of im1 are set to 0."""
    c = MS_CASES[name]
    img, gt, _ = _ms_common(name)
    mask, lp, ls = _ms_mask(name, term), TERMS[term][1], TERMS[term][2]
    out = []
    for p in _ms_preds(name):
        h, w = p.shape[-2:]
        l0, g0 = O.multiscale_loss([p], img, gt, mask, [1.0], lp, ls, MS_EPS)
        per = []
        for axis, n_in, n_out in ((1, c.H, h), (2, c.W, w)):
            m2, im2 = mask.copy(), img.copy()
            sl = [slice(None)] * 3
            if term == "smooth":
                i0, i1 = O.linear_taps(n_in, n_out)[:2]
                sl[axis] = [int(i0[-1]), int(i1[-1])]
                im2[(slice(None), slice(0, 3)) + tuple(sl[1:])] = 0.0
            else:
                sl[axis] = int(O.nearest_index(n_in, n_out)[-1])
                m2[tuple(sl)] = 0.0
            l1, g1 = O.multiscale_loss([p], im2, gt, m2, [1.0], lp, ls, MS_EPS)
            per.append((abs(l1 - l0) / (LOSS_ATOL + LOSS_RTOL * abs(l0)),
                        float(np.abs(g1[0] - g0[0]).max() / (GRAD_TOL * np.abs(g0[0]).max()))))
        out.append(tuple(per))
    return out


# ---------------------------------------------------------------- batch-strided operands
def strided_np(a, extra=37):
    """(buffer [B, n + extra] with NaN in the gap, the view of `a`'s shape into it): NumPy twin of the GPU file's _strided"""
    B, n = a.shape[0], a[0].size
    buf = np.full((B, n + extra), np.nan, a.dtype)
    buf[:, :n] = a.reshape(B, n)
    return buf, buf[:, :n].reshape(a.shape)


def read_ignoring_stride(buf, shape):
    """what a kernel that took the dense batch stride would read from the buffer of strided_np (inside the allocation)"""
    return buf.ravel()[:int(np.prod(shape))].reshape(shape)


# ---------------------------------------------------------------- comparators (pure NumPy, on downloaded arrays)
def check_loss(got, ref, what="loss"):
    """Scalars or arrays of losses / denominators within LOSS_RTOL |ref| + LOSS_ATOL each.  Returns the worst error / bound."""
    got, ref = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(ref, np.float64))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ratio = np.abs(got - ref) / (LOSS_ATOL + LOSS_RTOL * np.abs(ref))
    assert np.all(ratio <= 1.0), "%s %s, oracle %s: error / bound %s" % (what, got, ref, ratio)              # also fails on NaN
    return float(ratio.max())


def check_grad(g, gref, what="gradient", scale=1.0):
    """A gradient against scale x the oracle's: every element within GRAD_TOL of the largest entry of the reference; exactly 0
    everywhere when the reference is.  No element is left out.  Returns the worst error / bound."""
    g, gref = np.asarray(g, np.float64), np.asarray(gref, np.float64) * scale
    assert g.shape == gref.shape, (what, g.shape, gref.shape)
    gmax = np.abs(gref).max()
    if gmax == 0.0:
        assert not g.any() and not np.isnan(g).any(), "%s: the oracle's is exactly 0, %d entries are not" % (what, int(np.count_nonzero(g)))
        return 0.0
    bound = GRAD_TOL * gmax
    err = np.abs(g - gref)
    worst = float(err.max() / bound)
    assert np.all(err <= bound), ("%s: error %.3e at %s, bound %.3e (%.2f x)"                                # also fails on NaN
                                  % (what, np.nanmax(err), np.unravel_index(np.nanargmax(err), err.shape), bound, worst))
    return worst


def check_flow(res, ref, tag="", scale=1.0):
    """{"loss", "den", "grad"} of a flow-loss run against flow_oracle's; the gradient against scale x the oracle's.  Returns
    {quantity: worst error / bound}."""
    return {"loss": check_loss(res["loss"], ref["loss"], tag + " loss"), "den": check_loss(res["den"], ref["den"], tag + " den"),
            "grad": check_grad(res["grad"], ref["grad"], tag + " gradient", scale)}


def check_ms(res, ref, tag="", scale=1.0):
    """{"total", "levels", "den_c", "den_p", "grads"} of a multiscale run against ms_oracle's: total and level losses, both
    denominators of every level (the photometric one where lambda_photo > 0: without it the kernel does not sum the mask), and
    every level's gradient against scale x the oracle's, each under its own max|g|.  den_c counts pixels: an integer below 2^24,
    exact in float32 whatever the order of the sum, so it is compared for equality.  Returns {quantity: worst error / bound}."""
    L = len(ref["grads"])
    assert len(res["grads"]) == L and len(res["levels"]) == L, (tag, len(res["grads"]), L)
    worst = {"loss": max(check_loss(res["total"], ref["total"], tag + " total"),
                         check_loss(res["levels"], ref["levels"], tag + " level losses"))}
    assert np.array_equal(np.asarray(res["den_c"], np.float64), ref["den_c"]), (tag, "den_c", res["den_c"], ref["den_c"])
    worst["den"] = check_loss(res["den_p"], ref["den_p"], tag + " den_p") if ref["photo_on"] else 0.0
    worst["grad"] = max(check_grad(g, gr, "%s gradient of level %d" % (tag, l), scale)
                        for l, (g, gr) in enumerate(zip(res["grads"], ref["grads"])))
    return worst
