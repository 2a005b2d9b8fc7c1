"""Cases and seeded input makers of the fused resize / score / encode path (pwc_pil_flow_eval), shared by
tools/gen_golden_inference_eval.py, tests/test_inference_eval_cpu.py and tests/test_gpu_inference_eval.py.  The inputs are made
here from seeds, so the fixture tests/golden/g22_inference_eval.npz holds the reference's RESULTS only.

Inputs: the network-resolution flow is N(0, 1.5) px of noise around (+20, -20) px, so the resized and rescaled prediction stays far
inside +-512 px.  The ground truth is that prediction (pil_resize_oracle.resize_flow, which the fixture pins to the reference's own
resize_flow bit for bit) plus N(0, 2) px per component -- end-point errors on both sides of 3 px -- with about 30 % of the pixels
multiplied by 4 so that |gt| is large enough for the relative threshold to rule, clipped to +-500 px and rounded to 1/64 px, the
PNG's step.  About 70 % of the pixels are valid."""
import numpy as np

import pil_resize_oracle as R

# name -> (B, network-resolution (h, w), original (H, W), seed): the smallest shapes at which each thing can go wrong
CASES = {
    "tile_edges": (2, (6, 20), (17, 65), 2201),       # one pixel past the 16 x 64 tile on both axes; odd W: rows of the uint16 arrays 2-byte aligned
    "one_tile": (1, (4, 16), (16, 64), 2202),         # a single full tile
    "down": (2, (40, 150), (15, 63), 2203),           # a downscale with wide taps
    "x_unchanged": (1, (5, 33), (19, 33), 2204),      # copy instantiation (x)
    "y_unchanged": (1, (9, 12), (9, 70), 2205),       # copy instantiation (y)
    "identity": (1, (7, 9), (7, 9), 2206),            # both axes copied
    "one_px": (1, (3, 5), (1, 1), 2207),              # one output pixel
    "kitti_like": (3, (24, 80), (94, 311), 2208),     # inference.py's 96 x 320 -> 375 x 1242 at a quarter: 6 x 5 tiles, 3 samples
    "tall": (1, (250, 2), (100, 5), 2209),            # Pillow's vertical-first order (through the wrapper)
}
# the relative threshold cannot rule where 4 x |prediction| stays under 60 px
NO_RELATIVE = ("down", "one_px")
SMALL = 20000            # cases whose flow has at most this many elements are stored as arrays, the others as digests


def make_flow(name):
    """float32 [B,2,h,w]: the network's output."""
    B, (h, w), _, seed = CASES[name]
    rng = np.random.RandomState(seed)
    f = rng.randn(B, 2, h, w) * 1.5
    f[:, 0] += 20.0
    f[:, 1] -= 20.0
    return f.astype(np.float32)


def make_gt(name, pred=None):
    """(gt float32 [B,H,W,2], valid bool [B,H,W]) around `pred` [B,2,H,W] (default: the oracle's resize of make_flow)."""
    B, _, (H, W), seed = CASES[name]
    if pred is None:
        pred = R.resize_flow(make_flow(name), (H, W))
    rng = np.random.RandomState(seed + 5000)
    gt = pred.transpose(0, 2, 3, 1).astype(np.float64) + rng.randn(B, H, W, 2) * 2.0
    gt = np.where(rng.rand(B, H, W, 1) < 0.3, gt * 4.0, gt)
    gt = (np.round(np.clip(gt, -500.0, 500.0) * 64.0) / 64.0).astype(np.float32)
    valid = rng.rand(B, H, W) < 0.7
    if name == "one_px":
        valid[...] = True
    return gt, valid


def gt_u16(gt, valid, order):
    """The ground truth as PNG samples uint16 [B,H,W,3]: "kitti" = {u, v, valid}, "reference" = {valid, v, u}; exact, since gt is a
    multiple of 1/64 inside +-512."""
    e = np.round(gt.astype(np.float64) * 64.0 + 32768.0)
    assert e.min() >= 0 and e.max() <= 65535
    u, v, ok = e[..., 0].astype(np.uint16), e[..., 1].astype(np.uint16), valid.astype(np.uint16)
    return np.ascontiguousarray(np.stack([u, v, ok] if order == "kitti" else [ok, v, u], axis=-1))


_CACHE = {}


def case(name):
    """(flow, pred, gt, valid, score) of one case: the inputs, the oracle's prediction and inference_eval_oracle.score's totals,
    computed once per session, read-only."""
    if name not in _CACHE:
        import inference_eval_oracle as O
        flow = make_flow(name)
        pred = O.predict(flow, CASES[name][2])
        gt, valid = make_gt(name, pred)
        for a in (flow, pred, gt, valid):
            a.setflags(write=False)
        _CACHE[name] = (flow, pred, gt, valid, O.score(pred, gt, valid))
    return _CACHE[name]
