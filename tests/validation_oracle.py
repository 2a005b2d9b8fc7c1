"""float64 oracle of the fused validation metrics (csrc/pwc_fb_metrics.hip), shared by the validation tests.

Steps 1-4 of include/pwc_hip.h (pwc_fb_metrics) restated in float64 with NumPy, every decision taken in float64 as well:
  1. a = up(flow12): align_corners bilinear interpolation of the [h,w] field to the H x W grid, x * W/w, y * H/h;
  2. (px, py) = (X + a.x, Y + a.y); out of bounds when px < 0, px > W-1, py < 0 or py > H-1;
  3. wv = bilinear sample of up(flow21) at the point clamped to the image (border mode);
  4. cycle = sum |a.x + wv.x| + |a.y + wv.y|.
It also counts the KNIFE-EDGE pixels, those whose sample point lies within 1e-3 px of one of the four image borders
(min(|px|, |px-(W-1)|, |py|, |py-(H-1)|) < 1e-3): float32 rounds px by about 6e-5 px per operation at x ~ 1000, so on these
pixels a float32 evaluation may legitimately decide the out-of-bounds test the other way, and on no others."""
import numpy as np

KNIFE = 1e-3


def _axis(n_in, n_out):
    """source index pair and upper weight of each output index (align_corners): s = i (n_in - 1) / (n_out - 1)"""
    if n_in == n_out:
        i = np.arange(n_out)
        return i, i, np.zeros(n_out)
    s = np.arange(n_out, dtype=np.float64) * (float(n_in - 1) / float(n_out - 1))
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def upsample(flow, H, W):
    """[B,2,h,w] -> float64 [B,2,H,W], vectors scaled to the larger grid; the field itself at equal size"""
    f = np.asarray(flow, dtype=np.float64)
    h, w = f.shape[-2:]
    if (h, w) == (H, W):
        return f
    y0, y1, ty = _axis(h, H)
    x0, x1, tx = _axis(w, W)
    ty, tx = ty[:, None], tx[None, :]
    rows0, rows1 = f[:, :, y0], f[:, :, y1]
    up = (1 - ty) * ((1 - tx) * rows0[..., x0] + tx * rows0[..., x1]) + ty * ((1 - tx) * rows1[..., x0] + tx * rows1[..., x1])
    up[:, 0] *= W / w
    up[:, 1] *= H / h
    return up


def sample_points(flow12, H, W):
    a = upsample(flow12, H, W)
    px = np.arange(W, dtype=np.float64)[None, None, :] + a[:, 0]
    py = np.arange(H, dtype=np.float64)[None, :, None] + a[:, 1]
    return a, px, py


def oob_count(flow12, H, W):
    """(number of out-of-bounds pixels, number of knife-edge pixels)"""
    _, px, py = sample_points(flow12, H, W)
    oob = (px < 0) | (px > W - 1) | (py < 0) | (py > H - 1)
    edge = np.minimum(np.minimum(np.abs(px), np.abs(px - (W - 1))), np.minimum(np.abs(py), np.abs(py - (H - 1))))
    return int(oob.sum()), int((edge < KNIFE).sum())


def cycle_sum(flow12, flow21, H, W):
    a, px, py = sample_points(flow12, H, W)
    g = upsample(flow21, H, W)
    ix, iy = np.clip(px, 0, W - 1), np.clip(py, 0, H - 1)
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    tx, ty = (ix - x0)[:, None], (iy - y0)[:, None]
    B = g.shape[0]
    flat = g.reshape(B, 2, H * W)

    def tap(yi, xi):
        idx = np.broadcast_to((yi * W + xi).reshape(B, 1, H * W), (B, 2, H * W))
        return np.take_along_axis(flat, idx, axis=2).reshape(B, 2, H, W)

    wv = (1 - ty) * ((1 - tx) * tap(y0, x0) + tx * tap(y0, x1)) + ty * ((1 - tx) * tap(y1, x0) + tx * tap(y1, x1))
    return float(np.abs(a + wv).sum())


def metrics(flow12, flow21, H, W):
    """dict(cycle, cycle_sum, oob, oob_count, knife_edge) in float64 / int; flow21 None: the out-of-bounds part alone"""
    f12 = np.asarray(flow12, dtype=np.float64)
    B = f12.shape[0]
    n_oob, n_edge = oob_count(f12, H, W)
    out = {"oob_count": n_oob, "oob": n_oob / float(B * H * W), "knife_edge": n_edge, "cycle_sum": 0.0, "cycle": 0.0}
    if flow21 is not None:
        out["cycle_sum"] = cycle_sum(f12, flow21, H, W)
        out["cycle"] = out["cycle_sum"] / float(B * 2 * H * W)
    return out
