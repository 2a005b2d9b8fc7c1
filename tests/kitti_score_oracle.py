"""float64 oracle of the fused KITTI score kernel (csrc/pwc_kitti_score.hip), shared by the kitti-score tests.

Steps 1-4 of include/pwc_hip.h (pwc_kitti_score) restated in float64 with NumPy, every decision taken in float64 as well:
  1. pred = the top-left crop_h x crop_w of the quarter-resolution flow, align_corners bilinear interpolation to out_h x out_w,
     u * out_w / crop_w, v * out_h / crop_h (validation_oracle's `upsample` applied to the CROP, not to the whole map);
  2. ground truth from the uint16 PNG samples: u = (R - 32768) / 64, v alike, valid = B != 0 (or float planes + validity);
  3. epe = |pred - gt|, mag = |gt|, outlier when epe > max(3, 0.05 mag);
  4. per sample: sum of epe over valid pixels, number of valid pixels, number of valid outliers.
It also counts the KNIFE-EDGE pixels, the valid pixels with |epe - max(3, 0.05 mag)| < 1e-4: float32 carries epe ~ 3 with an
error of a few 1e-7 per operation (a handful of operations, inputs of magnitude up to ~100 whose interpolation rounds by ~1e-5), so on
these pixels a float32 evaluation may legitimately decide the outlier test the other way, and on no others."""
import numpy as np

from validation_oracle import _axis

KNIFE = 1e-4


def upsample_crop(flow_q, crop_h, crop_w, out_h, out_w):
    """[n,2,Hq,Wq] -> float64 [n,2,out_h,out_w]: crop, resize, rescale; the crop itself at equal size"""
    f = np.asarray(flow_q, dtype=np.float64)[:, :, :crop_h, :crop_w]
    if (crop_h, crop_w) == (out_h, out_w):
        return f.copy()
    y0, y1, ty = _axis(crop_h, out_h)
    x0, x1, tx = _axis(crop_w, out_w)
    ty, tx = ty[:, None], tx[None, :]
    rows0, rows1 = f[:, :, y0], f[:, :, y1]
    up = (1 - ty) * ((1 - tx) * rows0[..., x0] + tx * rows0[..., x1]) + ty * ((1 - tx) * rows1[..., x0] + tx * rows1[..., x1])
    up[:, 0] *= out_w / crop_w
    up[:, 1] *= out_h / crop_h
    return up


def decode(gt_u16):
    """uint16 [n,H,W,3] (R,G,B) -> float64 flow [n,2,H,W], bool valid [n,H,W]"""
    g = np.asarray(gt_u16)
    u = (g[..., 0].astype(np.float64) - 32768.0) / 64.0
    v = (g[..., 1].astype(np.float64) - 32768.0) / 64.0
    return np.stack([u, v], axis=1), g[..., 2] != 0


def score(flow_q, crop_h, crop_w, out_h, out_w, gt, valid=None):
    """gt: uint16 [n,H,W,3], or float [n,2,H,W] with `valid` [n,H,W] / None.  Returns a dict of per-sample float64 / int64 arrays:
    sum_epe, n_valid, n_outlier, knife_edge, n_relative (valid pixels whose threshold is the relative one, 0.05 mag > 3),
    epe and fl (nan for a sample without a valid pixel)."""
    pred = upsample_crop(flow_q, crop_h, crop_w, out_h, out_w)
    gt = np.asarray(gt)
    if gt.dtype == np.uint16:
        assert valid is None
        g, ok = decode(gt)
    else:
        g = gt.astype(np.float64)
        ok = np.ones(g[:, 0].shape, bool) if valid is None else np.asarray(valid).astype(bool)
    d = pred - g
    epe = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    mag = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1])
    thr = np.maximum(3.0, 0.05 * mag)
    ax = (1, 2)
    out = {"sum_epe": np.where(ok, epe, 0.0).sum(axis=ax), "n_valid": ok.sum(axis=ax).astype(np.int64),
           "n_outlier": ((epe > thr) & ok).sum(axis=ax).astype(np.int64),
           "knife_edge": ((np.abs(epe - thr) < KNIFE) & ok).sum(axis=ax).astype(np.int64),
           "n_relative": ((0.05 * mag > 3.0) & ok).sum(axis=ax).astype(np.int64)}
    with np.errstate(invalid="ignore", divide="ignore"):
        nv = out["n_valid"].astype(np.float64)
        out["epe"] = np.where(nv > 0, out["sum_epe"] / nv, np.nan)
        out["fl"] = np.where(nv > 0, 100.0 * out["n_outlier"] / nv, np.nan)
    return out
