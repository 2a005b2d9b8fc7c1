"""NumPy statement of what pwc_pil_flow_eval computes (include/pwc_hip.h): pil_resize_oracle.resize_flow, then the float32 metric
sequence of inference.py's compute_epe / compute_fl and save_flow's encoder.  tests/golden/g22_inference_eval.npz, made by the
reference's own functions, arbitrates between this file and the library."""
import numpy as np

import pil_resize_oracle as R

F32 = np.float32


def predict(flow, size, scale_vectors=True):
    """[B,2,h,w] float32 -> [B,2,H,W]: inference.py's resize_flow."""
    return R.resize_flow(np.asarray(flow, F32), size, scale_vectors)


def decode(gt16, order="kitti"):
    """uint16 [..,3] PNG samples -> (gt float32 [..,2], valid bool [..]): ((float)s - 32768) / 64 in float32."""
    g = np.asarray(gt16)
    iu, iv, ik = (0, 1, 2) if order == "kitti" else (2, 1, 0)
    u = (g[..., iu].astype(F32) - F32(32768.0)) / F32(64.0)
    v = (g[..., iv].astype(F32) - F32(32768.0)) / F32(64.0)
    return np.stack([u, v], axis=-1), g[..., ik] != 0


def epe_maps(pred, gt):
    """pred [B,2,H,W], gt [B,H,W,2], float32 -> (epe, mag) float32 [B,H,W], every operation rounded to float32, multiply and add
    separate: du = pu - gu; epe = sqrtf(du*du + dv*dv); mag = sqrtf(gu*gu + gv*gv)."""
    pu, pv = np.asarray(pred[:, 0], F32), np.asarray(pred[:, 1], F32)
    gu, gv = np.asarray(gt[..., 0], F32), np.asarray(gt[..., 1], F32)
    du, dv = pu - gu, pv - gv
    epe = np.sqrt(du * du + dv * dv)
    mag = np.sqrt(gu * gu + gv * gv)
    assert epe.dtype == F32 and mag.dtype == F32
    return epe, mag


def outliers_fmax(epe, mag):
    """The kernel's predicate: epe > fmaxf(3.0f, 0.05f * mag)."""
    return epe > np.maximum(F32(3.0), F32(0.05) * mag)


def outliers_reference(epe, mag):
    """The predicate as inference.py writes it: (epe > 3.0) & (epe > 0.05 * mag), on float32 arrays."""
    return (epe > 3.0) & (epe > 0.05 * mag)


def relative_ruled(mag):
    return F32(0.05) * mag > F32(3.0)


def score(pred, gt, valid=None):
    """Per-sample totals and scores of pred [B,2,H,W] against gt [B,H,W,2] / valid [B,H,W] (None = all valid): dict of sum_epe
    float64 [B] (the float32 errors added in float64), n_valid, n_outlier int64 [B], scores float32 [B,2] = {sum / n_valid,
    100 * n_outlier / n_valid} (NaN without a valid pixel), and the epe / mag maps."""
    epe, mag = epe_maps(pred, gt)
    ok = np.ones(epe.shape, bool) if valid is None else np.asarray(valid, bool)
    bad = outliers_fmax(epe, mag) & ok
    B = epe.shape[0]
    s = np.array([epe[b][ok[b]].astype(np.float64).sum() for b in range(B)], np.float64)
    nv = ok.reshape(B, -1).sum(1).astype(np.int64)
    no = bad.reshape(B, -1).sum(1).astype(np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        sc = np.stack([(s / nv).astype(F32), (100.0 * no / nv).astype(F32)], axis=1)
    sc[nv == 0] = np.nan
    return {"sum_epe": s, "n_valid": nv, "n_outlier": no, "scores": sc, "epe": epe, "mag": mag}


def encode(pred, order="reference"):
    """pred [B,2,H,W] float32 -> uint16 [B,H,W,3]: (uint16)(int)clamp(x * 64.0f + 32768.0f), truncation toward zero, the clamp to
    [0, 65535] with NaN -> 0; "reference" = {1, ev, eu}, "kitti" = {eu, ev, 1}."""
    p = np.asarray(pred, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        t = p * F32(64.0) + F32(32768.0)
        t = np.where(t > 0, np.minimum(t, F32(65535.0)), F32(0.0))
    e = np.trunc(t).astype(np.int64).astype(np.uint16)
    one = np.ones(e[:, 0].shape, np.uint16)
    return np.ascontiguousarray(np.stack([one, e[:, 1], e[:, 0]] if order == "reference" else [e[:, 0], e[:, 1], one], axis=-1))
