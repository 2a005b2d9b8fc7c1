"""fp64 NumPy restatement of the supervised losses of train.py / train2.py (forward and the gradient w.r.t. the flows), for the
tests: an oracle independent of torch's interpolate / grid_sample and of the HIP kernels.

Index arithmetic is torch's, in float32 (the kernels and torch agree on it; see include/pwc_hip.h):
  bilinear, align_corners=False: scale = f32(in) / f32(out); s = max(scale * (f32(dst) + 0.5) - 0.5, 0); i0 = int(s);
  i1 = i0 + (i0 < in-1); l1 = s - i0; l0 = 1 - l1.   nearest: min(floor(f32(dst) * scale), in-1).
Everything after the indices and weights is float64.  The interpolations are matrices: up = A_y f A_x^T, adjoint A_y^T g A_x.
"""
import numpy as np

F32 = np.float32


def linear_taps(n_in, n_out):
    """(i0, i1, l0, l1) per output index of torch's align_corners=False bilinear resize n_in -> n_out."""
    scale = F32(n_in) / F32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    s = scale * (dst + F32(0.5)) - F32(0.5)
    s = np.maximum(s, F32(0.0))
    i0 = s.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(np.float32)
    l0 = F32(1.0) - l1
    return i0, i1, l0.astype(np.float64), l1.astype(np.float64)


def nearest_index(n_in, n_out):
    scale = F32(n_in) / F32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def interp_matrix(n_in, n_out):
    i0, i1, l0, l1 = linear_taps(n_in, n_out)
    A = np.zeros((n_out, n_in))
    r = np.arange(n_out)
    np.add.at(A, (r, i0), l0)
    np.add.at(A, (r, i1), l1)
    return A


def resize(x, H, W):
    """[..., h, w] -> [..., H, W], torch's bilinear align_corners=False (either direction)."""
    Ay, Ax = interp_matrix(x.shape[-2], H), interp_matrix(x.shape[-1], W)
    return Ay @ x.astype(np.float64) @ Ax.T


def _plane(mask):
    if mask is None:
        return None
    m = np.asarray(mask, dtype=np.float64)
    return m[:, 0] if m.ndim == 4 else m


def flow_loss(pred, gt, mask=None, eps=1e-3, rule="threshold"):
    """(loss, d loss / d pred) of MaskedCharbonnier (rule "threshold") or compute_epe (rule "raw", eps 0) of pred [B,2,h,w]
    upsampled to gt [B,2,H,W] (vectors * W/w, H/h)."""
    pred, gt = np.asarray(pred, np.float64), np.asarray(gt, np.float64)
    B, _, H, W = gt.shape
    h, w = pred.shape[-2:]
    Ay, Ax = interp_matrix(h, H), interp_matrix(w, W)
    sc = np.array([float(F32(W / w)), float(F32(H / h))]).reshape(1, 2, 1, 1)
    up = (Ay @ pred @ Ax.T) * sc
    d = up - gt
    epe = np.sqrt((d ** 2).sum(1) + eps ** 2)
    m = _plane(mask)
    if m is None:
        m = np.ones((B, H, W))
    elif rule == "threshold":
        m = (m > 0.5).astype(np.float64)
    den = (max(m.sum(), 1.0) if rule == "threshold" else m.sum() + 1e-8) if mask is not None else float(B * H * W)
    loss = (epe * m).sum() / den
    with np.errstate(divide="ignore", invalid="ignore"):
        gfull = np.where(m[:, None] != 0, d / epe[:, None] * m[:, None], 0.0) / den
    grad = Ay.T @ (gfull * sc) @ Ax
    return loss, grad


def _sample_zeros(img, ix, iy):
    """grid_sample(bilinear, zeros, align_corners=True) of img [C,h,w] at pixel coordinates (ix, iy) [h,w]; value and slopes."""
    C, h, w = img.shape
    x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
    tx, ty = ix - x0, iy - y0

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(ok[None], img[:, np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], 0.0)

    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    val = (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 + tx * v11)
    sx = (1 - ty) * (v01 - v00) + ty * (v11 - v10)
    sy = (1 - tx) * (v10 - v00) + tx * (v11 - v01)
    return val, sx, sy


def multiscale_loss(preds, images, gt, mask, w=None, lambda_photo=0.0, lambda_smooth=0.0, eps=1e-3):
    """(total, [d total / d pred_l]) of supervised_multiscale_loss (train2.py:124-167)."""
    if w is None or len(w) == 0:
        w = [0.32, 0.08, 0.02, 0.01, 0.005]
    gt = np.asarray(gt, np.float64)
    B, _, H, W = gt.shape
    m_full = _plane(mask) if mask is not None else np.ones((B, H, W))
    total, grads = 0.0, []
    for li, pred in enumerate(preds):
        pred = np.asarray(pred, np.float64)
        h, w_ = pred.shape[-2:]
        wl = w[li] if li < len(w) else w[-1]
        inv = np.array([float(F32(1.0) / F32(W / w_)), float(F32(1.0) / F32(H / h))]).reshape(1, 2, 1, 1)
        gt_s = resize(gt, h, w_) * inv
        ms = m_full[:, nearest_index(H, h)][:, :, nearest_index(W, w_)]
        d = pred - gt_s
        epe = np.sqrt((d ** 2).sum(1) + eps ** 2)
        valid = (ms > 0.5).astype(np.float64)
        den_c = max(valid.sum(), 1.0)
        lvl = (epe * valid).sum() / den_c
        g = d / epe[:, None] * valid[:, None] / den_c
        if lambda_photo > 0 or lambda_smooth > 0:
            ims = resize(np.asarray(images, np.float64), h, w_)
            im1, im2 = ims[:, :3], ims[:, 3:]
            yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w_, dtype=np.float64), indexing="ij")
            if lambda_photo > 0:
                den_p = ms.sum() + 1e-8
                ph = 0.0
                for b in range(B):
                    val, sx, sy = _sample_zeros(im2[b], xx + pred[b, 0], yy + pred[b, 1])
                    r = im1[b] - val
                    ph += (np.abs(r) * ms[b][None]).sum()
                    gw = -np.sign(r) * ms[b][None] / den_p * lambda_photo
                    g[b, 0] += (gw * sx).sum(0)
                    g[b, 1] += (gw * sy).sum(0)
                lvl += lambda_photo * ph / den_p
            if lambda_smooth > 0:
                ex = np.exp(-np.abs(im1[:, :3, :, :-1] - im1[:, :3, :, 1:]).mean(1, keepdims=True))
                ey = np.exp(-np.abs(im1[:, :3, :-1, :] - im1[:, :3, 1:, :]).mean(1, keepdims=True))
                dx, dy = pred[:, :, :, :-1] - pred[:, :, :, 1:], pred[:, :, :-1, :] - pred[:, :, 1:, :]
                lvl += lambda_smooth * ((np.abs(dx) * ex).mean() + (np.abs(dy) * ey).mean())
                tx = np.sign(dx) * ex * lambda_smooth / dx.size
                ty = np.sign(dy) * ey * lambda_smooth / dy.size
                g[:, :, :, :-1] += tx
                g[:, :, :, 1:] -= tx
                g[:, :, :-1, :] += ty
                g[:, :, 1:, :] -= ty
        total += wl * lvl
        grads.append(g * wl)
    return total, grads
