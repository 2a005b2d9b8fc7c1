"""fp64 oracle of the fused proxy-label loss (csrc/pwc_proxy_loss.hip), shared by the proxy-loss tests.

The kernel's sample point is restated in float32 operation by operation (include/pwc_hip.h, pwc_proxy_loss_fwd): every floor and
clip decision -- which low-resolution flow pixels and which image taps a pixel uses, and whether the border clip passes the
gradient -- is taken from that float32 restatement, as tests/launch_audit.py does for the warp taps.  All arithmetic after the
decisions runs in float64 with autograd, so the gradient is what autograd derives from the reference's expression at the
kernel's sample points: the float32 point is the oracle's point (only its derivative w.r.t. the flow is taken in float64).
The side of |x - y|'s kink is decided on the restated float32 warped value in the same way.  The
kernel's constants -- the align_corners source scales rh = (h-1)/(H-1), rw and the vector scales
W/w, H/h -- are float32 numbers (as in torch's own float32 upsampling); the oracle uses those exact values, so that it evaluates
the kernel's function rather than one whose interpolation weights differ by ~1e-5 of a low-resolution pixel."""
import numpy as np
import torch
import torch.nn.functional as F


def _lin32(n_in, n_out):
    """float32 source coordinate of each output index (align_corners): fy = rh * (float)Y."""
    r = np.float32(n_in - 1) / np.float32(n_out - 1)
    f = (r * np.arange(n_out, dtype=np.float32)).astype(np.float32)
    i0 = f.astype(np.int64)
    i1 = i0 + (i0 < n_in - 1)
    l1 = (f - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, l1, np.float32(1.0) - l1


def sample_points32(flow32: torch.Tensor, H: int, W: int):
    """float32 (px, py) [B,H,W] before the clip, in the kernel's operation order (no fused multiply-add)."""
    B, _, h, w = flow32.shape
    f = flow32.detach().to("cpu", torch.float32)
    if (h, w) == (H, W):
        up = f
    else:
        y0, y1, ly1, ly0 = (torch.from_numpy(a) for a in _lin32(h, H))
        x0, x1, lx1, lx0 = (torch.from_numpy(a) for a in _lin32(w, W))
        g = lambda yi, xi: f[:, :, yi][:, :, :, xi]                     # noqa: E731
        ly0, ly1 = ly0.view(1, 1, H, 1), ly1.view(1, 1, H, 1)
        lx0, lx1 = lx0.view(1, 1, 1, W), lx1.view(1, 1, 1, W)
        up = ly0 * (lx0 * g(y0, x0) + lx1 * g(y0, x1)) + ly1 * (lx0 * g(y1, x0) + lx1 * g(y1, x1))
        up = torch.stack((up[:, 0] * np.float32(W / w), up[:, 1] * np.float32(H / h)), dim=1)
    X = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    Y = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    return X + up[:, 0], Y + up[:, 1]


def upsample64(flow64: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Upsampled flow in float64 with the float32 restatement's index decisions (differentiable w.r.t. flow64)."""
    B, _, h, w = flow64.shape
    if (h, w) == (H, W):
        return flow64
    y0, y1, _, _ = _lin32(h, H)
    x0, x1, _, _ = _lin32(w, W)
    # the kernel's constants are float32 numbers (rh, rw, W/w, H/h): the oracle evaluates the same function, exactly
    rh, rw = float(np.float32(h - 1) / np.float32(H - 1)), float(np.float32(w - 1) / np.float32(W - 1))
    fy = rh * torch.arange(H, dtype=torch.float64, device=flow64.device)
    fx = rw * torch.arange(W, dtype=torch.float64, device=flow64.device)
    ly1 = (fy - torch.from_numpy(y0).to(flow64.device)).view(1, 1, H, 1)
    lx1 = (fx - torch.from_numpy(x0).to(flow64.device)).view(1, 1, 1, W)
    y0, y1, x0, x1 = (torch.from_numpy(a).to(flow64.device) for a in (y0, y1, x0, x1))
    g = lambda yi, xi: flow64[:, :, yi][:, :, :, xi]                    # noqa: E731
    up = (1 - ly1) * ((1 - lx1) * g(y0, x0) + lx1 * g(y0, x1)) + ly1 * ((1 - lx1) * g(y1, x0) + lx1 * g(y1, x1))
    return torch.stack((up[:, 0] * float(np.float32(W / w)), up[:, 1] * float(np.float32(H / h))), dim=1)


def warp64(img64: torch.Tensor, flow64: torch.Tensor, flow32: torch.Tensor) -> torch.Tensor:
    """img sampled at the kernel's points: floor / clip decisions from float32, values and gradients in float64."""
    B, C, H, W = img64.shape
    dev = img64.device
    px32, py32 = (t.to(dev) for t in sample_points32(flow32, H, W))
    up = upsample64(flow64, H, W)
    X = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    Y = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    # the sample point's VALUE is the kernel's float32 one (at x ~ 1000 its rounding alone is ~6e-5 px, which the loss's
    # cancelling sums would carry to ~1e-4 of the gradient); its derivative w.r.t. the flow is the exact float64 one
    px = px32.to(torch.float64) + (up[:, 0] - up[:, 0].detach())
    py = py32.to(torch.float64) + (up[:, 1] - up[:, 1].detach())
    inx, iny = (px32 > 0) & (px32 < W - 1), (py32 > 0) & (py32 < H - 1)
    ix = torch.where(inx, px, px32.clamp(0, W - 1).to(torch.float64))
    iy = torch.where(iny, py, py32.clamp(0, H - 1).to(torch.float64))
    x0 = torch.floor(px32.clamp(0, W - 1)).long()
    y0 = torch.floor(py32.clamp(0, H - 1)).long()
    tx, ty = ix - x0.to(torch.float64), iy - y0.to(torch.float64)
    ox, oy = x0 + 1 < W, y0 + 1 < H
    x1, y1 = torch.where(ox, x0 + 1, x0), torch.where(oy, y0 + 1, y0)
    flat = img64.reshape(B, C, H * W)

    def tap(yi, xi, ok):
        v = torch.gather(flat, 2, (yi * W + xi).reshape(B, 1, H * W).expand(B, C, H * W)).reshape(B, C, H, W)
        return v * ok.unsqueeze(1).to(v.dtype)

    one = torch.ones_like(ox)
    v00, v01, v10, v11 = tap(y0, x0, one), tap(y0, x1, ox), tap(y1, x0, oy), tap(y1, x1, ox & oy)
    tx, ty = tx.unsqueeze(1), ty.unsqueeze(1)
    return (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 + tx * v11)


def warp32(img: torch.Tensor, flow32: torch.Tensor) -> torch.Tensor:
    """The kernel's float32 warp restated operation by operation (bilinear as (1-ty)*((1-tx)*v00 + tx*v01) + ty*(...), taps
    past the last row / column read as 0): the warped values the loss kernel compares with img1."""
    B, C, H, W = img.shape
    dev = img.device
    px, py = (t.to(dev) for t in sample_points32(flow32, H, W))
    ix, iy = px.clamp(0, W - 1), py.clamp(0, H - 1)
    fx, fy = torch.floor(ix), torch.floor(iy)
    x0, y0 = fx.long(), fy.long()
    tx, ty = (ix - fx).unsqueeze(1), (iy - fy).unsqueeze(1)
    ox, oy = x0 + 1 < W, y0 + 1 < H
    x1, y1 = torch.where(ox, x0 + 1, x0), torch.where(oy, y0 + 1, y0)
    flat = img.detach().to(torch.float32).reshape(B, C, H * W)

    def tap(yi, xi, ok):
        v = torch.gather(flat, 2, (yi * W + xi).reshape(B, 1, H * W).expand(B, C, H * W)).reshape(B, C, H, W)
        return torch.where(ok.unsqueeze(1), v, torch.zeros_like(v))

    v00, v01, v10, v11 = tap(y0, x0, torch.ones_like(ox)), tap(y0, x1, ox), tap(y1, x0, oy), tap(y1, x1, ox & oy)
    return (1 - ty) * ((1 - tx) * v00 + tx * v01) + ty * ((1 - tx) * v10 + tx * v11)


def proxy_loss64(flow32: torch.Tensor, img1: torch.Tensor, img2: torch.Tensor, mask=None, alpha_photo=1.0, alpha_smooth=0.1,
                 eps=0.0, grad_out=(1.0, 0.0, 0.0)):
    """((total, photo, smooth) as float64, grad_flow float64 for the upstream gradients grad_out)."""
    flow64 = flow32.detach().to(torch.float64).requires_grad_(True)
    x, y2 = img1.detach().to(torch.float64), img2.detach().to(torch.float64)
    y = warp64(y2, flow64, flow32)
    mu_x, mu_y = F.avg_pool2d(x, 3, 1, 1), F.avg_pool2d(y, 3, 1, 1)
    sx = F.avg_pool2d(x * x, 3, 1, 1) - mu_x * mu_x
    sy = F.avg_pool2d(y * y, 3, 1, 1) - mu_y * mu_y
    sxy = F.avg_pool2d(x * y, 3, 1, 1) - mu_x * mu_y
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim = ((2 * mu_x * mu_y + C1) * (2 * sxy + C2)) / ((mu_x ** 2 + mu_y ** 2 + C1) * (sx + sy + C2) + eps)
    # |x - y|: the side of the kink is a decision too (|0| has gradient 0); it is taken from the kernel's float32 warped values
    sgn = torch.sign(warp32(img2, flow32) - img1.detach().to(torch.float32)).to(torch.float64)
    pm = 0.85 * torch.clamp((1 - ssim) / 2, 0, 1).mean(1) + 0.15 * (sgn * (y - x)).mean(1)
    if mask is None:
        photo = pm.mean()
    else:
        m = mask.reshape(pm.shape)
        m = (m.float() > 0.5).to(torch.float64) if m.dtype != torch.bool else m.to(torch.float64)
        photo = (pm * m).sum() / m.sum().clamp_min(1.0)
    dx = (flow64[..., :-1] - flow64[..., 1:]).abs().mean()
    dy = (flow64[..., :-1, :] - flow64[..., 1:, :]).abs().mean()
    smooth = dx + dy
    total = alpha_photo * photo + alpha_smooth * smooth
    g = sum(float(c) * t for c, t in zip(grad_out, (total, photo, smooth)) if c != 0.0)
    (gf,) = torch.autograd.grad(g, flow64)
    return torch.stack((total, photo, smooth)).detach(), gf


def warp_image64(img: torch.Tensor, flow32: torch.Tensor) -> torch.Tensor:
    return warp64(img.detach().to(torch.float64), flow32.detach().to(torch.float64), flow32).detach()
