"""Self-supervised training losses of the reference's two newest training scripts.

ProxyLabelLoss restates train_pseudo.py:65-164 (variant "pseudo") and train_fundamental.py:62-166 (variant "fundamental": +1e-12
in the SSIM denominator and an optional valid_mask).  route="hip" runs the fused gfx950 kernels of ops.ProxyLossFunction (forward
and backward w.r.t. the flow, recomputed from the inputs, deterministic); route="torch" is the reference's composition restated
below.  The torch route is also taken, silently, where the kernels do not apply: an image or the mask requires grad (the kernels
give the flow's gradient only), the tensors are not on a ROCm device, or the library declines the geometry (H, W, h or w < 2,
H < h, W < w, C*H*W >= 2^31).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

_SSIM_EPS = {"pseudo": 0.0, "fundamental": 1e-12}


def upsample_flow_to(flow: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """Resize flow [B,2,h,w] to (H,W), vectors scaled by W/w and H/h (train_fundamental.py:65-77, train_pseudo.py:195-207);
    the flow itself when it already has that size."""
    b, c, h, w = flow.shape
    if (h, w) == (H, W):
        return flow
    up = F.interpolate(flow, size=(H, W), mode="bilinear", align_corners=True)
    return torch.stack((up[:, 0] * (W / w), up[:, 1] * (H / h)), dim=1)


def _warp_torch(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """train_fundamental.py:80-99 / train_pseudo.py:122-157: grid_sample at linspace grid + normalised flow (border, align_corners)."""
    B, C, H, W = img.shape
    flow = upsample_flow_to(flow, H, W)
    yy, xx = torch.meshgrid(torch.linspace(-1.0, 1.0, H, device=img.device, dtype=img.dtype),
                            torch.linspace(-1.0, 1.0, W, device=img.device, dtype=img.dtype), indexing="ij")
    base = torch.stack((xx, yy), dim=-1).unsqueeze(0).expand(B, H, W, 2)
    fn = torch.stack((2.0 * flow[:, 0] / max(W - 1, 1), 2.0 * flow[:, 1] / max(H - 1, 1)), dim=-1)
    return F.grid_sample(img, base + fn, mode="bilinear", padding_mode="border", align_corners=True)


def warp_image(img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """img [B,C,H,W] warped by flow [B,2,h,w] (upsampled and rescaled first).  On a ROCm device, without autograd on the inputs and
    within the kernel's geometry: pwc_flow_warp_image_fwd; otherwise the reference's composition."""
    if (img.is_cuda and flow.is_cuda and not (torch.is_grad_enabled() and (img.requires_grad or flow.requires_grad))
            and img.dtype != torch.float64 and flow.dtype != torch.float64          # the kernel is fp32: no silent precision loss
            and img.dim() == 4 and flow.dim() == 4 and flow.shape[0] == img.shape[0] and flow.shape[1] == 2
            and 2 <= flow.shape[2] <= img.shape[2] and 2 <= flow.shape[3] <= img.shape[3]
            and img.shape[1] * img.shape[2] * img.shape[3] < 2 ** 31):
        return ops.flow_warp_image(img.float(), flow.float()).to(img.dtype)
    return _warp_torch(img, flow)


def _ssim_map(x: torch.Tensor, y: torch.Tensor, eps: float, C1: float = 0.01 ** 2, C2: float = 0.03 ** 2) -> torch.Tensor:
    """Per-channel clamp((1 - SSIM) / 2, 0, 1) (train_pseudo.py:87-101, train_fundamental.py:139-150)."""
    mu_x = F.avg_pool2d(x, 3, 1, 1)
    mu_y = F.avg_pool2d(y, 3, 1, 1)
    sigma_x = F.avg_pool2d(x * x, 3, 1, 1) - mu_x * mu_x
    sigma_y = F.avg_pool2d(y * y, 3, 1, 1) - mu_y * mu_y
    sigma_xy = F.avg_pool2d(x * y, 3, 1, 1) - mu_x * mu_y
    ssim = ((2 * mu_x * mu_y + C1) * (2 * sigma_xy + C2)) / ((mu_x ** 2 + mu_y ** 2 + C1) * (sigma_x + sigma_y + C2) + eps)
    return torch.clamp((1 - ssim) / 2, 0, 1)


def _smoothness(flow: torch.Tensor) -> torch.Tensor:
    """train_pseudo.py:103-107, train_fundamental.py:152-156."""
    dx = torch.abs(flow[:, :, :, :-1] - flow[:, :, :, 1:])
    dy = torch.abs(flow[:, :, :-1, :] - flow[:, :, 1:, :])
    return dx.mean() + dy.mean()


def proxy_loss_torch(flow: torch.Tensor, img1: torch.Tensor, img2: torch.Tensor, valid_mask: Optional[torch.Tensor] = None,
                     alpha_photo: float = 1.0, alpha_smooth: float = 0.1, variant: str = "pseudo"):
    """(total, photo, smooth) as the reference composes them, in the dtype of the inputs (float64 on CPU for the golden fixture)."""
    warped = _warp_torch(img2, flow)
    if variant == "pseudo" and valid_mask is None:
        # train_pseudo.py:78-85: the L1 and SSIM means are taken separately over [B,C,H,W]
        photo = 0.85 * _ssim_map(img1, warped, 0.0).mean() + 0.15 * torch.abs(warped - img1).mean()
    else:
        # train_fundamental.py:128-150: per-pixel map (channel means), then the (masked) mean
        l1 = (img1 - warped).abs().mean(dim=1, keepdim=True)
        pm = 0.85 * _ssim_map(img1, warped, _SSIM_EPS[variant]).mean(dim=1, keepdim=True) + 0.15 * l1
        if valid_mask is None:
            photo = pm.mean()
        else:
            m = valid_mask.unsqueeze(1) if valid_mask.dim() == pm.dim() - 1 else valid_mask   # train_fundamental.py:117-126
            m = (m > 0.5).to(pm.dtype)
            photo = (pm * m).sum() / m.sum().clamp_min(1.0)
    smooth = _smoothness(flow)
    total = alpha_photo * photo + alpha_smooth * smooth
    return total, photo, smooth


class ProxyLabelLoss(nn.Module):
    """Photometric (0.85 SSIM + 0.15 L1 of img1 against img2 warped by the flow) + alpha_smooth * first-order smoothness.
    forward(flow [B,2,h,w], img1, img2 [B,C,H,W], valid_mask=None [B,H,W] / [B,1,H,W], bool or float) -> (total, photo, smooth),
    0-dim tensors.  variant "pseudo" = train_pseudo.py:65-164, "fundamental" = train_fundamental.py:62-166 (a mask is honoured by
    both: the masked mean of train_fundamental.py:117-126)."""

    def __init__(self, alpha_photo: float = 1.0, alpha_smooth: float = 0.1, variant: str = "pseudo", route: str = "hip"):
        super().__init__()
        if variant not in _SSIM_EPS:
            raise ValueError("variant must be 'pseudo' or 'fundamental', got %r" % (variant,))
        if route not in ("hip", "torch"):
            raise ValueError("route must be 'hip' or 'torch', got %r" % (route,))
        self.alpha_photo = alpha_photo
        self.alpha_smooth = alpha_smooth
        self.variant = variant
        self.route = route

    def _hip_applies(self, flow, img1, img2, valid_mask) -> bool:
        if self.route != "hip":
            return False
        if torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad
                                        or (valid_mask is not None and valid_mask.requires_grad)):
            return False
        # the kernels take float32; under autocast ProxyLossFunction casts fp16 / bf16 to float32 (float64 is never cast)
        ok = (torch.float32, torch.float16, torch.bfloat16) if torch.is_autocast_enabled("cuda") else (torch.float32,)
        if flow.dtype not in ok or img1.dtype not in ok or img2.dtype not in ok:
            return False
        m = valid_mask
        if m is not None and not (m.dim() == 3 or (m.dim() == 4 and m.shape[1] == 1)):
            return False
        return ops.proxy_loss_supported(flow, img1, img2, m)

    def forward(self, flow: torch.Tensor, img1: torch.Tensor, img2: torch.Tensor,
                valid_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        if self._hip_applies(flow, img1, img2, valid_mask):
            out = ops.ProxyLossFunction.apply(flow, img1, img2, valid_mask, float(self.alpha_photo), float(self.alpha_smooth),
                                              _SSIM_EPS[self.variant])
            return out[0], out[1], out[2]
        return proxy_loss_torch(flow, img1, img2, valid_mask, self.alpha_photo, self.alpha_smooth, self.variant)

    def warp(self, img: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
        """train_pseudo.py:122-157 (its forward-backward consistency check warps flows with it, C = 2)."""
        if self.route == "torch":
            return _warp_torch(img, flow)
        return warp_image(img, flow)
