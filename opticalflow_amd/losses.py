"""Self-supervised training losses of the reference's two newest training scripts.

ProxyLabelLoss restates train_pseudo.py:65-164 (variant "pseudo") and train_fundamental.py:62-166 (variant "fundamental": +1e-12
in the SSIM denominator and an optional valid_mask).  route="hip" runs the fused gfx950 kernels of ops.ProxyLossFunction (forward
and backward w.r.t. the flow, recomputed from the inputs, deterministic); route="torch" is the reference's composition restated
below.  The torch route is also taken, silently, where the kernels do not apply: an image or the mask requires grad (the kernels
give the flow's gradient only), the tensors are not on a ROCm device, or the library declines the geometry (H, W, h or w < 2,
H < h, W < w, C*H*W >= 2^31).

The supervised losses of the two fine-tuning scripts keep the reference's names: MaskedCharbonnier (train.py:31-48 on
upsample_flow_to(flow2), train2.py:114-122), supervised_multiscale_loss (train2.py:124-167) and compute_epe (train2.py:100-111).
route="hip" runs ops.FlowLossFunction / ops.MultiscaleLossFunction (fused gfx950 forward and backward w.r.t. the flows); a flow
smaller than the GT is upsampled inside the kernel (align_corners=False, as upsample_flow_to of data_processing_or.py:300-310).
route="torch" is the reference's chain restated below.  The torch route is also taken, silently, for tensors off the ROCm
device, float64 (or fp16 / bf16 outside autocast), a GT / mask / image that requires grad, and geometries the library declines
(h or w < 2, h > H, w > W, more than 8 levels, index overflow).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops

_SSIM_EPS = {"pseudo": 0.0, "fundamental": 1e-12}


def upsample_flow_to(flow: torch.Tensor, H: int, W: int, align_corners: bool = True) -> torch.Tensor:
    """Resize flow [B,2,h,w] to (H,W), vectors scaled by W/w and H/h; the flow itself when it already has that size.
    align_corners=True: train_fundamental.py:65-77, train_pseudo.py:195-207; False: data_processing_or.py:300-310 and
    train2.py:202-213 (the supervised scripts)."""
    b, c, h, w = flow.shape
    if (h, w) == (H, W):
        return flow
    up = F.interpolate(flow, size=(H, W), mode="bilinear", align_corners=align_corners)
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


# ---------------------------------------------------------------- supervised losses (train.py / train2.py)
MULTISCALE_WEIGHTS = (0.32, 0.08, 0.02, 0.01, 0.005)     # train2.py:133


def _plane_mask(mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """[B,1,H,W] and [B,H,W] masks are the same plane (train.py passes the first, train2.py the second)."""
    return mask[:, 0] if mask is not None and mask.dim() == 4 else mask


def _hip_dtypes_ok(*ts) -> bool:
    # the kernels take float32; under autocast the autograd Functions cast fp16 / bf16 to float32 (float64 is never cast)
    ok = (torch.float32, torch.float16, torch.bfloat16) if torch.is_autocast_enabled("cuda") else (torch.float32,)
    return all(t.dtype in ok for t in ts if t is not None)


def _needs_grad(*ts) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def masked_charbonnier_torch(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor], eps: float = 1e-3) -> torch.Tensor:
    """train.py:31-48 / train2.py:114-122 at full resolution (pred upsampled first when it is smaller than gt)."""
    H, W = gt.shape[-2:]
    if tuple(pred.shape[-2:]) != (H, W):
        pred = upsample_flow_to(pred, H, W, align_corners=False)
    epe = torch.sqrt(((pred - gt) ** 2).sum(dim=1, keepdim=True) + eps ** 2)
    if mask is None:
        return epe.mean()
    valid = (_plane_mask(mask) > 0.5).to(epe.dtype).unsqueeze(1)
    return (epe * valid).sum() / valid.sum().clamp(min=1.0)


def compute_epe_torch(flow_pred: torch.Tensor, flow_gt: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """train2.py:100-111 (flow_pred upsampled first, as validate does at :202-213, when it is smaller than flow_gt)."""
    H, W = flow_gt.shape[-2:]
    if tuple(flow_pred.shape[-2:]) != (H, W):
        flow_pred = upsample_flow_to(flow_pred, H, W, align_corners=False)
    epe = torch.sqrt(torch.sum((flow_pred - flow_gt) ** 2, dim=1))
    if mask is None:
        return epe.mean()
    m = _plane_mask(mask).to(epe.dtype)
    return (epe * m).sum() / (m.sum() + 1e-8)


def _warp_zeros_torch(im2: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """warp_image of train2.py:44-62: grid_sample(bilinear, zeros, align_corners=True) at pixel + flow."""
    B, C, H, W = im2.shape
    xx = torch.arange(0, W, device=im2.device).view(1, -1).repeat(H, 1)
    yy = torch.arange(0, H, device=im2.device).view(-1, 1).repeat(1, W)
    grid = torch.stack((xx, yy), 0).unsqueeze(0).to(flow.dtype)
    vgrid = grid + flow
    gx = 2.0 * vgrid[:, 0] / max(W - 1, 1) - 1.0
    gy = 2.0 * vgrid[:, 1] / max(H - 1, 1) - 1.0
    return F.grid_sample(im2, torch.stack((gx, gy), dim=-1), align_corners=True)


def supervised_multiscale_loss_torch(flow_preds, images, flows_gt, masks, w=None, lambda_photo=0.0, lambda_smooth=0.0):
    """train2.py:124-167 (with :44-97), restated."""
    if not isinstance(flow_preds, (list, tuple)):
        flow_preds = [flow_preds]
    if w is None:
        w = list(MULTISCALE_WEIGHTS)
    B, _, H, W = flows_gt.shape
    masks = _plane_mask(masks)
    if masks is None:
        masks = torch.ones((B, H, W), dtype=flows_gt.dtype, device=flows_gt.device)
    im1, im2 = (images[:, :3], images[:, 3:]) if images is not None else (None, None)
    total = 0.0
    for i, pred in enumerate(flow_preds):
        h, w_ = pred.shape[-2:]
        gt_s = F.interpolate(flows_gt, size=(h, w_), mode="bilinear", align_corners=False)
        mask_s = F.interpolate(masks.unsqueeze(1).float(), size=(h, w_), mode="nearest").squeeze(1)   # float32, as the script
        gt_s = torch.stack((gt_s[:, 0] / (W / float(w_)), gt_s[:, 1] / (H / float(h))), dim=1)
        lvl = masked_charbonnier_torch(pred, gt_s, mask_s)
        if lambda_photo > 0.0 or lambda_smooth > 0.0:
            im1_s = F.interpolate(im1, size=(h, w_), mode="bilinear", align_corners=False)
            im2_s = F.interpolate(im2, size=(h, w_), mode="bilinear", align_corners=False)
            if lambda_photo > 0.0:
                l1 = torch.abs(im1_s - _warp_zeros_torch(im2_s, pred)) * mask_s.unsqueeze(1)
                lvl = lvl + lambda_photo * (l1.sum() / (mask_s.sum() + 1e-8))
            if lambda_smooth > 0.0:
                dx = torch.abs(pred[:, :, :, :-1] - pred[:, :, :, 1:])
                dy = torch.abs(pred[:, :, :-1, :] - pred[:, :, 1:, :])
                img_dx = torch.mean(torch.abs(im1_s[:, :3, :, :-1] - im1_s[:, :3, :, 1:]), dim=1, keepdim=True)
                img_dy = torch.mean(torch.abs(im1_s[:, :3, :-1, :] - im1_s[:, :3, 1:, :]), dim=1, keepdim=True)
                lvl = lvl + lambda_smooth * ((dx * torch.exp(-img_dx)).mean() + (dy * torch.exp(-img_dy)).mean())
        total = total + (w[i] if i < len(w) else w[-1]) * lvl
    return total


class MaskedCharbonnier(nn.Module):
    """Masked Charbonnier EPE of train.py:31-48 / train2.py:114-122: sum(sqrt(|pred - gt|^2 + eps^2) [mask > 0.5]) /
    max(sum [mask > 0.5], 1).  forward(pred [B,2,h,w], gt [B,2,H,W], mask [B,1,H,W] or [B,H,W], float / bool / uint8): pred at
    gt's size, or smaller -- then it is train.py's loss_fn(upsample_flow_to(flow2, H, W), gt, valid) (align_corners=False) in one
    fused call, with no upsampled flow in memory."""

    def __init__(self, eps: float = 1e-3, route: str = "hip"):
        super().__init__()
        if route not in ("hip", "torch"):
            raise ValueError("route must be 'hip' or 'torch', got %r" % (route,))
        self.eps = eps
        self.route = route

    def forward(self, pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        if (self.route == "hip" and not _needs_grad(gt, mask) and _hip_dtypes_ok(pred, gt)
                and ops.sup_flow_loss_supported(pred, gt, mask)):
            return ops.FlowLossFunction.apply(pred, gt, _plane_mask(mask), float(self.eps), "threshold")[0]
        return masked_charbonnier_torch(pred, gt, mask, self.eps)


def compute_epe(flow_pred: torch.Tensor, flow_gt: torch.Tensor, mask: Optional[torch.Tensor] = None,
                route: str = "hip") -> torch.Tensor:
    """End-point error of train2.py:100-111: sum(|pred - gt| mask) / (sum mask + 1e-8) with the raw mask, the mean without one.
    flow_pred smaller than flow_gt is upsampled first (align_corners=False, as validate does), fused on the HIP route.  The HIP
    route is a forward only: a flow that requires grad takes the torch route."""
    if route not in ("hip", "torch"):
        raise ValueError("route must be 'hip' or 'torch', got %r" % (route,))
    if (route == "hip" and not _needs_grad(flow_pred, flow_gt, mask) and _hip_dtypes_ok(flow_pred, flow_gt)
            and ops.sup_flow_loss_supported(flow_pred, flow_gt, mask)):
        return ops.sup_flow_loss(flow_pred.float(), flow_gt.float(), _plane_mask(mask), 0.0, "raw")[0]
    return compute_epe_torch(flow_pred, flow_gt, mask)


def supervised_multiscale_loss(flow_preds, images, flows_gt, masks, w=None, lambda_photo: float = 0.0,
                               lambda_smooth: float = 0.0, route: str = "hip") -> torch.Tensor:
    """train2.py:124-167: sum_i w[i] (MaskedCharbonnier(pred_i, downsampled GT, nearest mask) + lambda_photo * photometric +
    lambda_smooth * edge-aware smoothness), every prediction supervised at its own size.  flow_preds: one tensor or the list /
    tuple of PWCDCNet(trainable=True); images [B,6,H,W] (read only when a lambda is > 0); flows_gt [B,2,H,W]; masks [B,H,W] or
    [B,1,H,W].  w defaults to (0.32, 0.08, 0.02, 0.01, 0.005), w[-1] past its end."""
    if route not in ("hip", "torch"):
        raise ValueError("route must be 'hip' or 'torch', got %r" % (route,))
    preds = list(flow_preds) if isinstance(flow_preds, (list, tuple)) else [flow_preds]
    wl = list(MULTISCALE_WEIGHTS) if w is None else list(w)
    weights = tuple(float(wl[i] if i < len(wl) else wl[-1]) for i in range(len(preds)))
    with_images = lambda_photo > 0.0 or lambda_smooth > 0.0
    img = images if with_images else None
    if (route == "hip" and not _needs_grad(flows_gt, masks, img) and _hip_dtypes_ok(flows_gt, img, *preds)
            and ops.sup_multiscale_loss_supported(preds, flows_gt, masks, img)):
        return ops.MultiscaleLossFunction.apply(flows_gt, _plane_mask(masks), img, weights, float(lambda_photo),
                                                float(lambda_smooth), *preds)[0]
    return supervised_multiscale_loss_torch(preds, images, flows_gt, masks, wl, lambda_photo, lambda_smooth)
