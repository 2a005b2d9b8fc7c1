"""Validation without ground truth, as the reference's two self-supervised scripts do it once per epoch
(train_pseudo.py:178-236 + :289-341, train_fundamental.py:388-428 + :503-536): photometric and smoothness terms of the proxy-label
loss, forward-backward cycle consistency ``mean |flow12 + warp(flow21, flow12)|`` and the out-of-bounds ratio of the sample
points ``x + flow12``.  The functions keep the scripts' names and signatures, so a script swaps an import and nothing else.

route="hip": both flow directions come from ``model.flow_pair`` (one feature-pyramid pass per image, engine.PwcBidirPlan) and
the two metrics from ONE fused launch (ops.fb_metrics / csrc/pwc_fb_metrics.hip: nothing image-sized in memory, deterministic);
``validate`` accumulates on the device and synchronises once, after the last batch.  The kernel's sample point is ``x + up`` in
float32 rather than the scripts' linspace + normalise + unnormalise chain -- the same point in exact arithmetic.

route="torch" restates the scripts' chain: three whole forwards per batch, upsample_flow_to + the grid_sample warp of losses.py,
the linspace grid of their oob_ratio.  It is also taken, silently, where the kernel does not apply: tensors off the ROCm device,
float64 (or fp16 / bf16 outside autocast; under autocast they are cast to float32 as ops.ProxyLossFunction casts), two flows of
different sizes, a flow that requires grad with grad mode enabled (the scripts run all of this under no_grad), and geometries
the library declines (H, W, h or w < 2, H < h, W < w, B*2*H*W >= 2^31).
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from . import ops
from .losses import _hip_dtypes_ok, _needs_grad, _warp_torch, upsample_flow_to

__all__ = ["forward_backward_cycle", "_forward_backward_consistency", "oob_ratio", "_oob_ratio", "cycle_and_oob", "validate"]


def _check_route(route: str) -> None:
    if route not in ("hip", "torch"):
        raise ValueError("route must be 'hip' or 'torch', got %r" % (route,))


def _select_finest_flow(outputs):
    """The largest flow of a training-mode tuple, or the tensor itself (train_pseudo.py:166-175, train_fundamental.py:388-394)."""
    if isinstance(outputs, (list, tuple)):
        flows = sorted((f for f in outputs if isinstance(f, torch.Tensor)), key=lambda t: t.shape[-2] * t.shape[-1], reverse=True)
        return flows[0]
    return outputs


def _hip_applies(route: str, flow12: torch.Tensor, flow21: Optional[torch.Tensor], H: int, W: int) -> bool:
    if route != "hip" or _needs_grad(flow12, flow21) or not _hip_dtypes_ok(flow12, flow21):
        return False
    return ops.fb_metrics_supported(flow12, flow21, int(H), int(W))


def cycle_torch(flow12: torch.Tensor, flow21: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """train_pseudo.py:186-193 / train_fundamental.py:403-409 on two given flows."""
    f12 = upsample_flow_to(flow12, H, W)
    f21 = upsample_flow_to(flow21, H, W)
    return (f12 + _warp_torch(f21, f12)).abs().mean()


def oob_torch(flow: torch.Tensor, H: int, W: int, device=None, dtype=None) -> torch.Tensor:
    """train_pseudo.py:210-233 / train_fundamental.py:412-428: the share of normalised sample points outside [-1, 1]."""
    flow = upsample_flow_to(flow, H, W)
    device = flow.device if device is None else device
    dtype = flow.dtype if dtype is None else dtype
    yy, xx = torch.meshgrid(torch.linspace(-1.0, 1.0, H, device=device, dtype=dtype),
                            torch.linspace(-1.0, 1.0, W, device=device, dtype=dtype), indexing="ij")
    x = xx.unsqueeze(0) + (2.0 * flow[:, 0] / max(W - 1, 1)).to(dtype)
    y = yy.unsqueeze(0) + (2.0 * flow[:, 1] / max(H - 1, 1)).to(dtype)
    return ((x < -1) | (x > 1) | (y < -1) | (y > 1)).float().mean()


def cycle_and_oob(flow12: torch.Tensor, flow21: torch.Tensor, H: int, W: int, route: str = "hip") -> Tuple[torch.Tensor, torch.Tensor]:
    """(cycle, oob) as 0-dim tensors for flows [B,2,h,w] and an H x W image grid: one fused launch on the HIP route."""
    _check_route(route)
    if _hip_applies(route, flow12, flow21, H, W):
        out = ops.fb_metrics(flow12.detach().float(), flow21.detach().float(), H, W)
        return out[0], out[1]
    with torch.no_grad():
        return cycle_torch(flow12, flow21, H, W), oob_torch(flow12, H, W)


def oob_ratio(flow: torch.Tensor, H: int, W: int, device=None, dtype=None, route: str = "hip") -> torch.Tensor:
    """Fraction of the B*H*W sample points x + up(flow) that leave the image (train_fundamental.py:412-428; train_pseudo.py's
    _oob_ratio).  `device` / `dtype` are the scripts' arguments for their linspace grid: the HIP route needs neither."""
    _check_route(route)
    if _hip_applies(route, flow, None, H, W) and dtype in (None, torch.float32):
        return ops.fb_metrics(flow.detach().float(), None, H, W)[1]
    with torch.no_grad():
        return oob_torch(flow, H, W, device, dtype)


_oob_ratio = oob_ratio


def _flows(model, img1: torch.Tensor, img2: torch.Tensor, route: str):
    """(flow12, flow21) of the model in eval mode: one shared-pyramid pass where the model offers flow_pair and the HIP route is
    asked for, otherwise the scripts' two forwards."""
    model.eval()
    with torch.no_grad():
        if route == "hip" and hasattr(model, "flow_pair"):
            return model.flow_pair(img1, img2)
        return (_select_finest_flow(model(torch.cat([img1, img2], dim=1))),
                _select_finest_flow(model(torch.cat([img2, img1], dim=1))))


def forward_backward_cycle(model, img1: torch.Tensor, img2: torch.Tensor, route: str = "hip") -> torch.Tensor:
    """train_fundamental.py:397-409: mean |flow12 + warp(flow21, flow12)| at image resolution, a 0-dim tensor."""
    _check_route(route)
    flow12, flow21 = _flows(model, img1, img2, route)
    H, W = img1.shape[-2:]
    return cycle_and_oob(flow12, flow21, H, W, route=route)[0]


def _forward_backward_consistency(model, img1: torch.Tensor, img2: torch.Tensor, warp_fn=None, route: str = "hip") -> torch.Tensor:
    """train_pseudo.py:178-193.  `warp_fn` (the script passes criterion.warp) is accepted for the signature; both routes warp
    with the same border-mode bilinear sampling that function is."""
    return forward_backward_cycle(model, img1, img2, route=route)


def _criterion_terms(criterion, flow, img1, img2):
    if getattr(criterion, "variant", None) == "fundamental":
        return criterion(flow, img1, img2, valid_mask=None)      # train_fundamental.py:517
    return criterion(flow, img1, img2)                          # train_pseudo.py:316


@torch.no_grad()
def validate(model, dataloader, criterion, device, route: str = "hip") -> Dict[str, float]:
    """The scripts' validate (train_pseudo.py:289-341, train_fundamental.py:503-536): the means over batches of the criterion's
    photometric and smoothness terms, the forward-backward cycle and the out-of-bounds ratio, as
    {"val_photo", "val_smooth", "val_fb", "val_oob"}.  route="hip": ONE model.flow_pair per batch (the scripts run three whole
    forwards), criterion(flow12, img1, img2) -- the HIP ProxyLabelLoss -- one metrics launch, sums kept on the device in float64
    and one synchronisation at the end.  route="torch": the scripts' chain."""
    _check_route(route)
    model.eval()
    acc = None
    n = 0
    for img1, img2 in dataloader:
        img1, img2 = img1.to(device), img2.to(device)
        H, W = img1.shape[-2:]
        if route == "hip":
            flow12, flow21 = _flows(model, img1, img2, route)
            _, photo, smooth = _criterion_terms(criterion, flow12, img1, img2)
            fb, oob = cycle_and_oob(flow12, flow21, H, W, route=route)
        else:
            flow12 = _select_finest_flow(model(torch.cat([img1, img2], dim=1)))
            _, photo, smooth = _criterion_terms(criterion, flow12, img1, img2)
            fb = forward_backward_cycle(model, img1, img2, route="torch")
            oob = oob_torch(upsample_flow_to(flow12, H, W), H, W, device=img1.device, dtype=img1.dtype)
        vals = torch.stack([t.detach().double().reshape(()) for t in (photo, smooth, fb, oob)])
        acc = vals if acc is None else acc + vals
        n += 1
    sums = [0.0, 0.0, 0.0, 0.0] if acc is None else acc.cpu().tolist()      # the only host synchronisation
    n = max(n, 1)
    return {"val_photo": sums[0] / n, "val_smooth": sums[1] / n, "val_fb": sums[2] / n, "val_oob": sums[3] / n}
