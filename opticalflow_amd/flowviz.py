"""Flow pictures on the device: what the reference's user-facing scripts make of a flow field, as HIP kernels (csrc/pwc_flowviz.hip).

  * ``flow_to_color``       the colour-wheel image of pwc_extract_flow.py:58-123, uint8 [B,h,w,3] RGB
  * ``dominant_direction``  calculate_dominant_direction of topview.py:122-134
  * ``quiver_arrows``       the arrow grid of create_quiver_frame (pwc_extract_flow_video.py:94-135, style "video") and of
                            draw_flow_arrows (topview.py:137-178, style "topview"): vectors, tips and flags per grid point.  Drawing the
                            arrows is left to the caller.

Every function takes the network's flow [B,2,Hq,Wq] (float32, on the device) and an optional ``crop`` = (h, w), the top-left part the
reference colours and draws (video.py documents why the scripts crop the quarter-resolution map).  Results stay on the device; nothing
synchronises.  ``Renderer`` holds the buffers of one fixed geometry so that the same kernels can be captured in a HIP graph
(video.FlowStream(render=...)).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from . import ops

__all__ = ["Arrows", "RenderSpec", "Rendered", "Renderer", "dominant_direction", "flow_to_color", "quiver_arrows", "quiver_params"]


class Arrows(NamedTuple):
    vec: torch.Tensor     # float32 [B,Gy,Gx,2]  (dx, dy) in frame pixels
    tip: torch.Tensor     # int32   [B,Gy,Gx,2]  (x, y) of the arrow head
    flags: torch.Tensor   # uint8   [B,Gy,Gx]    bit 0 keep, bit 1 aligned with the dominant direction


def flow_to_color(flow: torch.Tensor, clip_flow: Optional[float] = None, crop: Optional[Tuple[int, int]] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [B,h,w,3] RGB.  Each sample is normalised by its own maximum radius: the reference colours one image at a time."""
    stats = ops.flow_stats(flow, crop=crop, clip_flow=clip_flow)
    return ops.flow_color(flow, stats, crop=crop, clip_flow=clip_flow, out=out)


def dominant_direction(flow: torch.Tensor, threshold: float = 1.0, crop: Optional[Tuple[int, int]] = None):
    """(mean [B,2] float32, count [B] int64) over the pixels whose magnitude is > threshold; the mean is 0 where there are none."""
    stats = ops.flow_stats(flow, crop=crop, threshold=threshold)
    return stats[:, 2:4], stats.view(torch.int32)[:, 1].to(torch.int64)


def quiver_params(style: str, scale: float) -> Tuple[float, int]:
    """(gain, tip_rule) of a drawing style: "video" = int(round(x + dx / max(scale, 1e-6))), "topview" = int(x + dx * scale)."""
    if style == "video":
        return 1.0 / max(float(scale), 1e-6), 0
    if style == "topview":
        return float(scale), 1
    raise ValueError("style must be 'video' or 'topview', got %r" % (style,))


def quiver_arrows(flow: torch.Tensor, frame_hw: Tuple[int, int], step: int = 16, scale: float = 1.0, min_mag: float = 0.5,
                  crop: Optional[Tuple[int, int]] = None, style: str = "video", dominant: Optional[torch.Tensor] = None,
                  angle_threshold: float = 30.0, vec_scale: Optional[Tuple[float, float]] = None, out=None) -> Arrows:
    """The arrow grid every `step` pixels of an (H, W) frame.  vec_scale defaults to (W / w, H / h), create_quiver_frame's correction
    for the resize; topview.py rescales after resizing, which is (1, 1) here.  dominant: float32 [B,2] on the device (for instance
    dominant_direction's mean) colours the arrows by their agreement with it (flags bit 1)."""
    gain, tip_rule = quiver_params(style, scale)
    H, W = int(frame_hw[0]), int(frame_hw[1])
    h, w = (flow.shape[-2], flow.shape[-1]) if crop is None else crop
    if vec_scale is None:
        vec_scale = (float(W) / float(w), float(H) / float(h))
    return Arrows(*ops.flow_quiver(flow, H, W, step, vec_scale, gain, tip_rule, min_mag, crop=crop, dominant=dominant,
                                   angle_threshold=angle_threshold, out=out))


class RenderSpec(NamedTuple):
    """What video.FlowStream renders after every push.  quiver: None, or the keyword arguments of quiver_arrows without `crop`, `out`
    and `dominant` (frame_hw is required); dominant=True colours the arrows by the sample's own dominant direction."""
    color: bool = True
    clip_flow: Optional[float] = None
    quiver: Optional[dict] = None
    dominant: bool = False
    threshold: float = 1.0
    crop: Optional[Tuple[int, int]] = None


class Rendered(NamedTuple):
    color: Optional[torch.Tensor]
    arrows: Optional[Arrows]
    stats: torch.Tensor


class Renderer:
    """The kernels of one RenderSpec on static buffers for flows of one shape: `run(flow)` launches them on the current stream and
    allocates nothing, so it can sit inside a graph capture.  The outputs are reused by every run."""

    def __init__(self, spec: RenderSpec, flow_shape, device):
        n, _, Hq, Wq = flow_shape
        self.spec = spec
        self.crop = (Hq, Wq) if spec.crop is None else (int(spec.crop[0]), int(spec.crop[1]))
        h, w = self.crop
        self.stats = torch.zeros((n, 4), dtype=torch.float32, device=device)
        self.workspace = torch.empty(ops.flow_stats_workspace_bytes(n, h, w) // 8, dtype=torch.int64, device=device)
        self.color = torch.empty((n, h, w, 3), dtype=torch.uint8, device=device) if spec.color else None
        self.arrows = None
        if spec.quiver is not None:
            kw = dict(spec.quiver)
            bad = set(kw) - {"frame_hw", "step", "scale", "min_mag", "style", "angle_threshold", "vec_scale"}
            if bad or "frame_hw" not in kw:
                raise ValueError("RenderSpec.quiver takes frame_hw (required), step, scale, min_mag, style, angle_threshold, vec_scale; "
                                 "got %s" % sorted(kw))
            self.quiver_kw = kw
            H, W = kw["frame_hw"]
            step = int(kw.get("step", 16))
            if step < 1:
                raise ValueError("step must be >= 1, got %d" % step)
            gy, gx = (int(H) + step - 1) // step, (int(W) + step - 1) // step
            self.arrows = Arrows(torch.empty((n, gy, gx, 2), dtype=torch.float32, device=device),
                                 torch.empty((n, gy, gx, 2), dtype=torch.int32, device=device),
                                 torch.empty((n, gy, gx), dtype=torch.uint8, device=device))

    def run(self, flow: torch.Tensor) -> Rendered:
        sp = self.spec
        ops.flow_stats(flow, crop=self.crop, clip_flow=sp.clip_flow, threshold=sp.threshold, out=self.stats, workspace=self.workspace)
        if self.color is not None:
            ops.flow_color(flow, self.stats, crop=self.crop, clip_flow=sp.clip_flow, out=self.color)
        if self.arrows is not None:
            quiver_arrows(flow, crop=self.crop, dominant=self.stats[:, 2:4] if sp.dominant else None, out=tuple(self.arrows),
                          **self.quiver_kw)
        return Rendered(self.color, self.arrows, self.stats)
