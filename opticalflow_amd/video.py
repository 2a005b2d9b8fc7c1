"""Consecutive-frame optical flow for video, the loop of ``pwc_extract_flow_video.py:219-305``.

The reference reads frame t+1, runs the whole network on (frame t, frame t+1) and then does
``frame1 = frame2`` (pwc_extract_flow_video.py:300), so every frame passes through the feature
pyramid twice.  ``FlowStream`` keeps frame t's pyramid resident in HBM (engine.PwcVideoPlan) and
runs the pyramid once per frame; results are the same numbers as ``model(cat(frame_t, frame_t+1))``.

Pre/post-processing helpers follow the reference script:
  * ``frame_to_tensor``   BGR uint8 HWC -> RGB float32 CHW / 255        (pwc_extract_flow_video.py:27-34)
  * ``pad_to_multiple_of_64`` replicate-pad bottom/right                 (:36-42, same as kitti.pad_to_64)
  * ``unpad``             the reference crops the QUARTER-resolution flow by the FULL-resolution pad
                          (:44-47, :213) -- reproduced as is (kitti.model_infer documents the same quirk)

The first two run on the host and upload float32, four times the bytes of the frame.  ``ingest_frames`` is the same arithmetic as one
HIP kernel on raw uint8 frames (csrc/pwc_video.hip, bit for bit the host helpers' result), and ``RawFlowStream`` is a FlowStream whose
push starts from raw frames: upload of the bytes, ingest, network, pictures and vanishing point as one graph replay.
``flow_video(..., ingest="hip")`` and ``flow_video_rendered(..., ingest="hip")`` select it; ``flow_video_vanishing`` is the per-frame
loop of pwc_extract_flow_video_vanishpoint.py up to the drawing.
"""
from __future__ import annotations

from typing import Iterable, Iterator, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._pipeline import PinnedRing, capture_graph, pad64
from .engine import PwcVideoPlan
from .flowviz import Renderer, RenderSpec
from .kitti import pad_to_64, unpad as _unpad

__all__ = ["FlowStream", "RawFlowStream", "RawGeometry", "RenderSpec", "frame_to_tensor", "flow_video", "flow_video_rendered",
           "flow_video_vanishing", "ingest_frames", "raw_geometry"]


def frame_to_tensor(frame: np.ndarray) -> torch.Tensor:
    """numpy (H,W,3) BGR uint8 -> tensor (3,H,W) RGB float32 in [0,1] (pwc_extract_flow_video.py:27-34)."""
    if frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError("expected an (H,W,3) BGR frame, got %s" % (frame.shape,))
    rgb = frame[:, :, ::-1].astype(np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(np.transpose(rgb, (2, 0, 1))))


def ingest_frames(frames_u8: torch.Tensor, bgr: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raw frames uint8 [n,H,W,3] (or one [H,W,3]) on the device -> float32 [n,3,Hp,Wp]: ``frame_to_tensor`` (with bgr; bgr=False keeps
    the channel order) + ``pad_to_64`` as one HIP kernel, the same bits.  frames_u8 may be a view with a batch stride, out likewise."""
    if torch.is_tensor(frames_u8) and frames_u8.dim() == 3:
        frames_u8 = frames_u8.unsqueeze(0)
    return ops.video_ingest(frames_u8, out=out, bgr=bgr)


class RawGeometry(NamedTuple):
    height: int                 # Hp: the frame's height rounded up to a multiple of 64 (what the network sees)
    width: int                  # Wp
    pads: Tuple[int, int]       # (pad_h, pad_w) of pad_to_multiple_of_64
    crop: Tuple[int, int]       # (Hp/4 - pad_h, Wp/4 - pad_w): the part of the quarter-resolution flow the reference keeps


def raw_geometry(frame_h: int, frame_w: int) -> RawGeometry:
    """Padded size, pads and the reference's crop for frames of this size (pwc_extract_flow_video.py:36-47, 213: the FULL-resolution
    pad comes off the QUARTER-resolution flow).  A frame so small against its pad that nothing would be left is refused."""
    H, W = int(frame_h), int(frame_w)
    Hp, Wp, pad_h, pad_w = pad64(H, W)
    crop = (Hp // 4 - pad_h, Wp // 4 - pad_w)
    if crop[0] < 1 or crop[1] < 1:
        raise ValueError("a %dx%d frame pads by (%d, %d) to %dx%d: cropping the quarter-resolution flow by the full-resolution pad, as "
                         "the reference does, leaves nothing" % (H, W, pad_h, pad_w, Hp, Wp))
    return RawGeometry(Hp, Wp, (pad_h, pad_w), crop)


class FlowStream:
    """flow(frame[t] -> frame[t+1]) for a running sequence of equally sized frames.

    ``net`` is an ``opticalflow_amd.PWCDCNet`` on the ROCm device.  ``batch`` frames are consumed per
    ``push``; ``batch=1`` is the reference's loop.  With ``use_graph`` each push is one HIP-graph replay.

    ``render`` (a ``flowviz.RenderSpec``): every push also makes the colour image and / or the arrow grid of its flows, on the device
    and, with ``use_graph``, inside the same replay; ``rendered`` then holds them (static buffers, like the flow: consume or clone
    them before the next push).  Without ``render`` nothing changes.
    """

    def __init__(self, net, batch: int, height: int, width: int, use_graph: bool = True, render: Optional[RenderSpec] = None):
        params = {k: v.detach() for k, v in net.state_dict(keep_vars=True).items()}
        p0 = next(iter(params.values()))
        if not p0.is_cuda:
            from ._lib import PwcHipError
            raise PwcHipError("FlowStream needs the model on the ROCm device (parameters are on %s)" % p0.device)
        self.device = p0.device
        self.batch, self.height, self.width = batch, height, width
        if getattr(net, "precision", "fp32") == "fp16-strict":
            from .engine_strict import PwcVideoPlanStrict
            self.plan = PwcVideoPlanStrict(params, batch, height, width, self.device, net.md, net.normalize_corr,
                                           net.align_corners, getattr(net, "variant", "dc"))
        elif getattr(net, "precision", "fp32") == "fp16":
            from .engine_f16 import PwcVideoPlanF16
            self.plan = PwcVideoPlanF16(params, batch, height, width, self.device, net.md, net.normalize_corr,
                                        net.align_corners, getattr(net, "variant", "dc"))
        else:
            self.plan = PwcVideoPlan(params, batch, height, width, self.device, torch.float32, net.md,
                                     net.normalize_corr, net.align_corners, net.conv_backend,
                                     getattr(net, "variant", "dc"))
        self.use_graph = use_graph
        self._graph = None
        self._static = torch.empty((batch, 3, height, width), device=self.device, dtype=torch.float32)
        self.renderer = Renderer(render, tuple(self.plan.flow_out.shape), self.device) if render is not None else None
        self.rendered = None

    def _push(self, frames: torch.Tensor) -> torch.Tensor:
        flow = self.plan.push(frames)
        if self.renderer is not None:
            self.rendered = self.renderer.run(flow)
        return flow

    def prime(self, frame: torch.Tensor) -> None:
        """First frame of the sequence, [1,3,H,W] or [3,H,W]."""
        if frame.dim() == 3:
            frame = frame.unsqueeze(0)
        with torch.no_grad():
            self.plan.prime(frame.to(self.device, torch.float32))

    def push(self, frames: torch.Tensor) -> torch.Tensor:
        """``batch`` further frames [B,3,H,W]; returns [B,2,H/4,W/4], row i = flow from the frame before
        frames[i] to frames[i] (a view of the plan's output buffer: clone it to keep it across pushes)."""
        if frames.dim() == 3:
            frames = frames.unsqueeze(0)
        with torch.no_grad():
            if not self.use_graph:
                return self._push(frames.to(self.device, torch.float32))
            if not self.plan.primed:
                raise RuntimeError("FlowStream.push before prime(first_frame)")
            if tuple(frames.shape) != tuple(self._static.shape):
                raise ValueError("expected frames %s, got %s" % (tuple(self._static.shape), tuple(frames.shape)))
            self._static.copy_(frames)
            return self._replay(self._static)

    def _replay(self, src: torch.Tensor) -> torch.Tensor:
        """One push from the static input buffer `src` as a graph replay (captured on the first call)."""
        if self._graph is None:
            # warm-up outside capture would advance the carry slot: save and restore it around the capture (the strict plan's pyr_a
            # is its fp32 upper plan's)
            keep = {l: self.plan.pyr_a[l][0].clone() for l in range(2, 7)}

            def restore():
                for l, t in keep.items():
                    self.plan.pyr_a[l][0].copy_(t)
            self._graph, _ = capture_graph(lambda: self._push(src), self.device, between=restore)
        self._graph.replay()
        return self.plan.flow_out


def _frame_render(render: Optional[RenderSpec], crop: Tuple[int, int], frame_hw: Tuple[int, int]) -> Optional[RenderSpec]:
    """`render` for frames of one size: the crop filled in, the quiver's frame_hw defaulting to the frame."""
    q = None if render is None or render.quiver is None else dict({"frame_hw": frame_hw}, **render.quiver)
    return None if render is None else render._replace(crop=crop, quiver=q)


class RawFlowStream(FlowStream):
    """A FlowStream whose push starts from raw frames: uint8 [batch,frame_h,frame_w,3] as cv2 decodes them (bgr=True; False for RGB).

    The stream owns a static uint8 device buffer for the frames and two pinned host staging slots; each slot's reuse is guarded by an
    event, so a push waits for the upload two pushes back at the most, never for the previous replay's.  It pads to multiples of 64
    itself (`height`, `width`, `pads`) and knows the reference's crop (`crop`, see raw_geometry).  One push is one replay: ingest kernel
    -> pyramid and decoder -> renderer (`render`, a RenderSpec whose crop is filled in here and whose quiver's frame_hw defaults to the
    frame) -> VanishingEstimator.run on the arrows' vec when `vanishing` is given: a dict of the estimator's keyword arguments
    (min_mag, max_points, grid_size, min_pairs, seed; step, if given, must be the quiver's), which needs a quiver in `render`.
    Results are static buffers reused by every push: the returned flow (uncropped, [batch,2,Hp/4,Wp/4]), `rendered`, `points`.
    Nothing inside the replay allocates or synchronises.
    """

    def __init__(self, net, batch: int, frame_h: int, frame_w: int, bgr: bool = True, render: Optional[RenderSpec] = None,
                 vanishing: Optional[dict] = None, use_graph: bool = True):
        geo = raw_geometry(frame_h, frame_w)
        self.frame_h, self.frame_w, self.bgr = int(frame_h), int(frame_w), bool(bgr)
        self.pads, self.crop = geo.pads, geo.crop
        render = _frame_render(render, geo.crop, (self.frame_h, self.frame_w))
        if vanishing is not None and (render is None or render.quiver is None):
            raise ValueError("vanishing needs the arrow grid: give a RenderSpec with a quiver")
        super().__init__(net, batch, geo.height, geo.width, use_graph=use_graph, render=render)
        self._raw = torch.empty((batch, self.frame_h, self.frame_w, 3), dtype=torch.uint8, device=self.device)
        self._ring = PinnedRing(2)
        for _ in range(2):                      # both staging slots are pinned here, not in the first two pushes
            self._ring.acquire((self._raw.shape, torch.uint8))
        self.estimator = None
        self.points = None
        if vanishing is not None:
            from .vanishing import VanishingEstimator
            kw, q = dict(vanishing), render.quiver
            if int(kw.setdefault("step", q.get("step", 16))) != int(q.get("step", 16)):
                raise ValueError("vanishing step %s differs from the quiver's %s" % (kw["step"], q.get("step", 16)))
            if "frame_hw" in kw or "device" in kw or "batch" in kw:
                raise ValueError("vanishing takes step, min_mag, max_points, grid_size, min_pairs, seed; the rest is the stream's")
            self.estimator = VanishingEstimator(batch, tuple(q["frame_hw"]), device=self.device, **kw)

    def _push(self, raw: torch.Tensor) -> torch.Tensor:
        ops.video_ingest(raw, out=self._static, bgr=self.bgr)
        flow = super()._push(self._static)
        if self.estimator is not None:
            self.points = self.estimator.run(self.rendered.arrows.vec)
        return flow

    def _as_frames(self, frames, n: int) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(frames)) if isinstance(frames, np.ndarray) else frames
        if not torch.is_tensor(t):
            raise TypeError("frames must be a NumPy array or a tensor, got %s" % type(frames).__name__)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dtype != torch.uint8 or tuple(t.shape) != (n, self.frame_h, self.frame_w, 3):
            raise ValueError("expected uint8 frames %s, got %s %s" % ((n, self.frame_h, self.frame_w, 3), t.dtype, tuple(t.shape)))
        return t

    def _upload(self, t: torch.Tensor) -> None:
        """frames -> the static device buffer, on the current stream (so behind the previous replay, which reads that buffer)"""
        if t.is_cuda:
            self._raw.copy_(t)
            return
        stage, = self._ring.acquire((self._raw.shape, torch.uint8))     # waits until the upload two pushes back has read this slot
        stage.copy_(t)
        self._raw.copy_(stage, non_blocking=True)
        self._ring.mark(torch.cuda.current_stream(self.device))

    def prime(self, frame) -> None:
        """First frame of the sequence: uint8 [frame_h,frame_w,3] or [1,frame_h,frame_w,3], NumPy, CPU tensor or device tensor."""
        t = self._as_frames(frame, 1).to(self.device)
        with torch.no_grad():
            self.plan.prime(ops.video_ingest(t, bgr=self.bgr))

    def push(self, frames) -> torch.Tensor:
        """``batch`` further raw frames; returns [batch,2,Hp/4,Wp/4] like FlowStream.push (a view of the plan's output buffer; the
        reference's result is its top-left `crop`)."""
        t = self._as_frames(frames, self.batch)
        if not self.plan.primed:
            raise RuntimeError("RawFlowStream.push before prime(first_frame)")
        with torch.no_grad(), torch.cuda.device(self.device):
            self._upload(t)
            return self._replay(self._raw) if self.use_graph else self._push(self._raw)


class _HostStream:
    """ingest="host" behind the part of RawFlowStream the frame loops use (batch 1): ``frame_to_tensor`` + ``pad_to_64`` on the host, the
    float32 frame uploaded, a plain FlowStream.  What this path costs is the baseline tools/bench_video_ingest.py reports against."""

    def __init__(self, net, batch: int, frame_h: int, frame_w: int, render: Optional[RenderSpec] = None, use_graph: bool = True):
        Hp, Wp, pad_h, pad_w = pad64(frame_h, frame_w)
        self.frame_h, self.frame_w, self.pads = frame_h, frame_w, (pad_h, pad_w)
        self.crop = (Hp // 4 - pad_h, Wp // 4 - pad_w)     # the reference's unpad: the full-resolution pad off the quarter-resolution map
        self._stream = FlowStream(net, batch, Hp, Wp, use_graph=use_graph, render=_frame_render(render, self.crop, (frame_h, frame_w)))
        self.renderer = self._stream.renderer

    rendered = property(lambda self: self._stream.rendered)

    def _upload(self, frame: np.ndarray) -> torch.Tensor:
        return pad_to_64(frame_to_tensor(frame).unsqueeze(0))[0].to(self._stream.device)

    def prime(self, frame: np.ndarray) -> None:
        self._stream.prime(self._upload(frame))

    def push(self, frame: np.ndarray) -> torch.Tensor:
        return self._stream.push(self._upload(frame))


def _pushes(frames: Iterable[np.ndarray], ingest: str, net, **kw):
    """The per-frame loop of the flow_video family: the stream (RawFlowStream for ingest="hip", _HostStream for "host", batch 1, **kw)
    is built for the first frame's size and primed with it; every further frame is pushed, yielding (stream, flow)."""
    if ingest not in ("host", "hip"):
        raise ValueError("ingest must be 'host' or 'hip', got %r" % (ingest,))
    stream = None
    for frame in frames:
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("expected an (H,W,3) BGR frame, got %s" % (frame.shape,))
        if stream is None:
            stream = (RawFlowStream if ingest == "hip" else _HostStream)(net, 1, frame.shape[0], frame.shape[1], **kw)
            stream.prime(frame)
        elif tuple(frame.shape[:2]) != (stream.frame_h, stream.frame_w):
            raise ValueError("frame size changed mid-stream")
        else:
            yield stream, stream.push(frame)


def flow_video(net, frames: Iterable[np.ndarray], use_graph: bool = True, ingest: str = "host") -> Iterator[np.ndarray]:
    """Generator over BGR uint8 frames yielding one (h,w,2) float32 flow per consecutive pair, exactly
    what ``process_frame_pair`` returns for (frame_t, frame_t+1) (pwc_extract_flow_video.py:192-216).
    ingest="hip": the raw frame is uploaded and prepared on the device (RawFlowStream); the same numbers."""
    for stream, flow in _pushes(frames, ingest, net, use_graph=use_graph):
        flow = _unpad(flow, stream.pads[0], stream.pads[1])     # full-resolution pad, like the reference
        yield flow.squeeze(0).permute(1, 2, 0).contiguous().cpu().numpy()


def _rendered_dict(stream: FlowStream, flow: torch.Tensor, with_flow: bool) -> dict:
    r, out = stream.rendered, {}
    if r.color is not None:
        out["color"] = r.color[0].cpu().numpy()
    if r.arrows is not None:
        out["vec"], out["tip"], out["flags"] = (a[0].cpu().numpy() for a in r.arrows)
    if with_flow:
        ch, cw = stream.renderer.crop
        out["flow"] = flow[0, :, :ch, :cw].permute(1, 2, 0).contiguous().cpu().numpy()
    return out


def flow_video_rendered(net, frames: Iterable[np.ndarray], color: bool = True, quiver: Optional[dict] = None, use_graph: bool = True,
                        clip_flow: Optional[float] = None, dominant: bool = False, with_flow: bool = False,
                        ingest: str = "host") -> Iterator[dict]:
    """flow_video that hands back pictures instead of the float flow: per consecutive pair a dict with "color" (h,w,3) uint8 RGB (the
    colour wheel of pwc_extract_flow.py's flow_to_color) when `color`, and "vec" (Gy,Gx,2) float32, "tip" (Gy,Gx,2) int32, "flags"
    (Gy,Gx) uint8 when `quiver` is given: the keyword arguments of flowviz.quiver_arrows (step, scale, min_mag, style, ...;
    frame_hw defaults to the frame's size).  Both are made on the device from the same cropped quarter-resolution flow flow_video
    yields, and only they are downloaded; with_flow=True adds "flow", exactly flow_video's array.  ingest="hip": raw frames are
    uploaded and prepared on the device (RawFlowStream); the same results."""
    spec = RenderSpec(color=color, clip_flow=clip_flow, quiver=quiver, dominant=dominant)
    for stream, flow in _pushes(frames, ingest, net, render=spec, use_graph=use_graph):
        yield _rendered_dict(stream, flow, with_flow)


def flow_video_vanishing(net, frames: Iterable[np.ndarray], step: int = 16, scale: float = 1, min_mag: float = 1, use_graph: bool = True,
                         with_flow: bool = False, **vanishing) -> Iterator[dict]:
    """The per-frame loop of pwc_extract_flow_video_vanishpoint.py (process_video -> create_quiver_frame(..., draw_vanishing_point=True),
    :258-367, :502-530) up to the drawing: per consecutive pair of BGR uint8 frames a dict with the arrow grid "vec" (Gy,Gx,2) float32,
    "tip" (Gy,Gx,2) int32, "flags" (Gy,Gx) uint8 and "vanishing": (vx, vy, prob) as the reference's
    estimate_vanishing_point_from_flow(flow, step, min_mag) returns them, or None where it returns None.  Raw frames go up, the ingest,
    the network, the arrows and the estimate are one replay (RawFlowStream); **vanishing are VanishingEstimator's remaining arguments
    (max_points, grid_size, min_pairs, seed; vanishing.py says how its subsampling differs from np.random.choice).  with_flow=True adds
    "flow", flow_video's array.  The shrink canvas and the drawing are the caller's."""
    from .vanishing import to_host
    spec = RenderSpec(color=False, quiver=dict(step=step, scale=scale, min_mag=min_mag, style="video"))
    for raw, flow in _pushes(frames, "hip", net, render=spec, vanishing=dict(vanishing, min_mag=min_mag), use_graph=use_graph):
        out = _rendered_dict(raw, flow, with_flow)
        out["vanishing"] = to_host(raw.points)[0]
        yield out
