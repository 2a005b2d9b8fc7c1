"""cv2.resize-exact (INTER_LINEAR) ingest and flow exit on the device: the image-space steps of the reference's script_pwc.py:43-83 and
topview.py:79-119 (compute_flow) as two kernels (csrc/pwc_cv_resize.hip) and one captured pipeline.

    ingest : both frames cv2.resize'd to multiples of 64, channel order flipped, / 255, HWC -> CHW, stacked to [n,6,H_,W_]
    exit   : flow2 * gain (20 in script_pwc.py, 1 in topview.py), u and v cv2.resize'd to (W, H), u *= W / W_, v *= H / H_

"Exact" is equality with this project's statement of OpenCV's published algorithm (harness.py's docstring, pinned by
tests/test_harness.py): cv2 itself is not available here, so cv2 parity is unpinned.  The per-axis tables are made here on the host
(`axis_table`), uploaded once per (input length, output length, device) and kept; the kernels only apply them.  Once the tables of a
geometry are resident (`prepare`, or one eager call) the calls neither allocate tables nor synchronise and can be captured in a HIP
graph.  The byte -> float table is made with the IEEE division both scripts use (`byte_lut`): float32(v) / float32(255), which is
float32(float64(v) / 255.0) for every byte, whereas a multiplication by the float reciprocal (what `t / 255.0` is on the device)
differs from it for 126 of the 256 bytes.  There is no CPU fallback."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from .harness import padded_size
from .kitti import GraphedInfer


# ------------------------------------------------------------------ host tables (no GPU needed)
def axis_table(src: int, dst: int) -> Tuple[np.ndarray, np.ndarray]:
    """cv::resize's xofs / alpha of one axis for INTER_LINEAR: (first tap s0 int32 [dst], weight fx float32 [dst] of the second tap
    min(s0 + 1, src - 1)).  Double scale, float fx; a tap clamped at either end gets fx = 0."""
    src, dst = int(src), int(dst)
    if src <= 0 or dst <= 0:
        raise ValueError("sizes must be positive, got %d -> %d" % (src, dst))
    scale = 1.0 / (float(dst) / float(src))                                     # scale_x = 1. / inv_scale_x, in double
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx)
    fx = (fx - sx).astype(np.float32)
    sx = sx.astype(np.int64)
    lo, hi = sx < 0, sx >= src - 1
    fx[lo | hi] = np.float32(0)
    sx[lo] = 0
    sx[hi] = src - 1
    return sx.astype(np.int32), fx


def byte_lut(mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None) -> torch.Tensor:
    """float32 [3, 256] on the host: float32(v) / float32(255) by IEEE division for every byte value, and with mean / std
    (lut - float32(mean[c])) / float32(std[c]) per OUTPUT channel c, in float32."""
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    lut = np.repeat((np.arange(256, dtype=np.float32) / np.float32(255))[None], 3, axis=0)
    if mean is not None:
        m, s = np.asarray(mean, np.float32).reshape(-1), np.asarray(std, np.float32).reshape(-1)
        if m.size != 3 or s.size != 3 or (s == 0).any():
            raise ValueError("mean / std must have three entries and std no zero")
        lut = ((lut - m[:, None]) / s[:, None]).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(lut, dtype=np.float32))


# ------------------------------------------------------------------ resident device tables
_TABLES = {}
_LUTS = {}


def _axis(src: int, dst: int, device):
    key = (int(src), int(dst), str(device))
    got = _TABLES.get(key)
    if got is None:
        s0, fx = axis_table(src, dst)
        got = _TABLES[key] = (torch.from_numpy(s0).to(device), torch.from_numpy(fx).to(device))
    return got


def _lut(lut: Optional[torch.Tensor], device) -> torch.Tensor:
    if lut is not None and (not torch.is_tensor(lut) or lut.dtype != torch.float32 or tuple(lut.shape) != (3, 256)):
        raise ValueError("lut must be a float32 [3,256] tensor")
    if lut is not None and lut.is_cuda:
        return lut
    key = (None if lut is None else lut.contiguous().numpy().tobytes(), str(device))
    got = _LUTS.get(key)
    if got is None:
        got = _LUTS[key] = (byte_lut() if lut is None else lut.contiguous()).to(device)
    return got


def prepare(in_hw, out_hw, device, lut: Optional[torch.Tensor] = None) -> None:
    """Make the tables of one geometry resident (what the first call does), e.g. before capturing a graph."""
    _axis(in_hw[1], out_hw[1], device)
    _axis(in_hw[0], out_hw[0], device)
    _lut(lut, device)


# ------------------------------------------------------------------ operators
def _check_frames(t: torch.Tensor, dims: int, name: str) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() != dims or t.shape[-1] != 3 or (dims == 5 and t.shape[1] != 2):
        raise ValueError("%s must be uint8 %s" % (name, "[n,2,H,W,3]" if dims == 5 else "[n,H,W,3]"))
    if not t.is_cuda:
        raise ValueError("%s must be on the device: the HIP path has no CPU fallback" % name)


def resize_frames(frames_u8: torch.Tensor, size=None, flip_channels: bool = True, lut: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames [n,H,W,3] on the device -> float32 [n,3,h,w]: cv2.resize(frame, (w, h)), [:, :, ::-1] when flip_channels, the byte
    table (default / 255), HWC -> CHW, as one kernel.  size None: harness.padded_size (multiples of 64).  `out` may be a channel slice of
    a wider tensor (e.g. x[:, 3:6]); lut: float32 [3,256] on the host (uploaded once and kept) or on the device."""
    from . import ops
    _check_frames(frames_u8, 4, "frames_u8")
    n, H, W, _ = frames_u8.shape
    h, w = padded_size(H, W) if size is None else (int(size[0]), int(size[1]))
    dev = frames_u8.device
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
    return ops.cv_resize_frames(frames_u8.contiguous(), (h, w), _axis(W, w, dev), _axis(H, h, dev), _lut(lut, dev), out,
                                flip_channels, n)


def ingest_pairs(pairs_u8: torch.Tensor, flip_channels: bool = True, lut: Optional[torch.Tensor] = None, size=None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 pairs [n,2,H,W,3] on the device -> the [n,6,H_,W_] network input in one launch (script_pwc.py:43-65; topview.py:79-101
    with flip_channels on BGR frames).  `out`: a contiguous float32 [n,6,H_,W_] tensor to fill."""
    from . import ops
    _check_frames(pairs_u8, 5, "pairs_u8")
    n, _, H, W, _ = pairs_u8.shape
    h, w = padded_size(H, W) if size is None else (int(size[0]), int(size[1]))
    dev = pairs_u8.device
    if out is None:
        out = torch.empty((n, 6, h, w), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n, 6, h, w) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 %s tensor" % ((n, 6, h, w),))
    # a dense [n,6,h,w] is [2n,3,h,w]: frame 2b + k lands in channels 3k .. 3k+2 of item b
    ops.cv_resize_frames(pairs_u8.contiguous().view(2 * n, H, W, 3), (h, w), _axis(W, w, dev), _axis(H, h, dev), _lut(lut, dev),
                         out.view(2 * n, 3, h, w), flip_channels, 2 * n)
    return out


def resize_flow(flow: torch.Tensor, size, gain: float = 1.0, scale_vectors: bool = True, layout: str = "chw",
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The exit of script_pwc.py:72-81 / topview.py:104-117 for a batch: flow [n,2,H_/4,W_/4] (the network's output for an [H_,W_]
    input) -> (flow * gain) cv2.resize'd to size = (H, W), then with scale_vectors u * float32(W / W_) and v * float32(H / H_).
    layout "chw": [n,2,H,W]; "hwc": [n,H,W,2] (what write_flo takes per item)."""
    from . import ops
    if layout not in ("chw", "hwc"):
        raise ValueError("layout must be 'chw' or 'hwc', got %r" % (layout,))
    if not torch.is_tensor(flow) or flow.dim() != 4 or flow.shape[1] != 2 or flow.dtype != torch.float32:
        raise ValueError("flow must be float32 [n,2,h,w]")
    if not flow.is_cuda:
        raise ValueError("flow must be on the device: the HIP path has no CPU fallback")
    H, W = int(size[0]), int(size[1])
    h, w = flow.shape[2:]
    fu, fv = (W / float(4 * w), H / float(4 * h)) if scale_vectors else (1.0, 1.0)
    dev = flow.device
    return ops.cv_resize_flow(flow, (H, W), _axis(w, W, dev), _axis(h, H, dev), gain, float(np.float32(fu)), float(np.float32(fv)),
                              layout == "hwc", out)


MODES = {"script": dict(gain=20.0, layout="hwc"),      # script_pwc.py: RGB in (imageio), BGR to the net, x 20, [H,W,2] for write_flo
         "topview": dict(gain=1.0, layout="chw")}      # topview.py: BGR in (cv2 video frames), RGB to the net, no gain


class CvGraphedInfer(GraphedInfer):
    """cv2-exact ingest -> net -> cv2-exact exit for one fixed frame size as ONE HIP graph (kitti.GraphedInfer's capture scaffolding
    with this module's two kernels around the model).  ``__call__(pairs_u8)`` takes uint8 pairs [n<=batch,2,H,W,3] on the device and
    returns a static buffer (consume or clone it before the next call): mode "script" [n,H,W,2] = flow * 20 in pixels of the frame,
    mode "topview" [n,2,H,W] without the gain.  Both flip the channel order of the frames (RGB -> BGR in script_pwc.py, BGR -> RGB in
    topview.py) and scale u by float32(W / W_) and v by float32(H / H_).  ``x_in`` [batch,6,H_,W_] is the input the model saw,
    ``flow_quarter`` its output."""

    def __init__(self, net, height: int, width: int, device, batch: int = 1, mode: str = "script"):
        if mode not in MODES:
            raise ValueError("mode must be one of %s, got %r" % (sorted(MODES), mode))
        self.mode = mode
        super().__init__(net, height, width, torch.device(device), batch=batch)

    def _alloc_outputs(self, height: int, width: int, device) -> None:
        hwc = MODES[self.mode]["layout"] == "hwc"
        self.flow_full = torch.empty((self.batch, height, width, 2) if hwc else (self.batch, 2, height, width), dtype=torch.float32,
                                     device=device)
        h_, w_ = padded_size(height, width)
        prepare((height, width), (h_, w_), device)                              # resident before the capture
        prepare((h_ // 4, w_ // 4), (height, width), device)

    def _pairs(self) -> torch.Tensor:
        """The uint8 pairs [batch,2,H,W,3] the ingest reads (a subclass prepares them first)."""
        return self.static_u8

    def _body(self) -> torch.Tensor:
        h, w = self.static_u8.shape[2:4]
        flow = self._forward(ingest_pairs(self._pairs(), True, out=self.x_in))
        m = MODES[self.mode]
        return resize_flow(flow, (h, w), m["gain"], True, m["layout"], out=self.flow_full)
