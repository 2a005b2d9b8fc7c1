"""cv2.warpPerspective-exact top-view warp on the device: the step of the reference's topview.py:218,232 that the cv2-exact pipeline
of cv_resize.py left with the caller, as one gather kernel (csrc/pwc_cv_warp.hip), its host helpers and two captured drivers.

    warp   : cv2.warpPerspective(frame, M, (width, height)) with the script's defaults INTER_LINEAR, BORDER_CONSTANT, border value 0
    M      : cv2.getPerspectiveTransform of the script's eight points (`topview_matrix`), inverted on the host (`invert3x3`)

"Exact" is equality with this project's statement of OpenCV's published algorithm (imgproc's warpPerspective plus the 8-bit bilinear
remap; written out in include/pwc_hip.h and as NumPy in tests/cv_warp_oracle.py): cv2 itself is not available here, so cv2 parity is
unpinned.  One point of the statement cannot be settled from the published source either: how OpenCV's int16 weight table stores the
single weight 32768 at a zero fraction on both axes; it is taken as 32768, so an identity warp returns the image.  The inverse map is
made here on the host in float64, uploaded once per (matrix, device) and kept; once it is resident (`prepare`, or one eager call) a
warp neither allocates a table nor synchronises and can be captured in a HIP graph.  There is no CPU fallback."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops
from .cv_resize import CvGraphedInfer, _check_frames


# ------------------------------------------------------------------ host helpers (no GPU, no torch needed)
def invert3x3(M) -> np.ndarray:
    """OpenCV's closed form of a 3x3 inverse in float64: the determinant by cofactor expansion along the first row, d = 1.0 / det,
    each adjugate entry times d.  A zero determinant (OpenCV: the zero matrix) and non-finite entries raise ValueError."""
    S = np.asarray(M, np.float64)
    if S.shape != (3, 3):
        raise ValueError("M must be 3x3, got %s" % (S.shape,))
    if not np.isfinite(S).all():
        raise ValueError("M must be finite")
    d = (S[0, 0] * (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) - S[0, 1] * (S[1, 0] * S[2, 2] - S[1, 2] * S[2, 0])
         + S[0, 2] * (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]))
    if d == 0.0:
        raise ValueError("M is singular")
    d = 1.0 / d
    t = np.empty((3, 3), np.float64)
    t[0, 0] = (S[1, 1] * S[2, 2] - S[1, 2] * S[2, 1]) * d
    t[0, 1] = (S[0, 2] * S[2, 1] - S[0, 1] * S[2, 2]) * d
    t[0, 2] = (S[0, 1] * S[1, 2] - S[0, 2] * S[1, 1]) * d
    t[1, 0] = (S[1, 2] * S[2, 0] - S[1, 0] * S[2, 2]) * d
    t[1, 1] = (S[0, 0] * S[2, 2] - S[0, 2] * S[2, 0]) * d
    t[1, 2] = (S[0, 2] * S[1, 0] - S[0, 0] * S[1, 2]) * d
    t[2, 0] = (S[1, 0] * S[2, 1] - S[1, 1] * S[2, 0]) * d
    t[2, 1] = (S[0, 1] * S[2, 0] - S[0, 0] * S[2, 1]) * d
    t[2, 2] = (S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]) * d
    return t


def perspective_matrix(src_pts, dst_pts) -> np.ndarray:
    """cv2.getPerspectiveTransform: the 8x8 system of the four float32 point pairs widened to double, solved with numpy.linalg.solve,
    c22 = 1.  Returns the forward map float64 [3,3] (source -> destination)."""
    src = np.asarray(src_pts, np.float32).astype(np.float64)
    dst = np.asarray(dst_pts, np.float32).astype(np.float64)
    if src.shape != (4, 2) or dst.shape != (4, 2):
        raise ValueError("src_pts and dst_pts must be four (x, y) points each")
    A, b = np.zeros((8, 8), np.float64), np.zeros(8, np.float64)
    for i in range(4):
        A[i, 0] = A[i + 4, 3] = src[i, 0]
        A[i, 1] = A[i + 4, 4] = src[i, 1]
        A[i, 2] = A[i + 4, 5] = 1.0
        A[i, 6] = -src[i, 0] * dst[i, 0]
        A[i, 7] = -src[i, 1] * dst[i, 0]
        A[i + 4, 6] = -src[i, 0] * dst[i, 1]
        A[i + 4, 7] = -src[i, 1] * dst[i, 1]
        b[i], b[i + 4] = dst[i, 0], dst[i, 1]
    return np.append(np.linalg.solve(A, b), 1.0).reshape(3, 3)


def topview_matrix(width: int, height: int) -> np.ndarray:
    """The side-camera -> top-view matrix of topview.py:57-76 (get_perspective_matrix) for one frame size: its eight points as float32."""
    src = np.float32([[width * 0.2, height * 0.8], [width * 0.8, height * 0.8], [width * 0.3, height * 0.4], [width * 0.7, height * 0.4]])
    dst = np.float32([[width * 0.2, height * 0.9], [width * 0.8, height * 0.9], [width * 0.2, height * 0.1], [width * 0.8, height * 0.1]])
    return perspective_matrix(src, dst)


def inverse_maps(M, inverse_map: bool = False) -> np.ndarray:
    """[3,3] or [n,3,3] array-like -> the destination -> source maps the kernel reads, float64 [9] or [n,9]: each matrix inverted
    (`invert3x3`), or taken as it is with inverse_map (cv2's WARP_INVERSE_MAP).  Non-finite entries raise ValueError."""
    S = np.asarray(M, np.float64)
    if S.shape[-2:] != (3, 3) or S.ndim not in (2, 3):
        raise ValueError("M must be [3,3] or [n,3,3], got %s" % (S.shape,))
    if not np.isfinite(S).all():
        raise ValueError("M must be finite")
    if not inverse_map:
        S = invert3x3(S) if S.ndim == 2 else np.stack([invert3x3(m) for m in S])
    return np.ascontiguousarray(S.reshape(S.shape[:-2] + (9,)))


# ------------------------------------------------------------------ resident device matrices
_MATS = {}


def prepare(M, device, inverse_map: bool = False) -> torch.Tensor:
    """Make the inverse map(s) of M resident on the device (what the first call does), e.g. before capturing a graph; returns them."""
    mi = inverse_maps(M, inverse_map)
    key = (mi.shape, mi.tobytes(), str(device))
    got = _MATS.get(key)
    if got is None:
        got = _MATS[key] = torch.from_numpy(mi).to(device)
    return got


# ------------------------------------------------------------------ operator
def warp_frames(frames_u8: torch.Tensor, M, dsize=None, inverse_map: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 frames [n,H,W,3] on the device -> uint8 [n,h,w,3]: cv2.warpPerspective(frame, M, (w, h)) per frame, one launch.  M: the
    forward map, [3,3] for all frames or [n,3,3], array-like in float64 (inverse_map: the destination -> source map itself).  dsize:
    (h, w) in this package's order (cv2 writes (w, h)); None keeps the source size, as topview.py does.  The frames may be a view with
    a larger batch stride, and `out` one half `buf[:, k]` of a pair buffer [n,2,h,w,3]."""
    _check_frames(frames_u8, 4, "frames_u8")
    n, H, W, _ = frames_u8.shape
    h, w = (H, W) if dsize is None else (int(dsize[0]), int(dsize[1]))
    mats = prepare(M, frames_u8.device, inverse_map)
    if mats.dim() == 2 and mats.shape[0] != n:
        raise ValueError("M holds %d matrices for %d frames" % (mats.shape[0], n))
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames_u8.device)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or out.device != frames_u8.device:
        raise ValueError("out must be uint8 %s on %s" % ((n, h, w, 3), frames_u8.device))
    return ops.cv_warp_perspective(frames_u8, mats, out)


# ------------------------------------------------------------------ captured drivers
class TopviewInfer(CvGraphedInfer):
    """topview.py's per-pair work from the decoded frames on as ONE HIP graph: warp (both frames of every pair, one launch) ->
    cv2-exact ingest -> net -> cv2-exact exit, CvGraphedInfer(mode="topview") with the warp in front.  ``__call__(raw_pairs_u8)`` takes
    raw BGR pairs uint8 [n<=batch,2,H,W,3] on the device and returns the flow [n,2,H,W] (a static buffer: consume or clone it before
    the next call).  ``warped`` [batch,2,H,W,3] is the static buffer of warped frames (``warped[:, 1]`` is the curr_frame_warped the
    script draws on; consume or clone), ``x_in`` the input the model saw, ``flow_quarter`` its output.  M: the forward map [3,3]
    (`topview_matrix(width, height)` for the script's)."""

    def __init__(self, net, height: int, width: int, device, M, batch: int = 1):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("TopviewInfer needs a ROCm device: the HIP path has no CPU fallback")
        if np.asarray(M).shape != (3, 3):
            raise ValueError("M must be one 3x3 matrix")
        self.M = np.array(M, np.float64)
        self.mats = prepare(self.M, device)                                     # resident before the capture
        super().__init__(net, height, width, device, batch=batch, mode="topview")

    def _alloc_outputs(self, height: int, width: int, device) -> None:
        super()._alloc_outputs(height, width, device)
        self.warped = torch.zeros((self.batch, 2, height, width, 3), dtype=torch.uint8, device=device)

    def _warp(self) -> None:
        h, w = self.static_u8.shape[2:4]
        ops.cv_warp_perspective(self.static_u8.view(2 * self.batch, h, w, 3), self.mats, self.warped.view(2 * self.batch, h, w, 3))

    def _pairs(self) -> torch.Tensor:
        self._warp()                                                            # CvGraphedInfer's body, fed the warped pairs
        return self.warped


class _StreamInfer(TopviewInfer):
    """TopviewStream's graph: static_u8[0, 1] is the raw new frame; slot 0 of `warped` is carried from the previous replay."""

    def _warp(self) -> None:
        ops.cv_warp_perspective(self.static_u8[:, 1], self.mats, self.warped[:, 1])

    def _body(self) -> torch.Tensor:
        out = super()._body()
        self.warped[:, 0].copy_(self.warped[:, 1])                              # the graph's last node: this frame is the next one's previous
        return out


class TopviewStream:
    """topview.py:212-255 frame by frame, each frame warped once: ``prime(frame_u8)`` warps the first frame [H,W,3] (raw BGR, uint8,
    on the device) into slot 0; every ``push(frame_u8)`` returns the flow [1,2,H,W] from the previous frame to this one with ONE graph
    replay, which warps the new frame into slot 1, runs ingest, net and exit on the two slots, and ends by copying slot 1 to slot 0.
    ``warped_current`` [H,W,3] is slot 1 as that push left it, the curr_frame_warped the script draws on.  The flow and
    ``warped_current`` are static buffers: consume or clone them before the next push."""

    def __init__(self, net, height: int, width: int, device, M):
        self._pipe = _StreamInfer(net, height, width, device, M, batch=1)
        self._primed = False

    def _check(self, frame_u8: torch.Tensor) -> None:
        want = tuple(self._pipe.static_u8.shape[2:])
        if not torch.is_tensor(frame_u8) or frame_u8.dtype != torch.uint8 or tuple(frame_u8.shape) != want or not frame_u8.is_cuda:
            raise ValueError("expected a uint8 device frame %s" % (want,))

    @property
    def warped_current(self) -> torch.Tensor:
        return self._pipe.warped[0, 1]

    def prime(self, frame_u8: torch.Tensor) -> None:
        self._check(frame_u8)
        ops.cv_warp_perspective(frame_u8.unsqueeze(0), self._pipe.mats, self._pipe.warped[:, 0])
        self._primed = True

    def push(self, frame_u8: torch.Tensor) -> torch.Tensor:
        self._check(frame_u8)
        if not self._primed:
            raise ValueError("prime() the stream with the first frame before push()")
        self._pipe.static_u8[0, 1].copy_(frame_u8, non_blocking=True)
        self._pipe.graph.replay()
        return self._pipe.out
