"""Vanishing point of a flow field on the device: estimate_vanishing_point_from_flow of pwc_extract_flow_video_vanishpoint.py:93-255
(what create_quiver_frame(..., draw_vanishing_point=True) computes per frame), batched, as HIP kernels (csrc/pwc_vanishing.hip).

The input is the arrow grid of ``flowviz.quiver_arrows`` (style "video"): its ``vec`` is exactly the ``flow[y, x]`` the reference
samples every `step` pixels after its resize to the frame.  Pair intersections, the weighted 64 x 64 vote, the best bin and the
least-squares refinement all run on the device in fp64; results stay there and nothing synchronises.

One thing differs from the reference by necessity.  When more than `max_points` vectors pass `min_mag` the reference subsamples with
``np.random.choice`` on NumPy's global state.  Here the subset is decided by ``order_table(cells, seed)``, a permutation of the grid
cells drawn once per (cells, seed) with ``np.random.default_rng(seed)`` and kept on the device: the kept cells are ranked by their
position in it and the first `max_points` are used, in that order.  That is a uniform random subset too, and the same one on every run.

``to_host`` turns a result into the reference's return values, ``(vx, vy, prob)`` or ``None`` per frame, in one download.
"""
from __future__ import annotations

import threading
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import flowviz, ops

__all__ = ["VanishingEstimator", "VanishingPoints", "order_table", "to_host", "vanishing_point", "vanishing_point_from_flow"]

_TABLES: Dict[Tuple[int, int], np.ndarray] = {}
_DEVICE_TABLES: Dict[Tuple[int, int, str], torch.Tensor] = {}
_LOCK = threading.Lock()


class VanishingPoints(NamedTuple):
    xy: torch.Tensor       # float64 [B,2]  refined (vx, vy); the bin centre when status is 1; NaN when status >= 2
    prob: torch.Tensor     # float64 [B]    votes of the best bin / all votes; 0 when status >= 2
    center: torch.Tensor   # float64 [B,2]  centre of the best bin
    info: torch.Tensor     # int32   [B,6]  status, N used, pairs kept, best gx, best gy, inliers

    @property
    def ok(self) -> torch.Tensor:
        """bool [B]: the reference would have returned a point (status 0 refined, 1 bin centre kept)."""
        return self.info[:, 0] <= 1


def order_table(cells: int, seed: int = 0) -> np.ndarray:
    """int32 [cells]: ``np.random.default_rng(seed).permutation(cells)``, cached per (cells, seed)."""
    key = (int(cells), int(seed))
    with _LOCK:
        t = _TABLES.get(key)
        if t is None:
            t = np.random.default_rng(int(seed)).permutation(int(cells)).astype(np.int32)
            _TABLES[key] = t
    return t


def _device_order(cells: int, seed: int, device: torch.device) -> torch.Tensor:
    key = (int(cells), int(seed), str(device))
    with _LOCK:
        t = _DEVICE_TABLES.get(key)
    if t is None:
        t = torch.from_numpy(order_table(cells, seed)).to(device)
        with _LOCK:
            _DEVICE_TABLES[key] = t
    return t


def _grid(frame_hw, step: int) -> Tuple[int, int, int, int]:
    H, W, step = int(frame_hw[0]), int(frame_hw[1]), int(step)
    if step < 1:
        raise ValueError("step must be >= 1, got %d" % step)
    if H < 1 or W < 1:
        raise ValueError("frame size must be positive, got %dx%d" % (H, W))
    return H, W, (H + step - 1) // step, (W + step - 1) // step


def _points(vp: torch.Tensor, info: torch.Tensor) -> VanishingPoints:
    return VanishingPoints(vp[:, 0:2], vp[:, 2], vp[:, 3:5], info)


def vanishing_point(vec: torch.Tensor, frame_hw: Tuple[int, int], step: int = 16, min_mag: float = 1.0, max_points: int = 300,
                    grid_size: int = 64, min_pairs: int = 50, seed: int = 0, out=None) -> VanishingPoints:
    """Vanishing point per frame from the arrow grid vec float32 [B,Gy,Gx,2] (``quiver_arrows(...).vec`` of an (H, W) frame at this
    step).  The defaults are the reference's.  vec must be contiguous (a strided view is refused).  out: optional (vp float64 [B,5],
    info int32 [B,6]) to write into; the fields of the result are views of them."""
    H, W, gy, gx = _grid(frame_hw, step)
    order = _device_order(gy * gx, seed, vec.device) if gy * gx > int(max_points) and vec.is_cuda else None
    vp, info = ops.vanishing_point(vec, H, W, step, min_mag, max_points, grid_size, min_pairs, order=order, out=out)
    return _points(vp, info)


def vanishing_point_from_flow(flow: torch.Tensor, frame_hw: Tuple[int, int], step: int = 16, min_mag: float = 1.0,
                              crop: Optional[Tuple[int, int]] = None, **kw) -> VanishingPoints:
    """The same from the network's flow [B,2,Hq,Wq]: ``quiver_arrows`` (style "video", the top-left `crop` resized to the frame and
    scaled as create_quiver_frame does) and then ``vanishing_point``; **kw are its remaining arguments."""
    arrows = flowviz.quiver_arrows(flow, frame_hw, step=step, min_mag=min_mag, crop=crop, style="video")
    return vanishing_point(arrows.vec, frame_hw, step=step, min_mag=min_mag, **kw)


class VanishingEstimator:
    """The kernels on static buffers for arrow grids of one geometry: `run(vec)` launches them on the current stream and allocates
    nothing, so it can sit inside a HIP graph capture.  The outputs are reused by every run."""

    def __init__(self, batch: int, frame_hw: Tuple[int, int], step: int = 16, min_mag: float = 1.0, max_points: int = 300,
                 grid_size: int = 64, min_pairs: int = 50, seed: int = 0, device=None):
        self.frame_h, self.frame_w, self.gy, self.gx = _grid(frame_hw, step)
        self.batch, self.step, self.min_mag = int(batch), int(step), float(min_mag)
        self.max_points, self.grid_size, self.min_pairs = int(max_points), int(grid_size), int(min_pairs)
        device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        need = ops.vanishing_workspace_bytes(self.batch, self.gy, self.gx, self.grid_size)
        self.vp = torch.empty((self.batch, 5), dtype=torch.float64, device=device)
        self.info = torch.empty((self.batch, 6), dtype=torch.int32, device=device)
        self.workspace = torch.empty((need + 7) // 8, dtype=torch.int64, device=device)
        self.order = _device_order(self.gy * self.gx, seed, device) if self.gy * self.gx > self.max_points else None
        self.points = _points(self.vp, self.info)

    def run(self, vec: torch.Tensor) -> VanishingPoints:
        if vec.shape[0] != self.batch:
            raise ValueError("vec has batch %d, the estimator was built for %d" % (vec.shape[0], self.batch))
        ops.vanishing_point(vec, self.frame_h, self.frame_w, self.step, self.min_mag, self.max_points, self.grid_size, self.min_pairs,
                            order=self.order, out=(self.vp, self.info), workspace=self.workspace)
        return self.points


def to_host(vp: VanishingPoints) -> List[Optional[Tuple[float, float, float]]]:
    """Per frame what the reference returns: (vx, vy, prob) as Python floats, or None where it would have returned None.  One
    device-to-host copy (a failed frame is the one whose vx is NaN)."""
    rows = torch.cat([vp.xy, vp.prob[:, None]], dim=1).cpu().tolist()
    return [None if r[0] != r[0] else (r[0], r[1], r[2]) for r in rows]
