"""Epipolar hard mask and soft Sampson penalty of train_fundamental.py (reference :169-382, used at :459-483), batched on HIP.

Names and defaults follow the reference; every function takes a batch and runs on ROCm device tensors only (no CPU fallback --
the NumPy restatement lives in tests/epipolar_oracle.py).  The RANSAC hypotheses use the reference's own sampler,
``numpy.random.default_rng(seed).choice(N, 8, replace=False)`` once per iteration, so the index sequence depends only on
(N, seed): it is generated on the host, cached per (N, seed) with the longest prefix asked for so far, and uploaded once per
device.  Because an image mask or a non-finite flow changes N, ``ransac_fundamental`` (and ``build_epipolar_mask_from_flow``,
which calls it) reads the per-sample N back once per call -- a B x int32 device-to-host copy and the only synchronisation of this
module.  Everything after it (hypotheses, scoring, refit, distance map, quantile threshold, mask, soft loss and its backward)
stays on the device.
"""
from __future__ import annotations

import threading
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import ops
from ._lib import PwcHipError

_TABLES: Dict[Tuple[int, int], np.ndarray] = {}
_DEVICE_TABLES: Dict[Tuple[int, int, str], torch.Tensor] = {}
_LOCK = threading.Lock()


def index_table(N: int, seed: int, iters: int) -> np.ndarray:
    """int32 [iters, 8]: row i = the i-th ``rng.choice(N, size=8, replace=False)`` of ``rng = np.random.default_rng(seed)``
    (train_fundamental.py:240-245).  Cached per (N, seed); a shorter request is a prefix of a longer one."""
    key = (int(N), int(seed))
    with _LOCK:
        t = _TABLES.get(key)
        if t is None or t.shape[0] < iters:
            rng = np.random.default_rng(seed)
            t = np.stack([rng.choice(N, size=8, replace=False) for _ in range(iters)]).astype(np.int32)
            _TABLES[key] = t
            for k in [k for k in _DEVICE_TABLES if k[:2] == key]:
                del _DEVICE_TABLES[k]
    return t[:iters]


def _device_table(N: int, seed: int, iters: int, device: torch.device) -> torch.Tensor:
    key = (int(N), int(seed), str(device))
    with _LOCK:
        t = _DEVICE_TABLES.get(key)
    if t is None or t.shape[0] < iters:
        index_table(N, seed, iters)
        t = torch.from_numpy(np.ascontiguousarray(_TABLES[(int(N), int(seed))])).to(device)
        with _LOCK:
            _DEVICE_TABLES[key] = t
    return t[:iters]


def _require_device(t: torch.Tensor, name: str) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PwcHipError("%s must be a ROCm device tensor: the epipolar path is HIP only (no CPU fallback)" % name)


def ransac_fundamental_ex(flow_full: torch.Tensor, stride: int = 4, thresh: float = 0.5, max_iters: int = 2000, seed: int = 0,
                          mask: Optional[torch.Tensor] = None):
    """ransac_fundamental plus its by-products: (F [B,3,3] f64, ok [B] bool, best [B] int32, counts [B,max_iters] int32,
    N [B] host int list)."""
    _require_device(flow_full, "flow_full")
    flow = flow_full.detach().float()
    pts, n = ops.epipolar_pairs(flow, stride, mask)
    N = [int(v) for v in n.cpu().tolist()]          # the one host synchronisation (see the module docstring)
    B, iters = flow.shape[0], int(max_iters)
    if iters < 1:
        raise ValueError("max_iters must be >= 1")
    usable = sorted({v for v in N if v >= 8})
    if len(usable) <= 1 and len(set(N)) == 1:
        idx = _device_table(usable[0], seed, iters, flow.device) if usable else \
            torch.zeros((iters, 8), dtype=torch.int32, device=flow.device)
    else:
        zero = torch.zeros((iters, 8), dtype=torch.int32, device=flow.device)
        idx = torch.stack([_device_table(v, seed, iters, flow.device) if v >= 8 else zero for v in N])
    F, ok, best, counts = ops.epipolar_ransac(pts, n, idx, thresh)
    return F.view(B, 3, 3), ok.bool(), best, counts, N


def ransac_fundamental(flow_full: torch.Tensor, stride: int = 4, thresh: float = 0.5, max_iters: int = 2000, seed: int = 0,
                       mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """_flow_to_pairs + _ransac_F (train_fundamental.py:169-258) per sample of flow_full [B,2,H,W]: (F float64 [B,3,3],
    ok bool [B]).  ok is False where the reference raises (N < 8 or fewer than 8 inliers); F is 0 there."""
    F, ok, _, _, _ = ransac_fundamental_ex(flow_full, stride, thresh, max_iters, seed, mask)
    return F, ok


def sampson_distance(flow_full: torch.Tensor, F) -> torch.Tensor:
    """_sampson_distance of every pixel (train_fundamental.py:285-296): float64 [B,H,W] for F [3,3] (numpy or torch) or [B,3,3]."""
    _require_device(flow_full, "flow_full")
    return ops.epipolar_distance(flow_full.detach().float(), F)


def build_epipolar_mask_from_flow(flow_full: torch.Tensor, tau: float = 1.0, stride: int = 4,
                                  img_mask_bhw: Optional[torch.Tensor] = None, keep_ratio: float = 0.2,
                                  min_keep: float = 0.05, return_thr: bool = False):
    """build_epipolar_mask_from_flow (train_fundamental.py:261-327) for any batch: bool [B,1,H,W], True = keep; all True for a
    sample whose fit fails or whose distances are all non-finite.  return_thr adds the per-sample threshold (float64 [B], NaN
    for those all-true samples)."""
    _require_device(flow_full, "flow_full")
    flow = flow_full.detach().float()
    F, ok = ransac_fundamental(flow, stride=stride, thresh=0.5, max_iters=2000, seed=0, mask=img_mask_bhw)
    mask, thr = ops.epipolar_mask(flow, F.view(-1, 9), ok, tau, keep_ratio, min_keep)
    return (mask, thr) if return_thr else mask


def epipolar_sampson_loss(flow_full: torch.Tensor, F, valid_mask: Optional[torch.Tensor] = None, robust: str = "huber",
                          delta: float = 1.0, weight: float = 0.1, ok=None) -> torch.Tensor:
    """epipolar_sampson_loss (train_fundamental.py:331-382): weight * mean over pixels with valid_mask > 0.5 of huber(delta) /
    l1 / plain Sampson distance, F rounded to float32.  F: numpy or torch [3,3] (all samples) or torch [B,3,3].  ok (bool scalar
    or [B], device or host): samples whose fit failed select nothing, so a failed single fit gives exactly 0 -- the term the
    script does not add.  Differentiable w.r.t. flow_full (ops.EpipolarSampsonFunction)."""
    _require_device(flow_full, "flow_full")
    return ops.EpipolarSampsonFunction.apply(flow_full, F, ok, valid_mask, robust, delta, weight)
