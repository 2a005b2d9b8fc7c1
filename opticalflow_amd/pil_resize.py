"""Pillow-exact bilinear resize on the device: the host-only first stage of train_pseudo.py / train_fundamental.py / inference.py
(transforms.Resize -> ToTensor -> Normalize on 8-bit frames) and inference.py's resize_flow (Pillow on float planes), bit for bit.

The coefficient tables are made here on the host (`coeff_tables`, `fixed_point`: Python floats are C doubles and int() truncates like
the C cast, so they are Pillow's), uploaded once per (input length, output length, device) and kept; the kernels of
csrc/pwc_pil_resize.hip only apply them.  Once the tables of a geometry are resident, `resize_frames` / `resize_flow` neither
allocate tables nor synchronise and can be captured in a HIP graph.  There is no CPU fallback: outside the supported scale range
(ops.pil_resize_supported) the calls raise.

Two rules of Image.resize sit above its two passes.  It takes no pass on an axis whose length does not change: the planes kernel
copies there (the frames kernel's identity table is exact on bytes).  And it takes the vertical pass first when the source is more
than 100 times as tall as wide and its height shrinks (`vertical_first`): the kernels are horizontal-first, so that regime is
composed here from two launches, (H, W) -> (h, W) and (h, W) -> (h, w), each a one-axis resize."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from ._pipeline import PinnedRing

PRECISION_BITS = 22          # 32 - 8 - 2: Pillow's fixed point for 8-bit images
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------ host tables (no GPU needed)
def ksize(in_size: int, out_size: int) -> int:
    """Length of one coefficient row: 2 * ceil(support) + 1 with support = max(in / out, 1)."""
    return 2 * int(math.ceil(max(in_size / out_size, 1.0))) + 1


def coeff_tables(in_size: int, out_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's BILINEAR coefficients of one axis: bounds int32 [out, 2] = (first tap, number of taps) and float64 [out, ksize]
    weights, normalised by their sum in tap order, zero past the last tap."""
    if in_size <= 0 or out_size <= 0:
        raise ValueError("sizes must be positive, got %d -> %d" % (in_size, out_size))
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ks = ksize(in_size, out_size)
    inv = 1.0 / fs
    bounds = np.zeros((out_size, 2), np.int32)
    coeffs = np.zeros((out_size, ks), np.float64)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        ww = 0.0
        row = []
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * inv
            if t < 0.0:
                t = -t
            w = 1.0 - t if t < 1.0 else 0.0
            row.append(w)
            ww += w
        if ww != 0.0:
            row = [w / ww for w in row]
        bounds[xx] = (xmin, xmax)
        coeffs[xx, :xmax] = row
    return bounds, coeffs


def fixed_point(coeffs: np.ndarray) -> np.ndarray:
    """The 8-bit path's int32 coefficients: (int)(w * 2^22 + 0.5), or - 0.5 for a negative one (truncation toward zero)."""
    c = np.asarray(coeffs, np.float64)
    return np.trunc(c * float(1 << PRECISION_BITS) + np.where(c < 0.0, -0.5, 0.5)).astype(np.int32)


def norm_lut(mean: Optional[Sequence[float]] = None, std: Optional[Sequence[float]] = None) -> torch.Tensor:
    """float32 [3, 256] on the host: ToTensor (float(u8) / 255) and, with mean / std, Normalize ((v - mean[c]) / std[c]) of every byte
    value, made with torch's own CPU operators so that indexing it equals running them."""
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
    if mean is None:
        return v.expand(3, 256).contiguous()
    m = torch.as_tensor([float(x) for x in mean], dtype=torch.float32)
    s = torch.as_tensor([float(x) for x in std], dtype=torch.float32)
    if m.numel() != 3 or s.numel() != 3 or bool((s == 0).any()):
        raise ValueError("mean / std must have three entries and std no zero")
    return v.expand(3, 256).clone().sub_(m[:, None]).div_(s[:, None])


# ------------------------------------------------------------------ resident device tables
_TABLES = {}
_LUTS = {}
_FACTORS = {}


def _axis_tables(in_size: int, out_size: int, fixed: bool, device):
    key = (in_size, out_size, fixed, str(device))
    got = _TABLES.get(key)
    if got is None:
        b, c = coeff_tables(in_size, out_size)
        k = fixed_point(c) if fixed else c
        got = (torch.from_numpy(b).to(device), torch.from_numpy(k).to(device), c.shape[1])
        _TABLES[key] = got
    return got


def _lut(mean, std, device) -> torch.Tensor:
    key = (None if mean is None else tuple(float(x) for x in mean), None if std is None else tuple(float(x) for x in std), str(device))
    got = _LUTS.get(key)
    if got is None:
        got = _LUTS[key] = norm_lut(mean, std).to(device)
    return got


def _size(size) -> Tuple[int, int]:
    h, w = (int(v) for v in size)
    return h, w


def _check_supported(in_hw, out_hw) -> None:
    from . import ops
    if not ops.pil_resize_supported(in_hw, out_hw):
        raise ValueError("resize %dx%d -> %dx%d is outside the supported range (a downscale of at most 8 per axis, more only to an "
                         "output shorter than a tile); there is no fallback" % (in_hw[0], in_hw[1], out_hw[0], out_hw[1]))


def vertical_first(in_hw, out_hw) -> bool:
    """Image.resize's pass order (the end of PIL/Image.py's resize): the vertical pass first when H > 100 * W and h < H."""
    return in_hw[0] > 100 * in_hw[1] and out_hw[0] < in_hw[0]


def _steps(in_hw, out_hw):
    """The launches of one resize as (source size, target size): one, or for a tall source the vertical pass and then the horizontal."""
    if vertical_first(in_hw, out_hw):
        mid = (out_hw[0], in_hw[1])
        return ((tuple(in_hw), mid), (mid, tuple(out_hw)))
    return ((tuple(in_hw), tuple(out_hw)),)


def prepare(in_hw, out_hw, device, frames: bool = True, mean=None, std=None) -> None:
    """Make the tables of one geometry resident (what the first call does), e.g. before capturing a graph."""
    _check_supported(in_hw, out_hw)
    for src, dst in _steps(in_hw, out_hw):
        _axis_tables(src[1], dst[1], frames, device)
        _axis_tables(src[0], dst[0], frames, device)
    if frames:
        _lut(mean, std, device)


# ------------------------------------------------------------------ operators
def _resize_frames(frames_u8: torch.Tensor, size, mean, std, out: torch.Tensor, out_u8: Optional[torch.Tensor], group: int):
    from . import ops
    n, H, W, _ = frames_u8.shape
    h, w = size
    _check_supported((H, W), (h, w))
    dev = frames_u8.device
    if vertical_first((H, W), (h, w)):
        # Pillow's order for a tall source: the vertical pass alone, its bytes kept (the float planes of this launch are not used)
        mid = torch.empty((n, h, W, 3), dtype=torch.uint8, device=dev)
        ops.pil_resize_frames(frames_u8, (h, W), _axis_tables(W, W, True, dev), _axis_tables(H, h, True, dev), _lut(mean, std, dev),
                              torch.empty((n, 3, h, W), dtype=torch.float32, device=dev), mid, n)
        frames_u8, H = mid, h
    xt = _axis_tables(W, w, True, dev)
    yt = _axis_tables(H, h, True, dev)
    return ops.pil_resize_frames(frames_u8, (h, w), xt, yt, _lut(mean, std, dev), out, out_u8, group)


def resize_frames(frames_u8: torch.Tensor, size, mean=None, std=None, out: Optional[torch.Tensor] = None, return_u8: bool = False):
    """uint8 RGB frames [n,H,W,3] on the device -> float32 [n,3,h,w]: Image.resize((w, h), BILINEAR) + ToTensor, and with mean / std
    Normalize, as one kernel.  `out` may be a channel slice of a larger tensor (e.g. x[:, 3:6]).  return_u8: also the resized bytes
    [n,h,w,3] (what Pillow returns), as a second result."""
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or frames_u8.dtype != torch.uint8:
        raise ValueError("frames_u8 must be uint8 [n,H,W,3], got %s %s" % (frames_u8.dtype, tuple(frames_u8.shape)))
    h, w = _size(size)
    n = frames_u8.shape[0]
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=frames_u8.device)
    u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device=frames_u8.device) if return_u8 else None
    _resize_frames(frames_u8, (h, w), mean, std, out, u8, n)
    return (out, u8) if return_u8 else out


def _factor_table(factors, c: int, device) -> Optional[torch.Tensor]:
    """The per-channel factors rounded to float32 as a resident device table (None without factors)."""
    if factors is None:
        return None
    key = (tuple(float(np.float32(f)) for f in factors), str(device))
    if len(key[0]) != c:
        raise ValueError("factors must have one entry per channel (%d), got %d" % (c, len(key[0])))
    fac = _FACTORS.get(key)
    if fac is None:
        fac = _FACTORS[key] = torch.tensor(key[0], dtype=torch.float32).to(device)
    return fac


def resize_planes(x: torch.Tensor, size, factors: Optional[Sequence[float]] = None) -> torch.Tensor:
    """float32 planes [n,c,h,w] on the device -> [n,c,H,W] as Pillow resizes mode "F" images; factors: one float per channel,
    multiplied in float32 after the resize."""
    from . import ops
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("x must be float32 [n,c,h,w], got %s %s" % (x.dtype, tuple(x.shape)))
    H, W = _size(size)
    n, c, h, w = x.shape
    _check_supported((h, w), (H, W))
    if vertical_first((h, w), (H, W)):          # Pillow's order for a tall source: the vertical pass alone, then the horizontal one
        x = ops.pil_resize_planes(x, (H, w), _axis_tables(w, w, False, x.device), _axis_tables(h, H, False, x.device))
        h = H
    xt = _axis_tables(w, W, False, x.device)
    yt = _axis_tables(h, H, False, x.device)
    return ops.pil_resize_planes(x, (H, W), xt, yt, _factor_table(factors, c, x.device))


def resize_flow(flow: torch.Tensor, size, scale_vectors: bool = True) -> torch.Tensor:
    """inference.py's resize_flow for a batch: [B,2,h,w] -> [B,2,H,W] with Pillow's BILINEAR on float planes, then u * (W / w) and
    v * (H / h) (the factor rounded to float32, the product in float32)."""
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError("flow must be [B,2,h,w], got %s" % (tuple(flow.shape),))
    H, W = _size(size)
    h, w = flow.shape[2:]
    return resize_planes(flow, (H, W), (W / w, H / h) if scale_vectors else None)


class FlowEval(NamedTuple):
    """What eval_flow hands out; members that were not asked for are None."""
    scores: Optional[torch.Tensor]       # float32 [B,2] = (EPE, Fl in percent) per sample, NaN without a valid pixel
    totals: Optional[torch.Tensor]       # int64 [B,3] = {bits of the fp64 sum of EPE, #valid, #outliers}: a view of a cached workspace
    encoded: Optional[torch.Tensor]      # torch.uint16 [B,H,W,3]: save_flow's samples
    flow: Optional[torch.Tensor]         # float32 [B,2,H,W]: resize_flow's result


def eval_flow(flow: torch.Tensor, size, gt: Optional[torch.Tensor] = None, valid: Optional[torch.Tensor] = None, gt_order: str = "kitti",
              encode: Optional[str] = None, keep_flow: bool = False, scale_vectors: bool = True, encoded_out: Optional[torch.Tensor] = None,
              flow_out: Optional[torch.Tensor] = None, scores_out: Optional[torch.Tensor] = None) -> FlowEval:
    """resize_flow with what inference.py does to its result, in the launch that makes it (ops.pil_flow_eval): [B,2,h,w] is resized
    to `size` = (H, W) and rescaled exactly as resize_flow does, and then
      gt given     -> scored: compute_epe / compute_fl of inference.py:105-159 per sample.  gt is torch.uint16 [B,H,W,3] (the PNG's
                      samples: {u, v, valid} with gt_order "kitti", what kitti.read_png16_rgb returns, or {valid, v, u} with "reference",
                      the order inference.py's own reader and save_flow use) or float32 [B,2,H,W] with `valid` None / bool / uint8 [B,H,W];
      encode given -> encoded: save_flow's uint16 samples, "reference" = {1, v, u} (inference.py:266-282), "kitti" = {u, v, 1};
      keep_flow    -> the float flow itself, bit-equal to resize_flow.
    No full-resolution float flow is written unless keep_flow asks for it.  `totals` is a view of a workspace cached per shape:
    consume it before the next call of that shape.  encoded_out / flow_out / scores_out: buffers to fill instead of new tensors
    (a captured pipeline's static outputs).  Never synchronises; capturable after `prepare(..., frames=False)` or one eager call
    per geometry.  In Pillow's vertical-first regime (`vertical_first`) the vertical pass runs as its own launch first."""
    from . import ops
    if flow.dim() != 4 or flow.shape[1] != 2 or flow.dtype != torch.float32:
        raise ValueError("flow must be float32 [B,2,h,w], got %s %s" % (flow.dtype, tuple(flow.shape)))
    if encode not in (None, "kitti", "reference"):
        raise ValueError("encode must be None, 'kitti' or 'reference', got %r" % (encode,))
    if gt is None and encode is None and not keep_flow:
        raise ValueError("nothing requested: give gt, encode or keep_flow")
    H, W = _size(size)
    B, _, h, w = flow.shape
    _check_supported((h, w), (H, W))
    dev = flow.device
    fac = _factor_table((W / w, H / h) if scale_vectors else None, 2, dev)      # from the ORIGINAL sizes, as resize_flow
    if vertical_first((h, w), (H, W)):          # Pillow's order for a tall source: the vertical pass alone, then the fused horizontal one
        flow = ops.pil_resize_planes(flow, (H, w), _axis_tables(w, w, False, dev), _axis_tables(h, H, False, dev))
        h = H
    xt = _axis_tables(w, W, False, dev)
    yt = _axis_tables(h, H, False, dev)
    if encode is not None and encoded_out is None:
        encoded_out = torch.empty((B, H, W, 3), dtype=torch.uint16, device=dev)
    if keep_flow and flow_out is None:
        flow_out = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    scores, totals = ops.pil_flow_eval(flow, (H, W), xt, yt, fac, gt=gt, valid=valid, gt_order=gt_order,
                                       enc_out=encoded_out if encode is not None else None, enc_order=encode or "reference",
                                       flow_out=flow_out if keep_flow else None, out=scores_out)
    return FlowEval(scores, totals, encoded_out if encode is not None else None, flow_out if keep_flow else None)


class FrameIngest:
    """Batches of raw uint8 frame pairs -> the normalised [B,6,h,w] network input: the frames of a batch go through a pinned host slot
    in ONE upload and ONE resize call.  Two slots alternate, so filling the next batch does not wait for the previous upload."""

    def __init__(self, size, mean=IMAGENET_MEAN, std=IMAGENET_STD, device="cuda", batch: int = 4):
        self.size = _size(size)
        self.mean, self.std = mean, std
        self.device = torch.device(device)
        self.batch = int(batch)
        if self.batch <= 0:
            raise ValueError("batch must be positive")
        self._ring = PinnedRing(2)
        self._dev = None

    def pairs(self, frames1, frames2, out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """frames1 / frames2: B host frames each ([B,H,W,3] uint8 tensor / array, or a sequence of [H,W,3]), all of one size ->
        (img1, img2), the channel halves [:, :3] and [:, 3:] of one [B,6,h,w] tensor (`img1._base`)."""
        fr = [torch.as_tensor(np.asarray(f)) if not torch.is_tensor(f) else f for f in list(frames1) + list(frames2)]
        B = len(fr) // 2
        if B == 0 or len(fr) != 2 * B or len(frames1) != B or B > self.batch:
            raise ValueError("pairs() takes 1..%d frames per side, the same number on both" % self.batch)
        H, W = fr[0].shape[:2]
        for f in fr:
            if f.dtype != torch.uint8 or tuple(f.shape) != (H, W, 3):
                raise ValueError("all frames of one call must be uint8 [%d,%d,3]; got %s %s" % (H, W, f.dtype, tuple(f.shape)))
        _check_supported((H, W), self.size)
        slot, = self._ring.acquire(((2 * self.batch, H, W, 3), torch.uint8))     # waits until the upload that last read it is done
        for j, f in enumerate(fr):
            slot[j].copy_(f)
        if self._dev is None or tuple(self._dev.shape) != tuple(slot.shape):
            self._dev = torch.empty(slot.shape, dtype=torch.uint8, device=self.device)
        dev = self._dev[:2 * B]
        dev.copy_(slot[:2 * B], non_blocking=True)
        self._ring.mark(torch.cuda.current_stream(self.device))
        h, w = self.size
        if out is None:
            out = torch.empty((B, 6, h, w), dtype=torch.float32, device=self.device)
        _resize_frames(dev, self.size, self.mean, self.std, out, None, B)
        return out[:, :3], out[:, 3:]


@torch.no_grad()
def infer_resized(model, frames1_u8: torch.Tensor, frames2_u8: torch.Tensor, image_size, mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """The loop body of inference.py:217-236 on the device: both frames [B,H,W,3] uint8 resized to image_size and normalised into
    one [B,6,h,w] input, the forward pass, and the flow resized back to (H, W) with its vectors rescaled -> [B,2,H,W]."""
    if frames1_u8.shape != frames2_u8.shape:
        raise ValueError("the two frame batches must have one shape")
    B, H, W, _ = frames1_u8.shape
    h, w = _size(image_size)
    x = torch.empty((B, 6, h, w), dtype=torch.float32, device=frames1_u8.device)
    resize_frames(frames1_u8, (h, w), mean, std, out=x[:, :3])
    resize_frames(frames2_u8, (h, w), mean, std, out=x[:, 3:])
    from .kitti import _flow_of
    return resize_flow(_flow_of(model, x), (H, W))
