"""KITTI evaluation path of the reference (`inference_kitti.py`), device-side.

    model_infer : cat -> replicate pad to multiples of 64 -> model -> unpad -> bilinear upsample
                  (align_corners=True) with vector rescale                (inference_kitti.py:53-91,208-224)
    metrics     : EPE and Fl-all (outlier if EPE > max(3, 0.05*|gt|))     (inference_kitti.py:94-128)
    flow PNG    : 16-bit RGB, u = (R-2^15)/64, v = (G-2^15)/64, valid = B != 0   (inference_kitti.py:23-52)
    inputs      : ToTensor + ImageNet normalisation, RGB order, NO x20     (inference_kitti.py:175-178)

Reference quirk kept on purpose: `unpad` removes the FULL-resolution pad amounts from the quarter-resolution
flow (inference_kitti.py:66-71,220), so for 1242x375 (pad 38, 9) the 320x96 flow is cropped to 282x87 before
being stretched to 1242x375.  `model_infer(..., reference_unpad=False)` crops by pad/4 instead.

`PairStream` is the config-5 ingest: uint8 pairs are staged in pinned host buffers and uploaded on a side
stream while the previous pair is being processed (double buffering); normalisation happens on the device
(2.8 MB/pair over PCIe instead of 11.2 MB as fp32).

`evaluate_stream` / `ScoredInfer` score on the device as well: the captured pipeline ends in the fused EPE / Fl-all kernel
(csrc/pwc_kitti_score.hip) instead of the upsample kernel, the ground truth travels with the images, and one [N,3] table of
raw totals is downloaded at the end.  `evaluate_pairs` is the reference's host loop.
"""
from __future__ import annotations

import functools
import os
import struct
import zlib
from typing import Iterable, Iterator, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from ._pipeline import PinnedRing, capture_graph, pad64

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


# ------------------------------------------------------------------ geometry
def pad_to_64(x: torch.Tensor) -> Tuple[torch.Tensor, int, int]:
    ph, pw = pad64(*x.shape[-2:])[2:]
    if ph == 0 and pw == 0:
        return x, 0, 0
    return F.pad(x, (0, pw, 0, ph), mode="replicate"), ph, pw


def unpad(x: torch.Tensor, pad_h: int, pad_w: int) -> torch.Tensor:
    if pad_h == 0 and pad_w == 0:
        return x
    h, w = x.shape[-2:]
    return x[..., :h - pad_h, :w - pad_w]


def flow_resize(flow: torch.Tensor, new_h: int, new_w: int) -> torch.Tensor:
    b, c, h, w = flow.shape
    if (h, w) == (new_h, new_w):
        return flow
    out = F.interpolate(flow, size=(new_h, new_w), mode="bilinear", align_corners=True)
    # python scalars, not a device tensor built per call: a pageable H2D copy here stalls the stream (measured
    # 20 ms per pair in the KITTI loop, tools/bench_kitti.py)
    out[:, 0].mul_(new_w / w)
    out[:, 1].mul_(new_h / h)
    return out


_NORM_CACHE = {}


def _norm_constants(device) -> Tuple[torch.Tensor, torch.Tensor]:
    """ImageNet mean / std as [1,3,1,1] tensors, uploaded once per device."""
    key = str(device)
    if key not in _NORM_CACHE:
        _NORM_CACHE[key] = (torch.tensor(IMAGENET_MEAN, device=device).view(1, 3, 1, 1),
                            torch.tensor(IMAGENET_STD, device=device).view(1, 3, 1, 1))
    return _NORM_CACHE[key]


def normalize_pair(img1_u8: torch.Tensor, img2_u8: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[H,W,3] (or batched [n,H,W,3]) uint8 RGB -> [1,3,H,W] ([n,3,H,W]) float, ToTensor + ImageNet normalisation
    (on the tensors' device)."""
    mean, std = _norm_constants(img1_u8.device)
    outs = []
    for im in (img1_u8, img2_u8):
        t = im[..., :3].movedim(-1, -3)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        outs.append((t.to(torch.float32) / 255.0 - mean) / std)
    return outs[0], outs[1]


def _flow_of(model, x: torch.Tensor) -> torch.Tensor:
    """The model's flow for x: the finest level, which comes first in the training tuple."""
    out = model(x)
    return out[0] if isinstance(out, (tuple, list)) else out


@torch.no_grad()
def model_infer(model, img1: torch.Tensor, img2: torch.Tensor, reference_unpad: bool = True) -> torch.Tensor:
    """img1, img2: [1,3,H,W] normalised images on the model's device -> flow [1,2,H,W] (network units, no x20)."""
    h, w = img1.shape[-2:]
    x, ph, pw = pad_to_64(torch.cat([img1, img2], dim=1))
    flow = _flow_of(model, x)
    if flow.is_cuda and flow.dtype == torch.float32:
        # unpad + bilinear resize + rescale as one kernel (the same one the captured pipeline uses; tests hold it to flow_resize)
        hq, wq = flow.shape[-2:]
        ch, cw = (hq - ph, wq - pw) if reference_unpad else (hq - ph // 4, wq - pw // 4)
        return ops.flow_upsample(flow, ch, cw, h, w)
    flow = unpad(flow, ph, pw) if reference_unpad else unpad(flow, ph // 4, pw // 4)
    return flow_resize(flow, h, w)


# ------------------------------------------------------------------ metrics (host, numpy -- like the reference)
def epe_metric(flow_pred: np.ndarray, flow_gt: np.ndarray, valid: Optional[np.ndarray]) -> float:
    d = flow_pred - flow_gt
    epe = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    if valid is not None:
        epe = epe[valid]
    return float(np.mean(epe)) if epe.size else float("nan")


def fl_all_metric(flow_pred: np.ndarray, flow_gt: np.ndarray, valid: Optional[np.ndarray]) -> float:
    d = flow_pred - flow_gt
    epe = np.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    mag = np.sqrt(flow_gt[..., 0] ** 2 + flow_gt[..., 1] ** 2)
    outlier = epe > np.maximum(3.0, 0.05 * mag)
    if valid is not None:
        outlier = outlier & valid
        denom = int(np.count_nonzero(valid))
    else:
        denom = outlier.size
    return 100.0 * float(np.count_nonzero(outlier)) / denom if denom else float("nan")


# ------------------------------------------------------------------ 16-bit flow PNG (no cv2 / 16-bit-capable PIL here)
def read_png16_rgb(path: str) -> np.ndarray:
    """Minimal PNG reader for what KITTI flow uses: colour type 2 (RGB), bit depth 16, non-interlaced -> [H,W,3] uint16."""
    data = open(path, "rb").read()
    if data[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("%s is not a PNG" % path)
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        n, = struct.unpack(">I", data[pos:pos + 4])
        kind = data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    if hdr is None:
        raise ValueError("%s: no IHDR" % path)
    w, h, depth, ctype, _, _, interlace = hdr
    if (depth, ctype, interlace) != (16, 2, 0):
        raise ValueError("%s: expected 16-bit RGB non-interlaced PNG, got depth %d type %d interlace %d" % (path, depth, ctype, interlace))
    raw = zlib.decompress(b"".join(idat))
    bpp, stride = 6, w * 6
    out = np.zeros((h, stride), dtype=np.uint8)
    prev = np.zeros(stride, dtype=np.uint8)
    p = 0
    for y in range(h):
        ft = raw[p]
        line = np.frombuffer(raw, dtype=np.uint8, count=stride, offset=p + 1).astype(np.int32)
        p += stride + 1
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        elif ft in (1, 3, 4):
            cur = np.zeros(stride, dtype=np.int32)
            pv = prev.astype(np.int32)
            for i in range(stride):                              # inherently sequential filters
                a = cur[i - bpp] if i >= bpp else 0
                b = pv[i]
                c = pv[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        else:
            raise ValueError("%s: bad filter type %d" % (path, ft))
        prev = cur.astype(np.uint8)
        out[y] = prev
    return out.reshape(h, w, 3, 2).astype(np.uint16) @ np.array([256, 1], dtype=np.uint16)


def write_png16_rgb(path: str, arr: np.ndarray) -> None:
    """[H,W,3] uint16 -> 16-bit RGB PNG (filter 0 on every row)."""
    arr = np.ascontiguousarray(arr, dtype=">u2")
    h, w, c = arr.shape
    if c != 3:
        raise ValueError("expected [H,W,3]")
    raw = b"".join(b"\x00" + arr[y].tobytes() for y in range(h))

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 16, 2, 0, 0, 0)) +
                chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def decode_flow_rgb16(arr: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """[H,W,3] uint16 (R,G,B) -> flow [H,W,2] float32, valid [H,W] bool   (inference_kitti.py:40-51)."""
    u = (arr[..., 0].astype(np.float32) - 32768.0) / 64.0
    v = (arr[..., 1].astype(np.float32) - 32768.0) / 64.0
    return np.stack([u, v], axis=-1).astype(np.float32), arr[..., 2] != 0


def encode_flow_rgb16(flow: np.ndarray, valid: Optional[np.ndarray] = None) -> np.ndarray:
    """Inverse of decode_flow_rgb16 (KITTI devkit convention: R=u, G=v, B=valid)."""
    u = np.clip(flow[..., 0] * 64.0 + 32768.0, 0, 65535).astype(np.uint16)
    v = np.clip(flow[..., 1] * 64.0 + 32768.0, 0, 65535).astype(np.uint16)
    b = np.ones(u.shape, np.uint16) if valid is None else valid.astype(np.uint16)
    return np.stack([u, v, b], axis=-1)


def load_flow_kitti_png(path: str) -> Tuple[np.ndarray, np.ndarray]:
    return decode_flow_rgb16(read_png16_rgb(path))


# ------------------------------------------------------------------ double-buffered ingest (BASELINE config 5)
def _host_u8(img) -> torch.Tensor:
    """A host image as a uint8 tensor view: cv2.imread hands the reference's loop numpy arrays (inference_kitti.py:236-237),
    the synthetic streams hand tensors; both are accepted, anything that is not uint8 [H,W,>=3] is refused."""
    t = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] < 3:
        raise ValueError("an image must be uint8 [H,W,>=3], got %s %s" % (t.dtype, tuple(t.shape)))
    return t


@functools.lru_cache(maxsize=None)
def _torch_dtype(np_dtype) -> torch.dtype:
    return torch.from_numpy(np.empty(0, np_dtype)).dtype


class _Ingest:
    """Host uint8 pairs -> device batches [n,2,H,W,3], one batch ahead of the consumer.

    Batch k+1 is copied into one of two pinned staging buffers and its upload started on a copy stream before batch k is
    handed out; the consumer's stream waits on the upload's event, and since the consumer only enqueues work (a captured
    pipeline costs 0.05 ms of host time per replay) the host runs ahead and the copies overlap the previous batch's
    kernels.  (A producer thread + queue was measured slower than this single-threaded order, 2.5 vs 1.77 ms per step.)
    A staging buffer is rewritten only after the upload that last read it has completed.  The fill is a plain memcpy per
    image (numpy.copyto: 11 MB in 0.26 ms on the GPU box); Tensor.copy_ fans a 1.4 MB image out over every OpenMP thread
    torch sees (128 on a box whose share is 16) and took 2-3 ms for the same bytes, which capped the whole stream at
    ~1000 pairs/s while the captured pipeline does 2300-3400
    (tools/bench_host_pin.py, tools/bench_kitti_parts.py)."""

    def __init__(self, pairs, device: torch.device, batch: int, n_extra: int = 0):
        self.pairs, self.device, self.batch, self.n_extra = iter(pairs), device, batch, n_extra
        self.copy_stream = torch.cuda.Stream(device=device)
        # two pinned staging slots, allocated on first use per shape: the images [batch,2,H,W,3] and, with n_extra > 0 (every item is (img1,
        # img2, e_0 .. e_{n_extra-1}), numpy arrays of one shape and dtype per k: evaluate_stream's ground truth), tensors [batch, *e_k.shape]
        self.ring, self._views = PinnedRing(2), {}

    def _fill(self):
        imgs, extras = [], []
        for item in self.pairs:
            a, b = _host_u8(item[0]), _host_u8(item[1])
            if len(item) != 2 + self.n_extra:
                raise ValueError("an item must be (img1, img2) plus %d extra arrays, got %d entries" % (self.n_extra, len(item)))
            extras.append(item[2:])
            if tuple(b.shape[:2]) != tuple(a.shape[:2]) or (imgs and tuple(a.shape[:2]) != tuple(imgs[0].shape[:2])):
                raise ValueError("a batch needs uint8 [H,W,>=3] images of one size")
            imgs += [a, b]
            if len(imgs) == 2 * self.batch:
                break
        if not imgs:
            return None
        n, (h, w) = len(imgs) // 2, imgs[0].shape[:2]
        specs = [((self.batch, 2, h, w, 3), torch.uint8)]
        specs += [((self.batch,) + e.shape, _torch_dtype(e.dtype)) for e in map(np.asarray, extras[0])]
        slot, *xslots = self.ring.acquire(*specs)  # waits until the DMA that last read this slot is done, before it is rewritten
        if slot not in self._views:                # the same memory as numpy arrays, made once per allocation (tensors hash by identity)
            if len(self._views) == 2:              # a new shape: the views of the allocations it replaces go
                self._views.clear()
            self._views[slot] = [slot.view(2 * self.batch, h, w, 3).numpy()] + [t.numpy() for t in xslots]
        views = self._views[slot]
        for i, img in enumerate(imgs):             # straight into pinned memory (an intermediate torch.stack cost 5 ms/pair)
            np.copyto(views[0][i], img.numpy()[..., :3])
        for i, ex in enumerate(extras):
            for xview, e in zip(views[1:], ex):
                np.copyto(xview[i], e, casting="no")
        with torch.cuda.stream(self.copy_stream):
            dev = slot[:n].to(self.device, non_blocking=True)
            xdev = tuple(t[:n].to(self.device, non_blocking=True) for t in xslots)
        # the slot's event: the consumer waits on it before the slot comes round again and the event is recorded anew
        return dev, self.ring.mark(self.copy_stream), xdev

    def batches_with_extra(self) -> Iterator[Tuple[torch.Tensor, Tuple[torch.Tensor, ...]]]:
        pending = self._fill()
        while pending is not None:
            dev, ev, xdev = pending
            pending = self._fill()                 # batch k+1 is staged and its upload started before batch k is consumed
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(ev)
            dev.record_stream(cur)
            for t in xdev:
                t.record_stream(cur)
            yield dev, xdev

    def batches(self) -> Iterator[torch.Tensor]:
        return (dev for dev, _ in self.batches_with_extra())


class PairStream(_Ingest):
    """Iterate device-resident normalised pairs from host uint8 pairs with upload/compute overlap (_Ingest, one pair per
    step).  ``raw=True`` yields the uploaded uint8 tensor [2,H,W,3] instead (for GraphedInfer, which normalises inside
    its HIP graph)."""

    def __init__(self, pairs: Iterable[Tuple[torch.Tensor, torch.Tensor]], device: torch.device, raw: bool = False):
        super().__init__(pairs, device, 1)
        self.raw = raw

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        for dev in self.batches():
            yield dev[0] if self.raw else normalize_pair(dev[0, 0], dev[0, 1])


class GraphedInfer:
    """normalise -> pad -> PWCDCNet -> unpad -> resize for one fixed image size as ONE HIP graph.

    At batch 1 the forward takes 2.4 ms of GPU time while the ~30 small launches of the eager pre/post-processing
    plus the graph launch cost ~4 ms of host time per pair (tools/bench_kitti.py); captured together the loop is
    GPU-bound again.  ``__call__(pair_u8)`` takes the [2,H,W,3] uint8 device tensor PairStream(raw=True) yields and
    returns the [1,2,H,W] flow (a static buffer: consume or clone it before the next call)."""

    def __init__(self, model, height: int, width: int, device: torch.device, reference_unpad: bool = True, batch: int = 1):
        self.model, self.reference_unpad, self.batch = model, reference_unpad, batch
        self.static_u8 = torch.zeros((batch, 2, height, width, 3), dtype=torch.uint8, device=device)
        self.x_in = torch.empty((batch, 6) + pad64(height, width)[:2], dtype=torch.float32, device=device)
        self._alloc_outputs(height, width, device)
        keep, model.use_graph = getattr(model, "use_graph", False), False      # no nested capture
        try:
            self.graph, self.out = capture_graph(self._body, device)           # the warm-up run builds the plan
        finally:
            model.use_graph = keep

    def _alloc_outputs(self, height: int, width: int, device) -> None:
        self.flow_full = torch.empty((self.batch, 2, height, width), dtype=torch.float32, device=device)

    def _tail(self, ch: int, cw: int, h: int, w: int) -> torch.Tensor:
        """Last kernel of the captured pipeline: quarter-resolution flow -> what the graph hands out (ScoredInfer scores here instead)."""
        return ops.flow_upsample(self.flow_quarter, ch, cw, h, w, out=self.flow_full)

    def _forward(self, x: torch.Tensor) -> torch.Tensor:
        """The model on x; its output [batch,2,H_/4,W_/4] (a static buffer like `out`) stays in ``flow_quarter`` (a sharded stream gathers it)."""
        self.flow_quarter = _flow_of(self.model, x)
        return self.flow_quarter

    def _body(self) -> torch.Tensor:
        h, w = self.static_u8.shape[2:4]
        ph, pw = pad64(h, w)[2:]
        if os.environ.get("PWC_KITTI_TORCH_PREPOST") == "1":
            # the same steps as ~30 PyTorch launches (what round 2 captured; kept for A/B runs and as the statement the kernels are tested against)
            i1, i2 = normalize_pair(self.static_u8[:, 0], self.static_u8[:, 1])
            x, ph, pw = pad_to_64(torch.cat([i1, i2], dim=1))
            self._forward(x)
            flow = unpad(self.flow_quarter, ph, pw) if self.reference_unpad else unpad(self.flow_quarter, ph // 4, pw // 4)
            return flow_resize(flow, h, w)
        # ToTensor + normalisation + cat + replicate pad as ONE kernel, unpad + bilinear resize + rescale as another (csrc/pwc_kitti.hip):
        # as PyTorch launches they were 14.6 % of the fp16 stream's GPU time
        self._forward(ops.kitti_ingest(self.static_u8, IMAGENET_MEAN, IMAGENET_STD, out=self.x_in))
        hq, wq = self.flow_quarter.shape[-2:]
        ch, cw = (hq - ph, wq - pw) if self.reference_unpad else (hq - ph // 4, wq - pw // 4)
        self.crop = (ch, cw)                       # the top-left part of flow_quarter that is stretched to (h, w)
        return self._tail(ch, cw, h, w)

    def _check_pairs(self, pairs_u8: torch.Tensor) -> int:
        """n of uint8 pairs [n<=batch,2,H,W,3] of this pipeline's size; anything else is refused."""
        n = pairs_u8.shape[0]
        if pairs_u8.dim() != 5 or tuple(pairs_u8.shape[1:]) != tuple(self.static_u8.shape[1:]) or pairs_u8.dtype != torch.uint8 \
                or not 1 <= n <= self.batch:
            raise ValueError("expected uint8 [n<=%d,%s], got %s %s" % (self.batch, ",".join(map(str, self.static_u8.shape[1:])),
                                                                      pairs_u8.dtype, tuple(pairs_u8.shape)))
        return n

    def __call__(self, pair_u8: torch.Tensor) -> torch.Tensor:
        """pair_u8: [2,H,W,3] (one pair) or [n,2,H,W,3] with n <= batch; returns the first n flows [n,2,H,W]."""
        if pair_u8.dim() == 4:
            pair_u8 = pair_u8.unsqueeze(0)
        n = self._check_pairs(pair_u8)
        self.static_u8[:n].copy_(pair_u8, non_blocking=True)
        self.graph.replay()
        return self.out[:n]


class BatchStream(_Ingest):
    """PairStream for batches: yields uint8 device tensors [n,2,H,W,3] (n = batch, fewer for the tail) from host uint8
    pairs of one size, staged in two pinned buffers and uploaded on a side stream while the previous batch computes."""

    def __iter__(self) -> Iterator[torch.Tensor]:
        return self.batches()


def evaluate_pairs(model, samples: Iterable[Tuple[torch.Tensor, torch.Tensor, np.ndarray, np.ndarray]],
                   device: torch.device, reference_unpad: bool = True):
    """samples: (img1_u8 [H,W,3], img2_u8, flow_gt [H,W,2], valid [H,W]) -> (mean EPE, mean Fl-all, per-sample list)."""
    samples = list(samples)
    stream = PairStream(((s[0], s[1]) for s in samples), device)
    rows = []
    for (i1, i2), s in zip(stream, samples):
        fp = model_infer(model, i1, i2, reference_unpad)[0].permute(1, 2, 0).cpu().numpy()
        rows.append((epe_metric(fp, s[2], s[3]), fl_all_metric(fp, s[2], s[3])))
    if not rows:
        return float("nan"), float("nan"), rows
    return float(np.nanmean([r[0] for r in rows])), float(np.nanmean([r[1] for r in rows])), rows


class ScoredInfer(GraphedInfer):
    """GraphedInfer's graph with the score kernel in place of the upsample kernel: ingest -> forward -> ops.kitti_score, for one
    fixed image size and one ground-truth form.

    gt="png16": the ground truth is the KITTI PNG samples, uint16 [n,H,W,3] (R G B, what read_png16_rgb returns; 6 B/px);
    gt="float": float32 planes [n,2,H,W] plus uint8 validity [n,H,W] (9 B/px).  The graph reads static buffers of both the
    uint8 pairs and the ground truth.  keep_flow=False (default): no full-resolution flow exists anywhere; keep_flow=True also
    fills ``flow_full`` [batch,2,H,W] (for callers who save the flow as well).  ``__call__(pairs_u8, gt, row0)`` replays the graph
    and copies the batch's raw totals {fp64 sum of EPE, int64 #valid, int64 #outliers} into rows row0.. of ``table`` (int64
    [rows,3] on the device, allocated once for the whole dataset); nothing synchronises -- download the table once at the end
    (``results()``)."""

    def __init__(self, model, height: int, width: int, device: torch.device, reference_unpad: bool = True, batch: int = 1,
                 gt: str = "png16", rows: int = 0, keep_flow: bool = False):
        if gt not in ("png16", "float"):
            raise ValueError("gt must be 'png16' or 'float', got %r" % (gt,))
        if os.environ.get("PWC_KITTI_TORCH_PREPOST") == "1":
            raise ValueError("ScoredInfer has no PyTorch pre/post-processing variant (unset PWC_KITTI_TORCH_PREPOST)")
        self.gt_form, self.keep_flow = gt, keep_flow
        if gt == "png16":
            self.static_gt = (torch.zeros((batch, height, width, 3), dtype=torch.uint16, device=device),)
        else:
            self.static_gt = (torch.zeros((batch, 2, height, width), dtype=torch.float32, device=device),
                              torch.zeros((batch, height, width), dtype=torch.uint8, device=device))
        self.table = torch.zeros((max(int(rows), batch), 3), dtype=torch.int64, device=device)
        super().__init__(model, height, width, device, reference_unpad=reference_unpad, batch=batch)

    def _alloc_outputs(self, height: int, width: int, device) -> None:
        self.flow_full = torch.empty((self.batch, 2, height, width), dtype=torch.float32, device=device) if self.keep_flow else None
        self.scores = torch.empty((self.batch, 2), dtype=torch.float32, device=device)

    def _tail(self, ch: int, cw: int, h: int, w: int) -> torch.Tensor:
        valid = self.static_gt[1] if self.gt_form == "float" else None
        _, s, nv, no = ops.kitti_score(self.flow_quarter, ch, cw, h, w, self.static_gt[0], valid=valid, flow_out=self.flow_full,
                                       out=self.scores, raw=True)
        # the three columns are views of the [batch,3] head of ops.kitti_score's cached workspace: the same memory as one int64 table
        # (the fp64 sums as their bit patterns), so the graph needs no kernel to gather them
        self.totals = torch.as_strided(nv, (self.batch, 3), (3, 1), nv.storage_offset() - 1)
        return self.scores

    def __call__(self, pairs_u8: torch.Tensor, gt, row0: int) -> torch.Tensor:
        """pairs_u8 [n<=batch,2,H,W,3] uint8 and the ground truth of those n pairs on the device (a uint16 tensor, or (flow planes,
        validity)); fills table[row0:row0+n] and returns the float32 scores [n,2] = (EPE, Fl-all) (a static buffer)."""
        gt = tuple(gt) if isinstance(gt, (tuple, list)) else (gt,)
        n = self._check_pairs(pairs_u8)
        if len(gt) != len(self.static_gt) or any(tuple(g.shape) != (n,) + tuple(st.shape[1:]) for g, st in zip(gt, self.static_gt)):
            raise ValueError("ground truth does not match the %r form %s of this pipeline" % (self.gt_form, [tuple(st.shape[1:]) for st in self.static_gt]))
        if not 0 <= row0 <= self.table.shape[0] - n:
            raise ValueError("rows %d..%d do not fit the result table of %d rows" % (row0, row0 + n, self.table.shape[0]))
        self.static_u8[:n].copy_(pairs_u8, non_blocking=True)
        for st, g in zip(self.static_gt, gt):
            st[:n].copy_(g.view(torch.uint8) if g.dtype == torch.bool else g, non_blocking=True)
        self.graph.replay()
        self.table[row0:row0 + n].copy_(self.totals[:n], non_blocking=True)
        return self.out[:n]

    def results(self, rows: Optional[int] = None):
        """ONE download of the table (this synchronises): float64 (sum_epe [rows], n_valid, n_outlier) numpy arrays."""
        tab = self.table[:rows].cpu()
        return tab[:, 0].contiguous().view(torch.float64).numpy(), tab[:, 1].numpy().astype(np.float64), tab[:, 2].numpy().astype(np.float64)


def rows_from_totals(sum_epe, n_valid, n_outlier):
    """Per-sample (EPE, Fl-all in percent) in float64 from the raw totals; (nan, nan) for a sample without a valid pixel
    (epe_metric / fl_all_metric return np.nan there)."""
    rows = []
    for s, nv, no in zip(sum_epe, n_valid, n_outlier):
        rows.append((float(s) / float(nv), 100.0 * float(no) / float(nv)) if nv else (float("nan"), float("nan")))
    return rows


def _nanmean_rows(rows):
    if all(np.isnan(r[0]) for r in rows):
        return float("nan"), float("nan")
    return float(np.nanmean([r[0] for r in rows])), float(np.nanmean([r[1] for r in rows]))


def evaluate_stream(model, samples, device: torch.device, batch: int = 16, reference_unpad: bool = True,
                    pipe: Optional["ScoredInfer"] = None):
    """evaluate_pairs without the host in the loop: samples (img1_u8 [H,W,3], img2_u8, gt) of one size, gt either the uint16
    [H,W,3] array read_png16_rgb returns or (flow [H,W,2] float32, valid [H,W] bool) -- one form per call.  Images and ground
    truth are staged together in pinned double buffers and uploaded on the copy stream; one graph replay (ScoredInfer) per batch,
    no per-batch synchronisation; ONE download of the [N,3] totals at the end, from which the per-sample EPE and Fl-all are formed
    on the host in float64.  Returns (mean EPE, mean Fl-all, rows) with evaluate_pairs' nanmean semantics.  `pipe`: a ScoredInfer
    built for this size, batch and ground-truth form to reuse (its capture costs more than a short evaluation)."""
    samples = list(samples)
    if not samples:
        return float("nan"), float("nan"), []
    png = not isinstance(samples[0][2], (tuple, list))
    h, w = _host_u8(samples[0][0]).shape[:2]
    if pipe is None:
        pipe = ScoredInfer(model, h, w, device, reference_unpad=reference_unpad, batch=batch, gt="png16" if png else "float",
                           rows=len(samples))
    elif pipe.gt_form != ("png16" if png else "float") or pipe.table.shape[0] < len(samples):
        raise ValueError("pipe was built for another ground-truth form or fewer rows")

    def items():
        for s in samples:
            if isinstance(s[2], (tuple, list)) == png:
                raise ValueError("one ground-truth form per call")
            if png:
                g = np.asarray(s[2])
                if g.dtype != np.uint16 or g.shape != (h, w, 3):
                    raise ValueError("uint16 ground truth must be [%d,%d,3], got %s %s" % (h, w, g.dtype, g.shape))
                yield s[0], s[1], g
            else:
                f, v = np.asarray(s[2][0]), np.asarray(s[2][1])
                if f.dtype != np.float32 or f.shape != (h, w, 2) or v.shape != (h, w) or v.dtype not in (np.bool_, np.uint8):
                    raise ValueError("float ground truth must be (float32 [%d,%d,2], bool [%d,%d])" % (h, w, h, w))
                yield s[0], s[1], f.transpose(2, 0, 1), v.view(np.uint8)

    row0 = 0
    for dev, gt in _Ingest(items(), device, pipe.batch, n_extra=1 if png else 2).batches_with_extra():
        pipe(dev, gt, row0)
        row0 += dev.shape[0]
    rows = rows_from_totals(*pipe.results(len(samples)))
    return _nanmean_rows(rows) + (rows,)


# ------------------------------------------------------------------ the stream sharded over the GPUs of one node
class HostBatcher:
    """BatchStream without a device: yields [n,2,H,W,3] uint8 HOST batches (CPU rehearsal of ShardedStream under gloo)."""

    def __init__(self, pairs, device, batch):
        self.pairs, self.batch = iter(pairs), batch

    def __iter__(self):
        cur = []
        for a, b in self.pairs:
            cur.append(torch.stack((a[..., :3], b[..., :3])))
            if len(cur) == self.batch:
                yield torch.stack(cur)
                cur = []
        if cur:
            yield torch.stack(cur)


class ShardedStream:
    """BASELINE configs[4]: the KITTI-shaped stream on the N GPUs of one node, one process per GPU.

    The reference loop (inference_kitti.py:227-266,296-314) takes one pair at a time on one device.  Here rank r of N
    takes pairs r, r+N, r+2N, ... of the stream (round robin: the ranks advance through the sequence together), each
    rank with its OWN pinned double buffers and copy stream (BatchStream) and its own captured pipeline (GraphedInfer);
    there is no communication inside a step.  Per step the quarter-resolution network outputs ([n,2,H_/4,W_/4],
    245 KB per 375x1242 pair instead of 3.7 MB at full resolution) are gathered to rank 0 into buffers allocated once
    (parallel.FlowGather); full-resolution flows stay on the rank that made them.

    ``infer(u8 [n,2,H,W,3]) -> (flow_full [n,2,H,W], flow_quarter [n,2,h,w])`` and ``batcher`` default to the HIP pipeline;
    the gloo test substitutes host stand-ins (the HIP forward needs a GPU)."""

    def __init__(self, device, batch: int = 1, infer=None, batcher=None, group=None, gather: bool = True):
        import torch.distributed as dist
        self.device, self.batch, self.group, self.gather = device, batch, group, gather
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        self.infer = infer
        self.batcher = batcher or BatchStream
        self._gathers = {}
        self.score_geometry = None         # for_model(score=True): (crop_h, crop_w, H, W) of the pipeline's quarter-resolution flow
        self.last_quarter = None           # ... and the quarter-resolution flows of the step run() handed out last

    @classmethod
    def for_model(cls, model, height: int, width: int, device, batch: int = 1, reference_unpad: bool = True, score: bool = False, **kw):
        """score=True lets evaluate_pairs_sharded(route="hip") score from the quarter-resolution flow (it records the crop geometry and,
        per step, that flow); the pipeline and what run() yields are the same either way."""
        pipe = GraphedInfer(model, height, width, device, reference_unpad=reference_unpad, batch=batch)

        def infer(u8):
            full = pipe(u8)
            return full, pipe.flow_quarter[:u8.shape[0]]
        self = cls(device, batch=batch, infer=infer, **kw)
        if score:
            self.score_geometry = pipe.crop + (height, width)
        return self

    def my_indices(self, n_items: int):
        return range(self.rank, n_items, self.world)

    def step_counts(self, n_items: int):
        """[steps][world] pairs each rank processes in each step (identical on every rank; rank 0 runs the most steps)."""
        per_rank = [len(range(r, n_items, self.world)) for r in range(self.world)]
        steps = -(-per_rank[0] // self.batch) if per_rank[0] else 0
        return [[max(0, min(self.batch, c - s * self.batch)) for c in per_rank] for s in range(steps)]

    def _gather(self, q: torch.Tensor, counts):
        from .parallel import FlowGather
        key = (tuple(counts), tuple(q.shape[1:]), q.dtype)
        g = self._gathers.get(key)
        if g is None:
            g = self._gathers[key] = FlowGather(list(counts), tuple(q.shape[1:]), q.dtype, q.device, 0, self.group)
        return g(q)

    def run(self, pairs):
        """pairs: a sequence of (img1_u8 [H,W,3], img2_u8) on the host.  Yields per step
        (global indices of this rank's pairs, flow_full [n,2,H,W] or None, gathered): `gathered` is, on rank 0,
        (global indices in rank-major order, quarter flows [sum n_r,2,h,w]); None elsewhere / when gather is off."""
        n_items = len(pairs)
        mine = list(self.my_indices(n_items))
        plan = self.step_counts(n_items)
        batches = iter(self.batcher((pairs[i] for i in mine), self.device, self.batch))
        tail = None
        for s, counts in enumerate(plan):
            n = counts[self.rank]
            idx = mine[s * self.batch:s * self.batch + n]
            full = quarter = None
            if n:
                full, quarter = self.infer(next(batches))
                tail = (tuple(quarter.shape[1:]), quarter.dtype, quarter.device)
            if self.score_geometry is not None:
                self.last_quarter = quarter
            gathered = None
            if self.gather and self.world > 1:
                if quarter is None:                      # a rank that ran out of pairs still joins the collective
                    if tail is None:
                        raise RuntimeError("rank %d has no pairs at all: use at most as many ranks as pairs" % self.rank)
                    quarter = torch.zeros((0,) + tail[0], dtype=tail[1], device=tail[2])
                flows = self._gather(quarter, counts)
                if self.rank == 0:
                    order = [r + self.world * (s * self.batch + k) for r in range(self.world) for k in range(counts[r])]
                    gathered = (order, flows)
            elif self.gather and n:
                gathered = (idx, quarter)
            yield idx, full, gathered


def evaluate_pairs_sharded(stream: "ShardedStream", samples, group=None, route: str = "host"):
    """inference_kitti.py:296-314 over a sharded stream: each rank scores the pairs it processed against their ground
    truth (samples[i] = (img1_u8, img2_u8, flow_gt [H,W,2], valid [H,W])); only three numbers per rank travel:
    (sum EPE, sum Fl-all, count).  Returns (mean EPE, mean Fl-all, n) on every rank.
    route="host": every full-resolution flow is downloaded and scored with NumPy (the reference's loop).  route="hip": each rank
    scores its pairs with ops.kitti_score from the quarter-resolution flow its pipeline already holds (a stream made by
    ShardedStream.for_model(..., score=True)); per rank only the [n,3] totals are downloaded, once, after the last step."""
    import torch.distributed as dist
    if route not in ("host", "hip"):
        raise ValueError("route must be 'host' or 'hip', got %r" % (route,))
    if route == "hip" and stream.score_geometry is None:
        raise ValueError("route='hip' needs a stream made by ShardedStream.for_model(..., score=True)")
    acc = torch.zeros(3, dtype=torch.float64)
    keep, stream.gather = stream.gather, False
    try:
        if route == "hip":
            ch, cw, h, w = stream.score_geometry
            totals = []
            for idx, _, _ in stream.run([(s[0], s[1]) for s in samples]):
                if not idx:
                    continue
                gt = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(samples[i][2], dtype=np.float32).transpose(2, 0, 1) for i in idx])))
                valid = torch.from_numpy(np.stack([np.asarray(samples[i][3]).astype(np.uint8) for i in idx]))
                _, s_, nv, no = ops.kitti_score(stream.last_quarter, ch, cw, h, w, gt.to(stream.device), valid=valid.to(stream.device),
                                                raw=True)
                totals.append(torch.stack((s_.view(torch.int64), nv, no), dim=1))
            if totals:
                tab = torch.cat(totals).cpu()                                  # the one download (and synchronisation) of this rank
                rows = rows_from_totals(tab[:, 0].contiguous().view(torch.float64).numpy(), tab[:, 1].numpy(), tab[:, 2].numpy())
                for e, f in rows:
                    if not (np.isnan(e) or np.isnan(f)):
                        acc += torch.tensor([e, f, 1.0], dtype=torch.float64)
        else:
            for idx, full, _ in stream.run([(s[0], s[1]) for s in samples]):
                for k, i in enumerate(idx):
                    fp = full[k].permute(1, 2, 0).cpu().numpy()
                    e, f = epe_metric(fp, samples[i][2], samples[i][3]), fl_all_metric(fp, samples[i][2], samples[i][3])
                    if not (np.isnan(e) or np.isnan(f)):
                        acc += torch.tensor([e, f, 1.0], dtype=torch.float64)
    finally:
        stream.gather = keep
    if dist.is_initialized() and stream.world > 1:
        wire = acc if dist.get_backend(group) == "gloo" else acc.to(stream.device)
        dist.all_reduce(wire, group=group)
        acc = wire.cpu()
    n = int(acc[2].item())
    return (float(acc[0] / n), float(acc[1] / n), n) if n else (float("nan"), float("nan"), 0)
