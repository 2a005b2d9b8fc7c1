"""inference.py's evaluation loop on the device (reference inference.py:194-263 `inference`, with compute_epe / compute_fl :105-159,
resize_flow :162-190 and save_flow :266-282).

The loop resizes every frame pair to the network's input with Pillow, runs the model, resizes the flow back to the original size
with Pillow, scores it against the ground truth and optionally writes it as a KITTI PNG.  `ResizedEval` is that body for one original
size as ONE captured graph -- pil_resize's frame kernel, the forward pass and the fused resize / score / encode kernel
(ops.pil_flow_eval) -- and `evaluate` is the loop: samples of mixed sizes, one pipeline per size, one 24-byte row of totals per
sample downloaded once at the end, and 6 B/px of encoded flow per sample only when files are wanted.  No full-resolution float flow
exists anywhere unless asked for.

The host functions here (`compute_epe`, `compute_fl`, `encode_flow`, `save_flow`) restate the reference's in NumPy; they are what a
port without the fused kernel would call and what the tests compare the device path with."""
from __future__ import annotations

import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import kitti, pil_resize
from ._pipeline import PinnedRing, capture_graph

ORDERS = ("reference", "kitti")
GT_FORMS = (None, "kitti", "reference", "float")


# ------------------------------------------------------------------ host restatements (no GPU needed)
def _epe_map(flow_pred: np.ndarray, flow_gt: np.ndarray) -> np.ndarray:
    d = flow_pred - flow_gt
    return np.sqrt((d * d).sum(axis=-1))


def compute_epe(flow_pred: np.ndarray, flow_gt: np.ndarray, valid_mask: np.ndarray) -> float:
    """Mean end-point error of [H,W,2] flows over the valid pixels, in the arrays' own precision; 0.0 (not NaN) for a sample without
    a valid pixel, as inference.py reports it."""
    valid_mask = np.asarray(valid_mask, bool)
    if not valid_mask.any():
        return 0.0
    return float(_epe_map(flow_pred, flow_gt)[valid_mask].mean())


def compute_fl(flow_pred: np.ndarray, flow_gt: np.ndarray, valid_mask: np.ndarray, threshold: float = 3.0,
               relative_threshold: float = 0.05) -> float:
    """Percentage of valid pixels whose end-point error exceeds both `threshold` px and `relative_threshold` x |flow_gt|; 0.0 for a
    sample without a valid pixel."""
    valid_mask = np.asarray(valid_mask, bool)
    if not valid_mask.any():
        return 0.0
    epe = _epe_map(flow_pred, flow_gt)
    mag = np.sqrt((flow_gt * flow_gt).sum(axis=-1))
    bad = (epe > threshold) & (epe > relative_threshold * mag)
    return float(bad[valid_mask].sum() / valid_mask.sum() * 100.0)


def encode_flow(flow_hw2: np.ndarray, order: str = "reference") -> np.ndarray:
    """[H,W,2] float flow -> uint16 [H,W,3], the array save_flow builds: sample = (uint16)(x * 64 + 2^15) in float32, truncated toward
    zero, with validity 1 everywhere; "reference" = {1, v, u} (save_flow's own order), "kitti" = {u, v, 1} (the devkit's R, G, B, what
    kitti.read_png16_rgb / decode_flow_rgb16 expect).  Out of range (|x| >= 512 px) the reference's cast wraps modulo 2^16 on this
    platform and is undefined in C; here, as in the kernel and in kitti.encode_flow_rgb16, the value is clamped to [0, 65535] and NaN
    gives 0."""
    if order not in ORDERS:
        raise ValueError("order must be 'reference' or 'kitti', got %r" % (order,))
    f = np.asarray(flow_hw2, np.float32)
    if f.ndim != 3 or f.shape[2] != 2:
        raise ValueError("flow must be [H,W,2], got %s" % (f.shape,))
    with np.errstate(invalid="ignore"):
        t = f * np.float32(64.0) + np.float32(32768.0)
        t = np.where(t > 0, np.minimum(t, np.float32(65535.0)), np.float32(0.0))      # NaN compares false: 0
    e = t.astype(np.int32).astype(np.uint16)
    one = np.ones(e.shape[:2], np.uint16)
    return np.stack([one, e[..., 1], e[..., 0]] if order == "reference" else [e[..., 0], e[..., 1], one], axis=-1)


def flow_filename(filename: str) -> str:
    """inference.py's name rule for a saved flow: `..._10.png` -> `..._10_flow.png` (other names are kept)."""
    return filename.replace("_10.png", "_10_flow.png")


def save_flow(flow_or_encoded: np.ndarray, output_dir: str, filename: str, order: str = "reference") -> str:
    """Write one flow as a 16-bit RGB PNG under inference.py's name rule and return the path.  Takes the float flow [H,W,2] (encoded
    here with `encode_flow`) or an already encoded uint16 [H,W,3] array (what the device hands out; `order` is then only a label).
    Unlike the reference's save_flow this one actually produces a file: the reference hands its uint16 [H,W,3] array to
    Image.fromarray, which raises TypeError for that type, so it never writes.  The file goes through kitti.write_png16_rgb and is
    read back by kitti.read_png16_rgb; with order "reference" its R, G, B are {valid, v, u}, with "kitti" the devkit's {u, v, valid}."""
    a = np.asarray(flow_or_encoded)
    if a.dtype != np.uint16:
        a = encode_flow(a, order)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError("an encoded flow must be uint16 [H,W,3], got %s" % (a.shape,))
    os.makedirs(output_dir, exist_ok=True)
    path = os.path.join(output_dir, flow_filename(filename))
    kitti.write_png16_rgb(path, a)
    return path


def rows_from_totals(sum_epe, n_valid, n_outlier) -> List[Tuple[float, float]]:
    """Per-sample (EPE, FL in percent) in float64 from the raw totals, with inference.py's (0.0, 0.0) for a sample without a valid pixel."""
    return [(float(s) / float(nv), 100.0 * float(no) / float(nv)) if nv else (0.0, 0.0) for s, nv, no in zip(sum_epe, n_valid, n_outlier)]


# ------------------------------------------------------------------ the captured pipeline of one original size
class ResizedEval:
    """inference.py's loop body for one original size (H, W) = `in_hw` and one network input `image_size` as ONE HIP graph:
    static uint8 frame pairs [2,batch,H,W,3] (all first frames, then all second frames) and ground truth -> pil_resize's frame
    kernel into [batch,6,h,w] -> the model -> pil_resize.eval_flow, which resizes the flow to (H, W) and scores / encodes it.

    gt: None (no scoring), "kitti" / "reference" (torch.uint16 [n,H,W,3] samples {u, v, valid} / {valid, v, u}) or "float" (float32
    [n,2,H,W] planes plus uint8 validity [n,H,W]).  encode: None, "reference" or "kitti" -> ``encoded`` uint16 [batch,H,W,3].
    keep_flow -> ``flow_full`` float32 [batch,2,H,W].  With gt, every replay's raw totals {fp64 sum of EPE, #valid, #outliers} go to
    rows row0.. of ``table`` (int64 [rows,3] on the device, as kitti.ScoredInfer keeps it); nothing synchronises until
    ``results()`` downloads the table once.  All outputs are static buffers: consume them before the next replay.  The scoring
    workspace behind ``totals`` is ops.pil_flow_eval's, cached per (device, batch, H, W) and so shared by every pipeline of that
    shape: run such pipelines on ONE stream (as `evaluate` does), where each replay's copy into ``table`` precedes the next replay.

    ``feed`` takes HOST frames and ground truth: they go through a two-slot PinnedRing straight into the static buffers on the
    current stream, so filling the next batch overlaps the previous replay and no device-side staging copy exists."""

    def __init__(self, model, in_hw, image_size, device, batch: int = 1, gt: Optional[str] = "kitti", encode: Optional[str] = None,
                 keep_flow: bool = False, rows: int = 0, mean=pil_resize.IMAGENET_MEAN, std=pil_resize.IMAGENET_STD):
        if gt not in GT_FORMS:
            raise ValueError("gt must be None, 'kitti', 'reference' or 'float', got %r" % (gt,))
        if encode not in (None,) + ORDERS:
            raise ValueError("encode must be None, 'reference' or 'kitti', got %r" % (encode,))
        if gt is None and encode is None and not keep_flow:
            raise ValueError("nothing requested: give gt, encode or keep_flow")
        self.model, self.device, self.batch = model, torch.device(device), int(batch)
        self.in_hw, self.image_size = pil_resize._size(in_hw), pil_resize._size(image_size)
        self.gt_form, self.encode, self.keep_flow, self.mean, self.std = gt, encode, keep_flow, mean, std
        (H, W), (h, w), dev, B = self.in_hw, self.image_size, self.device, self.batch
        if B <= 0:
            raise ValueError("batch must be positive")
        pil_resize.prepare((H, W), (h, w), dev, frames=True, mean=mean, std=std)
        pil_resize.prepare((h, w), (H, W), dev, frames=False)
        self.static_u8 = torch.zeros((2, B, H, W, 3), dtype=torch.uint8, device=dev)
        self.x_in = torch.empty((B, 6, h, w), dtype=torch.float32, device=dev)
        if gt in ("kitti", "reference"):
            self.static_gt = (torch.zeros((B, H, W, 3), dtype=torch.uint16, device=dev),)
        elif gt == "float":
            self.static_gt = (torch.zeros((B, 2, H, W), dtype=torch.float32, device=dev), torch.zeros((B, H, W), dtype=torch.uint8, device=dev))
        else:
            self.static_gt = ()
        self.encoded = torch.zeros((B, H, W, 3), dtype=torch.uint16, device=dev) if encode else None
        self.flow_full = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev) if keep_flow else None
        self.scores = torch.empty((B, 2), dtype=torch.float32, device=dev) if gt else None
        self.table = torch.zeros((max(int(rows), B), 3), dtype=torch.int64, device=dev) if gt else None
        self.totals = None
        self._ring = PinnedRing(2)
        keep, model.use_graph = getattr(model, "use_graph", False), False      # no nested capture
        try:
            self.graph, self.out = capture_graph(self._body, dev)              # the warm-up run builds the plan and the tables
        finally:
            model.use_graph = keep

    def _body(self) -> pil_resize.FlowEval:
        H, W = self.in_hw
        pil_resize._resize_frames(self.static_u8.view(2 * self.batch, H, W, 3), self.image_size, self.mean, self.std, self.x_in, None,
                                  self.batch)
        self.flow_net = kitti._flow_of(self.model, self.x_in)
        got = pil_resize.eval_flow(self.flow_net, (H, W), gt=self.static_gt[0] if self.gt_form else None,
                                   valid=self.static_gt[1] if self.gt_form == "float" else None,
                                   gt_order="reference" if self.gt_form == "reference" else "kitti", encode=self.encode,
                                   keep_flow=self.keep_flow, encoded_out=self.encoded, flow_out=self.flow_full, scores_out=self.scores)
        self.totals = got.totals
        return got

    def _check(self, n: int, gt, row0: int) -> tuple:
        gt = () if gt is None else (tuple(gt) if isinstance(gt, (tuple, list)) else (gt,))
        if not 1 <= n <= self.batch:
            raise ValueError("a call takes 1..%d pairs, got %d" % (self.batch, n))
        if len(gt) != len(self.static_gt) or any(tuple(g.shape) != (n,) + tuple(st.shape[1:]) for g, st in zip(gt, self.static_gt)):
            raise ValueError("ground truth does not match the %r form %s of this pipeline" % (self.gt_form, [tuple(st.shape[1:]) for st in self.static_gt]))
        if self.table is not None and not 0 <= row0 <= self.table.shape[0] - n:
            raise ValueError("rows %d..%d do not fit the result table of %d rows" % (row0, row0 + n, self.table.shape[0]))
        return gt

    def _replay(self, n: int, row0: int) -> pil_resize.FlowEval:
        self.graph.replay()
        if self.table is not None:
            self.table[row0:row0 + n].copy_(self.totals[:n], non_blocking=True)
        o = self.out
        return pil_resize.FlowEval(*(None if t is None else t[:n] for t in o))

    def __call__(self, frames1_u8: torch.Tensor, frames2_u8: torch.Tensor, gt=None, row0: int = 0) -> pil_resize.FlowEval:
        """frames1_u8 / frames2_u8: uint8 [n<=batch,H,W,3] on the device; gt: the ground truth of those n pairs on the device (a uint16
        tensor, or (flow planes, validity)).  Fills table[row0:row0+n] and returns the first n items of the static outputs."""
        n = frames1_u8.shape[0]
        for f in (frames1_u8, frames2_u8):
            if f.dtype != torch.uint8 or tuple(f.shape) != (n,) + tuple(self.static_u8.shape[2:]):
                raise ValueError("frames must be uint8 [n,%d,%d,3], got %s %s" % (self.in_hw + (f.dtype, tuple(f.shape))))
        gt = self._check(n, gt, row0)
        self.static_u8[0, :n].copy_(frames1_u8, non_blocking=True)
        self.static_u8[1, :n].copy_(frames2_u8, non_blocking=True)
        for st, g in zip(self.static_gt, gt):
            st[:n].copy_(g.view(torch.uint8) if g.dtype == torch.bool else g, non_blocking=True)
        return self._replay(n, row0)

    def feed(self, frames1: Sequence, frames2: Sequence, gts: Optional[Sequence] = None, row0: int = 0) -> pil_resize.FlowEval:
        """The same from HOST data: n frames per side (uint8 [H,W,3] arrays or tensors) and, with gt, n ground truths (uint16 [H,W,3],
        or (flow [H,W,2] float32, valid [H,W]) for the "float" form), staged in one pinned slot and uploaded into the static buffers."""
        n = len(frames1)
        if len(frames2) != n or (self.gt_form and (gts is None or len(gts) != n)):
            raise ValueError("feed() takes the same number of first frames, second frames and ground truths")
        if not 1 <= n <= self.batch:
            raise ValueError("a call takes 1..%d pairs, got %d" % (self.batch, n))
        if self.table is not None and not 0 <= row0 <= self.table.shape[0] - n:
            raise ValueError("rows %d..%d do not fit the result table of %d rows" % (row0, row0 + n, self.table.shape[0]))
        slot = self._ring.acquire(*[(tuple(t.shape), t.dtype) for t in (self.static_u8,) + self.static_gt])
        for j in range(n):
            slot[0][0, j].copy_(kitti._host_u8(frames1[j])[..., :3])
            slot[0][1, j].copy_(kitti._host_u8(frames2[j])[..., :3])
            if self.gt_form == "float":
                f, v = gts[j]
                slot[1][j].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(f, np.float32).transpose(2, 0, 1))))
                slot[2][j].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(v)).astype(np.uint8)))
            elif self.gt_form:
                g = np.ascontiguousarray(gts[j])
                if g.dtype != np.uint16:
                    raise ValueError("uint16 ground truth expected, got %s" % g.dtype)
                slot[1][j].copy_(torch.from_numpy(g))
        self.static_u8[:, :n].copy_(slot[0][:, :n], non_blocking=True)
        for st, s in zip(self.static_gt, slot[1:]):
            st[:n].copy_(s[:n], non_blocking=True)
        self._ring.mark(torch.cuda.current_stream(self.device))
        return self._replay(n, row0)

    def download_encoded(self, n: int) -> np.ndarray:
        """The first n encoded flows of the last replay as uint16 [n,H,W,3] on the host (6 B/px; this synchronises)."""
        if self.encoded is None:
            raise ValueError("this pipeline was built without encode")
        return self.encoded[:n].cpu().numpy()

    def results(self, rows: Optional[int] = None):
        """ONE download of the table (this synchronises): float64 (sum_epe [rows], n_valid, n_outlier) numpy arrays."""
        if self.table is None:
            raise ValueError("this pipeline was built without ground truth")
        tab = self.table[:rows].cpu()
        return tab[:, 0].contiguous().view(torch.float64).numpy(), tab[:, 1].numpy().astype(np.float64), tab[:, 2].numpy().astype(np.float64)


# ------------------------------------------------------------------ the loop
def _gt_form(gt, order: str) -> Optional[str]:
    if gt is None:
        return None
    return "float" if isinstance(gt, (tuple, list)) else order


def evaluate(model, samples, image_size=(384, 1280), batch: int = 16, output_dir: Optional[str] = None, order: str = "reference",
             device="cuda", make_pipeline: Optional[Callable] = None) -> dict:
    """inference.py's `inference()` without the host in the loop.  samples: (img1_u8 [H,W,3], img2_u8, gt or None, filename); gt is the
    uint16 [H,W,3] samples of a KITTI flow PNG in `order` ("reference" = {valid, v, u}, what inference.py's reader indexes and what
    save_flow builds; "kitti" = {u, v, valid}, what kitti.read_png16_rgb returns) or (flow [H,W,2] float32, valid [H,W]).  The
    original sizes may differ, as KITTI's do: samples are grouped by size and ground-truth form, each group runs through one
    ResizedEval in batches of `batch`, and the results are reported in input order.  With `output_dir` every sample's encoded flow
    (`order`) is downloaded and written by `save_flow`; a sample with neither ground truth nor output_dir is not run.

    Returns {'EPE', 'FL', 'num_samples', 'rows'}: plain means over the scored samples, a sample without a valid pixel counting as
    0.0 (inference.py's semantics) and samples without ground truth not counted; the three keys are absent when nothing was scored,
    as in the reference.  'rows' has one (EPE, FL) per input sample, None where there was no ground truth.  Each sample's EPE is the
    fp64 sum of its float32 per-pixel errors over #valid (the reference takes NumPy's float32 mean: the same to ~1e-7 relative);
    the counts behind FL are the reference's exactly.  make_pipeline: what builds a group's pipeline (default ResizedEval)."""
    if order not in ORDERS:
        raise ValueError("order must be 'reference' or 'kitti', got %r" % (order,))
    samples = list(samples)
    make_pipeline = make_pipeline or ResizedEval
    groups = {}
    for i, s in enumerate(samples):
        if len(s) != 4:
            raise ValueError("a sample is (img1_u8, img2_u8, gt or None, filename)")
        form = _gt_form(s[2], order)
        if form is None and output_dir is None:
            continue
        groups.setdefault((tuple(np.shape(s[0])[:2]), form), []).append(i)
    rows: List[Optional[Tuple[float, float]]] = [None] * len(samples)
    for ((H, W), form), idx in groups.items():
        pipe = make_pipeline(model, (H, W), image_size, device, batch=min(int(batch), len(idx)), gt=form,
                             encode=order if output_dir is not None else None, rows=len(idx))
        for r0 in range(0, len(idx), pipe.batch):
            part = idx[r0:r0 + pipe.batch]
            pipe.feed([samples[i][0] for i in part], [samples[i][1] for i in part], [samples[i][2] for i in part] if form else None, r0)
            if output_dir is not None:
                for i, enc in zip(part, pipe.download_encoded(len(part))):
                    save_flow(enc, output_dir, samples[i][3], order)
        if form:
            for i, row in zip(idx, rows_from_totals(*pipe.results(len(idx)))):
                rows[i] = row
    scored = [r for r in rows if r is not None]
    out = {"rows": rows}
    if scored:
        out.update(EPE=float(np.mean([r[0] for r in scored])), FL=float(np.mean([r[1] for r in scored])), num_samples=len(scored))
    return out
