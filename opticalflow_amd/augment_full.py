"""train2.py's training batches on the device: the host side of pwc_kitti_augment_full (include/pwc_hip.h, csrc/pwc_augment_full.hip).

KittiAugmentationPipeline (data_processing.py:136-279) runs per sample inside train2.py's collate_fn on the host: crop, flip, up to two
cv2.warpAffine calls over nine float planes, a brightness / contrast map and a cv2.GaussianBlur of both frames.  Here the host only
draws the per-sample parameters -- in the reference's order from NumPy's generator, so that the same `np.random.seed` gives the same
augmentation -- and the raw uint8 frames and the ground truth are uploaded as they are, in the slot layout of opticalflow_amd.augment
(`pack_slots`).  One launch per batch then writes (x, flow, mask).  cv2.getRotationMatrix2D, cv2.warpAffine and the 8U cv2.GaussianBlur
are defined by the restatements in the header; parity against an actual cv2 build is unpinned, and the blur weights are rounded from a
float64 Gaussian where OpenCV uses softdouble.

A frame smaller than the crop is a ValueError (the reference would return a short tensor that torch.stack rejects)."""
from __future__ import annotations

import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from ._args import _require_device
from .augment import invert_affine, pack_slots

# pwc_augment_full_params
FULL_PARAMS_DTYPE = np.dtype([("m", "<f8", (6,)), ("cs", "<f8", (2,)), ("gain", "<f4"), ("wk", "<u2", (7,)), ("ksize", "<u2"),
                              ("y0", "<i4"), ("x0", "<i4"), ("h", "<i4"), ("w", "<i4"), ("tx", "<i4"), ("ty", "<i4"),
                              ("flip", "<i4"), ("rot", "<i4"), ("trans", "<i4"), ("bright", "<i4"), ("blur", "<i4")])
assert FULL_PARAMS_DTYPE.itemsize == ops.AUGMENT_FULL_RECORD_BYTES
MAX_SHIFT = ops.AUGMENT_FULL_MAX_SHIFT


def rotation_matrix(center_xy, angle_deg: float) -> np.ndarray:
    """cv2.getRotationMatrix2D(center, angle, 1.0) restated in float64: [[a, b, (1-a) cx - b cy], [-b, a, b cx + (1-a) cy]] with
    a = cos(angle pi/180), b = sin(angle pi/180)."""
    rad = float(angle_deg) * (math.pi / 180.0)
    a, b = math.cos(rad), math.sin(rad)
    cx, cy = float(center_xy[0]), float(center_xy[1])
    return np.array([[a, b, (1.0 - a) * cx - b * cy], [-b, a, b * cx + (1.0 - a) * cy]], dtype=np.float64)


def gaussian_weights(sigma: float) -> Tuple[int, np.ndarray]:
    """(k, uint16 [k]): the reference's kernel size k = ceil(4 sigma) made odd, and the Q8.8 weights of OpenCV's bit-exact 8U
    GaussianBlur: the float64 kernel exp(-x^2 / (2 sigma^2)) / sum, converted from the outside in with the rounding error carried
    (v = rint(k_i 256 + err)), the centre taking what is left of 256.  OpenCV evaluates the kernel in softdouble (unpinned)."""
    sigma = float(sigma)
    k = int(math.ceil(4.0 * sigma))
    if k % 2 == 0:
        k += 1
    if not 3 <= k <= 7:
        raise ValueError("sigma %r gives a %d-tap kernel; 3, 5 and 7 taps are provided (the reference draws sigma in [0.5, 1.5))" % (sigma, k))
    r = k // 2
    e = [math.exp(-(float(i - r) ** 2) / (2.0 * sigma * sigma)) for i in range(k)]
    total = math.fsum(e)
    w = np.zeros(k, np.uint16)
    err, acc = 0.0, 0
    for i in range(r):
        adj = e[i] / total * 256.0 + err
        v = int(np.rint(adj))
        err = adj - v
        v = min(max(v, 0), 256)
        w[i] = w[k - 1 - i] = v
        acc += 2 * v
    if acc > 256:
        raise ValueError("sigma %r: the outer weights already exceed 256" % sigma)
    w[r] = 256 - acc
    return k, w


def make_full_params(n: int) -> np.ndarray:
    """n records that do nothing: identity matrix, cos 1, gain 1, the 3-tap identity blur kernel, every stage off, origin (0, 0);
    the size fields are left 0 for the caller."""
    p = np.zeros(n, dtype=FULL_PARAMS_DTYPE)
    p["m"][:, 0] = p["m"][:, 4] = 1.0
    p["cs"][:, 0] = 1.0
    p["gain"] = 1.0
    p["wk"][:, 1] = 256
    p["ksize"] = 3
    return p


def set_rotation(rec, crop_hw, angle_deg: float) -> None:
    """Switch one record's rotation on: about (crop_w // 2, crop_h // 2) as the reference, flow vectors by np.radians as the reference."""
    ch, cw = crop_hw
    rec["m"] = invert_affine(rotation_matrix((cw // 2, ch // 2), angle_deg))
    theta = np.radians(angle_deg)
    rec["cs"] = (np.cos(theta), np.sin(theta))
    rec["rot"] = 1


def set_blur(rec, sigma: float) -> None:
    k, w = gaussian_weights(sigma)
    rec["wk"] = 0
    rec["wk"][:k] = w
    rec["ksize"] = k
    rec["blur"] = 1


def sample_full_params(sizes: Sequence[Tuple[int, int]], crop_hw: Tuple[int, int] = (320, 896), augment: bool = True, rng=np.random) -> np.ndarray:
    """Per-sample records (FULL_PARAMS_DTYPE) for frames of the given (H, W), drawn from `rng` (the numpy.random module or a RandomState)
    in the order KittiAugmentationPipeline.__call__ draws: randint(0, H - ch + 1), randint(0, W - cw + 1) (both always drawn); then, if
    `augment`: rand() < 0.5 flips; rand() < 0.5 -> uniform(-17, 17) degrees; rand() < 0.5 -> randint(-10, 11) twice (tx, ty);
    rand() < 0.5 -> uniform(0.8, 1.2) twice (gain = float32 of their float64 product); rand() < 0.5 -> uniform(0.5, 1.5) sigma.
    After np.random.seed(s) the records are those of the reference's next len(sizes) samples."""
    ch, cw = int(crop_hw[0]), int(crop_hw[1])
    p = make_full_params(len(sizes))
    for rec, (H, W) in zip(p, sizes):
        H, W = int(H), int(W)
        if H < ch or W < cw:
            raise ValueError("a %dx%d frame is smaller than the %dx%d crop" % (H, W, ch, cw))
        rec["h"], rec["w"] = H, W
        rec["y0"] = rng.randint(0, H - ch + 1)
        rec["x0"] = rng.randint(0, W - cw + 1)
        if not augment:
            continue
        if rng.rand() < 0.5:
            rec["flip"] = 1
        if rng.rand() < 0.5:
            set_rotation(rec, (ch, cw), rng.uniform(-17, 17))
        if rng.rand() < 0.5:
            rec["tx"] = rng.randint(-10, 11)
            rec["ty"] = rng.randint(-10, 11)
            rec["trans"] = 1
        if rng.rand() < 0.5:
            b = rng.uniform(0.8, 1.2)
            c = rng.uniform(0.8, 1.2)
            rec["gain"] = np.float32(b * c)
            rec["bright"] = 1
        if rng.rand() < 0.5:
            set_blur(rec, rng.uniform(0.5, 1.5))
    return p


def check_full_params(params: np.ndarray, n: int, slot_hw: Tuple[int, int], crop_hw: Tuple[int, int]) -> np.ndarray:
    """The records as a contiguous FULL_PARAMS_DTYPE array after the checks the kernel repeats on the device (there a record that fails
    is answered with zeros and a status flag; here it is a ValueError before anything is uploaded)."""
    p = np.ascontiguousarray(params)
    if p.dtype != FULL_PARAMS_DTYPE or p.shape != (n,):
        raise ValueError("params must be %d records of augment_full.FULL_PARAMS_DTYPE, got %s %s" % (n, p.dtype, p.shape))
    (Hs, Ws), (ch, cw) = slot_hw, crop_hw
    for b, r in enumerate(p):
        H, W = int(r["h"]), int(r["w"])
        if not (1 <= H <= Hs and 1 <= W <= Ws):
            raise ValueError("sample %d: size %dx%d does not fit the %dx%d slot" % (b, H, W, Hs, Ws))
        if ch > H or cw > W:
            raise ValueError("sample %d: a %dx%d frame is smaller than the %dx%d crop" % (b, H, W, ch, cw))
        if not (0 <= int(r["y0"]) <= H - ch and 0 <= int(r["x0"]) <= W - cw):
            raise ValueError("sample %d: crop origin (%d, %d) outside [0, %d] x [0, %d]" % (b, r["y0"], r["x0"], H - ch, W - cw))
        if r["trans"] and (abs(int(r["tx"])) > MAX_SHIFT or abs(int(r["ty"])) > MAX_SHIFT):
            raise ValueError("sample %d: shift (%d, %d) beyond +-%d" % (b, r["tx"], r["ty"], MAX_SHIFT))
        if r["blur"]:
            k = int(r["ksize"])
            if k not in (3, 5, 7):
                raise ValueError("sample %d: blur kernel of %d taps (3, 5 or 7)" % (b, k))
            if int(r["wk"][:k].astype(np.int64).sum()) != 256:
                raise ValueError("sample %d: the %d blur weights add up to %d, not 256" % (b, k, int(r["wk"][:k].astype(np.int64).sum())))
    return p


def _params_tensor(p: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(p.view(np.uint8).reshape(p.shape[0], FULL_PARAMS_DTYPE.itemsize))


def augment_full_batch(pairs_u8: torch.Tensor, gt: torch.Tensor, valid: Optional[torch.Tensor], params: np.ndarray,
                       crop_hw: Tuple[int, int] = (320, 896), out=None, return_status: bool = False):
    """(x [n,6,ch,cw], flow [n,2,ch,cw], mask [n,1,ch,cw]) float32 on the device from slot tensors already there (layout: augment.pack_slots,
    arguments: augment.augment_batch).  params: FULL_PARAMS_DTYPE records on the host (sample_full_params), validated here and uploaded.
    The mask is fractional after a rotation, as the reference's.  return_status=True adds the kernel's int32 [n] status."""
    _require_device(pairs_u8, "pairs_u8")
    if pairs_u8.dim() != 5:
        raise ValueError("pairs_u8 must be uint8 [n,2,Hs,Ws,3], got %s" % (tuple(pairs_u8.shape),))
    n, _, Hs, Ws, _ = pairs_u8.shape
    crop_hw = (int(crop_hw[0]), int(crop_hw[1]))
    p = check_full_params(params, n, (Hs, Ws), crop_hw)
    pd = _params_tensor(p).to(pairs_u8.device, non_blocking=True)
    x, flow, m, status = ops.kitti_augment_full(pairs_u8, gt, pd, crop_hw, valid=valid, out=out)
    return (x, flow, m, status) if return_status else (x, flow, m)


class DeviceFullAugmenter:
    """train2.py's collate_fn on the device: host samples of differing sizes in, the device batch (x, flow, mask) out.  The contract is
    augment.DeviceAugmenter's: pinned staging, device slots, the parameter buffer and the outputs are allocated once; `stage` fills the
    staging memory (records drawn with sample_full_params when None), `upload` starts the copies on the current stream, `run` launches
    the kernel, allocates nothing and may be captured in a graph; `__call__` does the three.  `augment=False` draws only the crop."""

    def __init__(self, device, batch: int, max_hw: Tuple[int, int], crop_hw: Tuple[int, int] = (320, 896), gt_kind: int = 1,
                 augment: bool = True):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ops.PwcHipError("DeviceFullAugmenter needs a GPU device, got %s: there is no CPU fallback" % (self.device,))
        Hs, Ws = int(max_hw[0]), int(max_hw[1])
        ch, cw = int(crop_hw[0]), int(crop_hw[1])
        if batch < 1 or not (1 <= ch <= Hs and 1 <= cw <= Ws):
            raise ValueError("crop %dx%d does not fit the %dx%d slot (or the batch is empty)" % (ch, cw, Hs, Ws))
        if gt_kind not in (0, 1):
            raise ValueError("gt_kind must be 0 or 1, got %r" % (gt_kind,))
        self.batch, self.slot_hw, self.crop_hw, self.gt_kind, self.augment = batch, (Hs, Ws), (ch, cw), gt_kind, bool(augment)
        shapes = [((batch, 2, Hs, Ws, 3), torch.uint8),
                  ((batch, Hs, Ws, 3), torch.uint16) if gt_kind == 1 else ((batch, 2, Hs, Ws), torch.float32),
                  ((batch, Hs, Ws), torch.uint8), ((batch, FULL_PARAMS_DTYPE.itemsize), torch.uint8)]
        self._host = [torch.zeros(s, dtype=d).pin_memory() for s, d in shapes]
        self._views = [t.numpy() for t in self._host]
        self._dev = [torch.zeros(s, dtype=d, device=self.device) for s, d in shapes]
        self.x = torch.empty((batch, 6, ch, cw), dtype=torch.float32, device=self.device)
        self.flow = torch.empty((batch, 2, ch, cw), dtype=torch.float32, device=self.device)
        self.mask = torch.empty((batch, 1, ch, cw), dtype=torch.float32, device=self.device)
        self.status = torch.zeros(batch, dtype=torch.int32, device=self.device)
        self._uploaded = None
        self._n, self._with_valid = 0, False

    def stage(self, samples, params: Optional[np.ndarray] = None) -> np.ndarray:
        """Fill the pinned staging memory from the host samples and their records (drawn with sample_full_params when None)."""
        n = len(samples)
        if not 1 <= n <= self.batch:
            raise ValueError("expected 1..%d samples, got %d" % (self.batch, n))
        if self._uploaded is not None:
            self._uploaded.synchronize()           # the copy that last read the staging memory must be done before it is rewritten
            self._uploaded = None
        fr, gt, va, _ = self._views
        _, _, v, sizes = pack_slots(samples, self.slot_hw, self.gt_kind, frames=fr[:n], gt=gt[:n], valid=va[:n])
        if params is None:
            params = sample_full_params(sizes, self.crop_hw, augment=self.augment)
        p = check_full_params(params, n, self.slot_hw, self.crop_hw)
        for b, (H, W) in enumerate(sizes):
            if (int(p[b]["h"]), int(p[b]["w"])) != (H, W):
                raise ValueError("sample %d is %dx%d but its record says %dx%d" % (b, H, W, p[b]["h"], p[b]["w"]))
        np.copyto(self._views[3][:n], p.view(np.uint8).reshape(n, -1))
        self._n, self._with_valid = n, v is not None
        return p

    def upload(self) -> None:
        """Start the copies of what `stage` left to the device slots on the current stream."""
        n = self._n
        if n < 1:
            raise RuntimeError("DeviceFullAugmenter.upload before stage")
        use = (0, 1, 3) + ((2,) if self._with_valid else ())
        with torch.cuda.device(self.device):
            for i in use:
                self._dev[i][:n].copy_(self._host[i][:n], non_blocking=True)
            self._uploaded = torch.cuda.Event()
            self._uploaded.record()

    def run(self):
        """The kernel alone, on the device slots as they are, on the current stream -> (x, flow, mask) views of the n staged samples.
        Nothing is allocated, so a graph may capture it and be replayed after each stage + upload of a batch of the same n."""
        n = self._n
        if n < 1:
            raise RuntimeError("DeviceFullAugmenter.run before stage")
        fr, gt, va, pr = self._dev
        ops.kitti_augment_full(fr[:n], gt[:n], pr[:n], self.crop_hw, valid=va[:n] if self._with_valid else None,
                               out=(self.x[:n], self.flow[:n], self.mask[:n]), status=self.status[:n])
        return self.x[:n], self.flow[:n], self.mask[:n]

    def __call__(self, samples, params: Optional[np.ndarray] = None):
        self.stage(samples, params)
        self.upload()
        return self.run()
